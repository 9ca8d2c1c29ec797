"""Thin torch-tensor → C-ABI wrappers.  PyTorch is used for device memory and streams only; every arithmetic op below
is a hand-written gfx950 kernel in libpadt_hip.so (see include/padt_hip.h).  No fallbacks."""
import operator
import struct

import torch

from . import _lib

EPI_NONE, EPI_GELU, EPI_RESID, EPI_SWIGLU = 0, 1, 2, 3
BF16 = torch.bfloat16
F16 = torch.float16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _chk_bf16(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == BF16 and t.stride(-1) == 1, (t.dtype, t.device, t.stride())


def _x16(*ts):
    """→ the ONE 16-bit operand type (bf16 or fp16) of the given device tensors (None entries skipped); mixing them is an error."""
    dt = None
    for t in ts:
        if t is None:
            continue
        assert t.is_cuda and t.dtype in (BF16, F16) and t.stride(-1) == 1, (t.dtype, t.device, t.stride())
        assert dt is None or t.dtype == dt, ("mixed 16-bit operand types", dt, t.dtype)
        dt = t.dtype
    return dt


def _fn(name, dt):
    """The library entry point of `name` for operand type dt: the bf16 instantiation keeps the header's names, its fp16 twin replaces
    `bf16` by `f16` in the name or appends `_f16` (include/padt_hip_f16.h)."""
    lib = _lib.load()
    if dt != F16:
        return getattr(lib, name)
    return getattr(lib, name.replace("bf16", "f16") if "bf16" in name else name + "_f16")


_STREAM_SCALE = {}


def stream_scale(dt):
    """Factor between an fp32 residual stream and its 16-bit mirror of type dt (1 for bf16, 2^-4 for fp16: padt_stream_scale)."""
    if dt not in _STREAM_SCALE:
        _STREAM_SCALE[dt] = float(_lib.load().padt_stream_scale(1 if dt == F16 else 0))
    return _STREAM_SCALE[dt]


def mirror_eps(eps, dt):
    """The eps a scale-invariant consumer of a stream mirror (row_rstd, the fused RMSNorm of gemm_packed / quant_rows_fp8) must be given
    so that it returns rstd(x) / stream_scale: rsqrt(mean((s x)^2) + s^2 eps) = rstd(x) / s."""
    return float(eps) * stream_scale(dt) ** 2


GEMM_LOG = None   # bench.py sets this to a list to record (and later replay) every GEMM launch of one step


class EventTimer:
    """HIP-event brackets on the stream a kernel is launched on (bench.py's in-situ roofline: torch.cuda.Event only sees torch's current
    stream object, these see whatever stream the launch uses).  begin() / end(ev, meta) around a launch; results() → [(ms, meta)]."""

    def __init__(self):
        import ctypes
        self._ct = ctypes
        self.recs = []
        self._free = []
        self._all = []

    def _event(self):
        if self._free:
            return self._free.pop()
        ev = self._ct.c_void_p()
        _lib.check(_lib.load().padt_event_create(self._ct.byref(ev)), "padt_event_create")
        self._all.append(ev)
        return ev

    def begin(self):
        ev = self._event()
        _lib.load().padt_event_record(ev, _stream())
        return ev

    def end(self, ev0, meta):
        ev1 = self._event()
        _lib.load().padt_event_record(ev1, _stream())
        self.recs.append((ev0, ev1, meta))

    def results(self):
        out = []
        ms = self._ct.c_float()
        for ev0, ev1, meta in self.recs:
            _lib.check(_lib.load().padt_event_elapsed_ms(ev0, ev1, self._ct.byref(ms)), "padt_event_elapsed_ms")
            out.append((ms.value, meta))
            self._free += [ev0, ev1]
        self.recs = []
        return out

    def close(self):
        for ev in self._all:
            _lib.load().padt_event_destroy(ev)
        self._all, self._free, self.recs = [], [], []


class GemmProfile:
    """In-kernel timing of every tile-GEMM call (rows > 64) between start() and stop() (padt_gemm_profile): the kernels fold their first
    block start / last block end (100 MHz wall-clock ticks) into one slot per call — no event packets in the queue, nothing serialised,
    the dispatch gap in front of a kernel is not counted.  results() → [(ms, (kind, M, N, K))] in call order."""

    def __init__(self, capacity, device):
        self.cap = int(capacity)
        self.slots = torch.empty((self.cap, 2), dtype=torch.int64, device=device)
        self.meta = []

    def start(self):
        global GEMM_PROF
        if torch.cuda.is_current_stream_capturing():                 # the slot pointer would be baked into the captured graph
            raise RuntimeError("GemmProfile.start() during a stream capture")
        self.slots[:, 0] = -1                                        # 0xFFFF...: the atomicMin identity
        self.slots[:, 1] = 0
        self.meta = []
        torch.cuda.synchronize()
        _lib.load().padt_gemm_profile(self.slots.data_ptr(), self.cap)
        GEMM_PROF = self

    def stop(self):
        global GEMM_PROF
        GEMM_PROF = None
        n = _lib.load().padt_gemm_profile(None, 0)
        torch.cuda.synchronize()
        assert n == len(self.meta) or n == self.cap, (n, len(self.meta))
        return n

    def results(self):
        t = self.slots[: min(len(self.meta), self.cap)].cpu()
        ticks = (t[:, 1] - t[:, 0]).tolist()
        return [(d * 1e-5, m) for d, m in zip(ticks, self.meta)]     # 100 MHz ticks → ms


GEMM_PROF = None    # a started GemmProfile: the wrappers below append (kind, M, N, K) for every call the library gives a slot
STEP_TIMER = None   # an EventTimer: every chunk of decode-step graph replays is bracketed (llm.DecodeSession.run_steps), meta = (steps, rows)


def _tg_note(kind, M, N, K):
    if GEMM_PROF is not None and M > 64:
        GEMM_PROF.meta.append((kind, M, N, K))


def row_rstd(x, eps=1e-6, out=None):
    """fp32 rsqrt(mean(x^2) + eps) per row — feeds gemm(..., row_scale=) for an RMSNorm whose weight is folded into W."""
    M, D = x.shape
    if out is None:
        out = torch.empty((M,), device=x.device, dtype=torch.float32)
    _lib.check(_fn("padt_row_rstd", _x16(x))(_stream(), _p(x), x.stride(0), _p(out), M, D, float(eps)), "padt_row_rstd")
    return out


def gemm(a, w, bias=None, out=None, epilogue=EPI_NONE, residual=None, out_f32=False, K=None, row_scale=None):
    """out[M,N'] = epi(row_scale[m] * (a[M,K] @ w[N,K]^T) + bias).  a/w/out may be row-strided 2-D views.  N' = N/2 for SwiGLU."""
    dt = _x16(a, w, bias, residual)
    M = a.shape[0]
    N = w.shape[0]
    K = K if K is not None else a.shape[1]
    assert w.shape[1] >= K or w.shape[1] == K, (w.shape, K)
    n_out = N // 2 if epilogue == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, n_out), device=a.device, dtype=torch.float32 if out_f32 else dt)
    assert out.stride(-1) == 1 and out.shape[0] == M and out.shape[1] >= n_out and out.dtype == (torch.float32 if out_f32 else dt)
    if row_scale is not None:
        assert row_scale.dtype == torch.float32 and row_scale.numel() >= M and row_scale.is_contiguous()
    if GEMM_LOG is not None:
        GEMM_LOG.append((a, w, bias, out, epilogue, residual, out_f32, K, row_scale))
    _tg_note("gemm", M, N, K)
    _lib.check(_fn("padt_gemm_bf16", dt)(_stream(), _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0),
                                  _p(residual), residual.stride(0) if residual is not None else 0, M, N, K, epilogue,
                                  1 if out_f32 else 0, _p(row_scale)), "padt_gemm_bf16")
    return out


def gemm_resid32(a, w, bias, x32, xb=None):
    """fp32 residual stream: x32[M,N] += a @ w^T + bias (in place); xb = X(stream_scale * x32) is the next projection's A operand."""
    dt = _x16(a, w, bias, xb)
    M, K = a.shape
    N = w.shape[0]
    assert x32.dtype == torch.float32 and x32.stride(-1) == 1 and x32.shape[0] >= M and x32.shape[1] >= N
    if GEMM_LOG is not None:
        GEMM_LOG.append(("r32", a, w, bias, x32, xb))
    _tg_note("r32", M, N, K)
    _lib.check(_fn("padt_gemm_resid32", dt)(_stream(), _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(x32), x32.stride(0), _p(xb),
                                     xb.stride(0) if xb is not None else 0, M, N, K), "padt_gemm_resid32")
    return x32


def quant_rows_fp8(x, norm_eps=None, out=None, rs=None):
    """bf16 rows → (e4m3 bytes (M, K) uint8, fp32 row scales (M,)) for gemm_fp8; norm_eps: fold rsqrt(mean(x^2) + eps) into the row scale."""
    dt = _x16(x)
    M, K = x.shape
    if out is None:
        out = torch.empty((M, K), device=x.device, dtype=torch.uint8)
    if rs is None:
        rs = torch.empty((M,), device=x.device, dtype=torch.float32)
    _lib.check(_fn("padt_quant_rows_fp8", dt)(_stream(), _p(x), x.stride(0), _p(out), out.stride(0), _p(rs), M, K,
                                               -1.0 if norm_eps is None else float(norm_eps)), "padt_quant_rows_fp8")
    return out, rs


def gemm_fp8(a8, w8, col_scale, row_scale, bias=None, out=None, epilogue=EPI_NONE, x32=None, xb=None, out_dtype=BF16):
    """fp8 x fp8 MFMA GEMM (padt_gemm_fp8): a8 (M, K) / w8 (N, K) uint8 e4m3, row_scale (M,) / col_scale (N,) fp32.
    epilogue EPI_NONE / EPI_SWIGLU → bf16 `out`; EPI_RESID → x32 += ... in place (+ bf16 mirror xb)."""
    assert a8.dtype == torch.uint8 and w8.dtype == torch.uint8 and a8.stride(-1) == 1 and w8.stride(-1) == 1
    assert row_scale.dtype == torch.float32 and col_scale.dtype == torch.float32 and col_scale.is_contiguous()
    dt = _x16(bias, xb, out) or out_dtype
    M, K = a8.shape
    N = w8.shape[0]
    if epilogue == EPI_RESID:
        assert x32 is not None and x32.dtype == torch.float32 and x32.stride(-1) == 1
    else:
        n_out = N // 2 if epilogue == EPI_SWIGLU else N
        if out is None:
            out = torch.empty((M, n_out), device=a8.device, dtype=dt)
        assert _x16(out) == dt
    _tg_note("fp8", M, N, K)
    _lib.check(_fn("padt_gemm_fp8", dt)(_stream(), _p(a8), a8.stride(0), _p(w8), w8.stride(0), _p(row_scale), _p(col_scale), _p(bias), _p(out),
                                 out.stride(0) if out is not None else 0, _p(x32), x32.stride(0) if x32 is not None else 0, _p(xb),
                                 xb.stride(0) if xb is not None else 0, M, N, K, int(epilogue)), "padt_gemm_fp8")
    return x32 if epilogue == EPI_RESID else out


def gemm_knobs(mode256=-1, mf=-1, peel=-1, colsplit=-1, group_m=-1):
    """Dispatch knobs of the 256-row tile kernel (tests / tuning tools); -1 keeps a field.  Defaults: (1, 0, 1, 1, 8)."""
    _lib.check(_lib.load().padt_gemm_knobs(int(mode256), int(mf), int(peel), int(colsplit), int(group_m)), "padt_gemm_knobs")


def gemm_rope(a, w, bias, out, cos, sin, rope_cols, head_dim, row_scale=None):
    """out = rope(row_scale[m] * (a @ w^T) + bias) with the leading rope_cols columns pair-interleaved per head (see
    weights.interleave_rope_rows): the ViT qkv projection with RoPE fused into the epilogue."""
    dt = _x16(a, w, bias, out)
    M, K = a.shape
    N = w.shape[0]
    assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.stride(0) == sin.stride(0)
    if GEMM_LOG is not None:
        GEMM_LOG.append((a, w, bias, out, EPI_NONE, None, False, None, row_scale))
    _tg_note("gemm", M, N, K)
    _lib.check(_fn("padt_gemm_rope_bf16", dt)(_stream(), _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), M, N, K,
                                       _p(row_scale), _p(cos), _p(sin), cos.stride(0), int(rope_cols), int(head_dim)),
               "padt_gemm_rope_bf16")
    return out


def gemm_rmsnorm(a, w, bias=None, out=None, epilogue=EPI_NONE, eps=1e-6):
    """out = epi(rstd(a) * (a @ w^T) + bias) for decode-sized batches (rows <= 64); w carries the folded norm weight."""
    dt = _x16(a, w, bias, out)
    M, K, N = a.shape[0], a.shape[1], w.shape[0]
    n_out = N // 2 if epilogue == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, n_out), device=a.device, dtype=dt)
    _lib.check(_fn("padt_gemm_rmsnorm_bf16", dt)(_stream(), _p(a), a.stride(0), float(eps), _p(w), w.stride(0), _p(bias), _p(out),
                                          out.stride(0), M, N, K, epilogue), "padt_gemm_rmsnorm_bf16")
    return out


def pack_weight(w):
    """[N][K] row-major → MFMA-fragment-packed [N/16][K/32][4 (k-quarter)][16 (row)][8] (N, K zero-padded to 16 / 32).
    One 16x32 tile = 1 KiB in exactly the lane order of the decode kernel's weight fragment load."""
    N, K = w.shape
    Np, Kp = (N + 15) // 16 * 16, (K + 31) // 32 * 32
    if (Np, Kp) != (N, K):
        wp = w.new_zeros((Np, Kp))
        wp[:N, :K] = w
        w = wp
    return w.view(Np // 16, 16, Kp // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(Np, Kp)


def quantize_fp8_rows(w, deq_dtype=BF16):
    """Per-output-row fp8 quantisation with POWER-OF-TWO scales: → (wq uint8 OCP e4m3 bits [N][K], scale fp32 [N], w_deq bf16 [N][K]).
    scale[n] = 2^ceil(log2(max|w[n]| / 448)); e4m3 x 2^k is exactly representable in bf16, so w_deq (what prefill multiplies with and
    what the oracle sees) and scale * wq (what the decode kernel computes) are the same numbers, bit for bit."""
    wf = w.float()
    amax = wf.abs().amax(dim=1).clamp_min(1e-30)
    scale = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn)
    deq = (q.float() * scale[:, None]).to(deq_dtype)
    return q.view(torch.uint8), scale.contiguous(), deq


def pack_weight_fp8(wq):
    """uint8 e4m3 [N][K] → fp8 fragment-packed image [N/16][K/64][64 lanes][16 B] (N, K zero-padded to 16 / 64): lane fq*16 + frow holds
    row n16*16 + frow, k = kp*64 + half*32 + fq*8 + e at byte half*8 + e."""
    N, K = wq.shape
    Np, Kp = (N + 15) // 16 * 16, (K + 63) // 64 * 64
    if (Np, Kp) != (N, K):
        t = wq.new_zeros((Np, Kp))
        t[:N, :K] = wq
        wq = t
    return wq.view(Np // 16, 16, Kp // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous().view(Np, Kp)


_E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MXFP4_BLOCK = 32


def mxfp4_min_exponent(deq_dtype):
    """Smallest block exponent e for which the smallest non-zero code, 0.5 * 2^e, is exactly representable in deq_dtype: fp16 ends at its
    smallest subnormal 2^-24 (e = -23); bf16 reaches further down than E8M0 does, so the limit is E8M0 byte 1 (e = -126, whose scale is still
    a normal fp32 number)."""
    return -23 if deq_dtype == F16 else -126


def quantize_mxfp4_rows(w, deq_dtype=BF16):
    """OCP MXFP4 quantisation of a weight matrix [N][K] (K % 32 == 0): → (codes uint8 [N][K/2], exps uint8 [N][K/32] (E8M0), w_deq [N][K]
    in deq_dtype).  One block = 32 consecutive K-elements of one row, scale 2^e with e = ceil(log2(amax / 6)) — nothing saturates, the
    convention of quantize_fp8_rows with 6 in place of 448 — clamped from below to mxfp4_min_exponent(deq_dtype) (an all-zero block gets that
    minimum).  Values round to the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6} to nearest, ties to the even code; code = sign << 3 | index, a zero
    is always +0; element k of a row sits in nibble k % 2 (low first) of byte k / 2.  w_deq = sign * grid[index] * 2^e is exactly
    representable in deq_dtype: what prefill multiplies with, what the oracle sees and what the decode kernel rebuilds in registers are the
    same numbers.  |w_deq - w| <= amax_block / 5 on un-clamped blocks (worst case: 5/6 of amax at the tie 5 → 4)."""
    N, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError("quantize_mxfp4_rows: K = %d is not a multiple of the MXFP4 block (32)" % K)
    wd = w.double().view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wd.abs().amax(dim=-1)
    e_min = mxfp4_min_exponent(deq_dtype)
    e = torch.ceil(torch.log2(amax.clamp_min(1e-300) / 6.0))
    e = torch.where(amax > 6.0 * torch.exp2(e), e + 1, e)              # log2 rounded across an integer: restore e = min{e : amax <= 6 * 2^e}
    e = torch.where(amax <= 6.0 * torch.exp2(e - 1), e - 1, e)
    e = torch.where(amax > 0, e, torch.full_like(e, e_min)).clamp(e_min, 127)
    x = wd.abs() / torch.exp2(e)[..., None]                             # exact: a power-of-two scaling in double
    idx = ((x > 0.25).to(torch.uint8) + (x >= 0.75).to(torch.uint8) + (x > 1.25).to(torch.uint8) + (x >= 1.75).to(torch.uint8)
           + (x > 2.5).to(torch.uint8) + (x >= 3.5).to(torch.uint8) + (x > 5.0).to(torch.uint8))      # ties go to the even code
    neg = (wd < 0) & (idx > 0)
    nib = (idx | (neg.to(torch.uint8) << 3)).view(N, K // 2, 2)
    codes = (nib[..., 0] | (nib[..., 1] << 4)).contiguous()
    grid = torch.tensor(_E2M1_GRID, dtype=torch.float64, device=w.device)
    deq = torch.where(neg, -1.0, 1.0) * grid[idx.long()] * torch.exp2(e)[..., None]
    return codes, (e + 127).to(torch.uint8).contiguous(), deq.view(N, K).to(deq_dtype)


def dequantize_mxfp4(codes, exps):
    """(codes [N][K/2], exps [N][K/32]) → fp64 [N][K]: sign * grid[index] * 2^(exps - 127), the statement of the format."""
    N, K = codes.shape[0], codes.shape[1] * 2
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).view(N, K)
    grid = torch.tensor(_E2M1_GRID, dtype=torch.float64, device=codes.device)
    v = grid[(nib & 7).long()] * torch.where((nib & 8) != 0, -1.0, 1.0)
    return (v.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * torch.exp2(exps.double() - 127)[..., None]).view(N, K)


def pack_weight_fp4(codes, exps):
    """(codes uint8 [N][K/2], exps uint8 [N][K/32]) → the decode image (nibbles uint8 [Np][Kp/2], exponents uint8 [Np/16][Kp/64][16][2]), N
    and K zero-padded to 16 / 64 (zero codes; padded exponents are 127 = 2^0).  Nibbles: [Np/16][Kp/64][64 lanes][8 B], lane fq*16 + frow
    holds row n16*16 + frow, k = kp*64 + half*32 + fq*8 + j in nibble j % 2 of byte half*4 + j/2 — the lane's fragment of K-step 2kp, then of
    2kp + 1; the exponent of (row, K-step) sits at [n16][kp][frow][half]."""
    N, K2 = codes.shape
    K = K2 * 2
    assert exps.shape == (N, K // MXFP4_BLOCK), (codes.shape, exps.shape)
    Np, Kp = (N + 15) // 16 * 16, (K + 63) // 64 * 64
    if (Np, Kp) != (N, K):
        c, e = codes.new_zeros((Np, Kp // 2)), exps.new_full((Np, Kp // MXFP4_BLOCK), 127)
        c[:N, :K2] = codes
        e[:N, :K // MXFP4_BLOCK] = exps
        codes, exps = c, e
    img = codes.view(Np // 16, 16, Kp // 64, 2, 4, 4).permute(0, 2, 4, 1, 3, 5).contiguous().view(Np, Kp // 2)
    return img, exps.view(Np // 16, 16, Kp // 64, 2).permute(0, 2, 1, 3).contiguous()


def unpack_weight_fp4(img, exps_packed, N, K):
    """Inverse of pack_weight_fp4 → (codes [N][K/2], exps [N][K/32])."""
    Np, Kp = img.shape[0], img.shape[1] * 2
    codes = img.view(Np // 16, Kp // 64, 4, 16, 2, 4).permute(0, 3, 1, 4, 2, 5).contiguous().view(Np, Kp // 2)
    exps = exps_packed.permute(0, 2, 1, 3).contiguous().view(Np, Kp // MXFP4_BLOCK)
    return codes[:N, :K // 2].contiguous(), exps[:N, :K // MXFP4_BLOCK].contiguous()


def new_splitk_workspace(n, split_k, device):
    """Zero-initialised split-K workspace (ticket header must start at zero), one per concurrently decoding stream."""
    return torch.zeros(_lib.load().padt_gemm_splitk_workspace(n, split_k), dtype=torch.uint8, device=device)


def pack_rows(src, dst, M, to_packed=True):
    """Row-major (M, K) <-> 16-row fragment-packed activation layout (buffers hold whole 16-row blocks)."""
    K = src.shape[1]
    _lib.check(_lib.load().padt_pack_rows(_stream(), _p(src), src.stride(0), _p(dst), dst.stride(0), M, K, 1 if to_packed else 0),
               "padt_pack_rows")
    return dst


def gemm_packed(a, wp, n, bias=None, out=None, epilogue=EPI_NONE, residual=None, norm_eps=None, split_k=1, workspace=None,
                a_packed=False, c_packed=False, rows=None, scales=None, exps=None):
    """Decode-step projection over a pack_weight() image (rows <= 128): out = epi(rstd?(a) * (a @ w^T) + bias).
    a_packed / c_packed: a / (out and residual) are fragment-packed activation buffers holding `rows` valid rows.
    scales given: wp is the fp8 image (pack_weight_fp8) and out = epi(rstd?(a) * scales[n] * (a @ wq^T) + bias).
    exps given: wp is the MXFP4 nibble image and exps its block exponents (pack_weight_fp4): gemm_packed_fp4."""
    if exps is not None:
        assert scales is None
        return gemm_packed_fp4(a, wp, exps, n, bias=bias, out=out, epilogue=epilogue, residual=residual, norm_eps=norm_eps, split_k=split_k,
                               workspace=workspace, a_packed=a_packed, c_packed=c_packed, rows=rows)
    if scales is None:
        dt, name = _x16(a, wp, bias, residual, out), "padt_gemm_packed_bf16"
    else:
        assert wp.dtype == torch.uint8 and scales.dtype == torch.float32 and scales.is_contiguous()
        dt, name = _x16(a, bias, residual, out), "padt_gemm_packed_fp8"
    M, K = a.shape
    if rows is not None:
        M = rows
    n_out = n // 2 if epilogue == EPI_SWIGLU else n
    if out is None:
        out = torch.empty((M, n_out), device=a.device, dtype=dt)
    sc = () if scales is None else (_p(scales),)
    _lib.check(_fn(name, dt)(_stream(), _p(a), a.stride(0), _p(wp), wp.shape[1], *sc, _p(bias), _p(out), out.stride(0),
                             _p(residual), residual.stride(0) if residual is not None else 0, M, n, K, epilogue,
                             -1.0 if norm_eps is None else float(norm_eps), int(split_k), _p(workspace),
                             (1 if a_packed else 0) | (2 if c_packed else 0)), name)
    return out


def gemm_packed_fp8(a, wq_packed, scales, n, *args, **kw):
    """gemm_packed over an fp8 image (pack_weight_fp8) and its per-row scales."""
    return gemm_packed(a, wq_packed, n, *args, scales=scales, **kw)


def gemm_packed_resid32(a, wp, n, x32, xb_packed, scales=None, split_k=1, workspace=None, a_packed=True, rows=None, exps=None):
    """Decode-step residual projection over the fp32 stream: x32[rows, n] += scales?[n] * (a @ w^T) in place, xb_packed = bf16(x32) in the
    fragment-packed activation layout.  wp: pack_weight() image, or with scales the fp8 image, or with exps the MXFP4 image."""
    if exps is not None:
        assert scales is None
        return gemm_packed_resid32_fp4(a, wp, exps, n, x32, xb_packed, split_k=split_k, workspace=workspace, a_packed=a_packed, rows=rows)
    dt = _x16(a, xb_packed, None if scales is not None else wp)
    M, K = a.shape
    if rows is not None:
        M = rows
    assert x32.dtype == torch.float32 and x32.stride(-1) == 1 and (scales is None or scales.dtype == torch.float32)
    _lib.check(_fn("padt_gemm_packed_resid32", dt)(_stream(), _p(a), a.stride(0), _p(wp), wp.shape[1], _p(scales), _p(x32), x32.stride(0),
                                            _p(xb_packed), xb_packed.stride(0), M, n, K, int(split_k), _p(workspace), 1 if a_packed else 0),
               "padt_gemm_packed_resid32")
    return x32


def _chk_fp4(wq, exps):
    assert wq.dtype == torch.uint8 and exps.dtype == torch.uint8 and wq.is_cuda and exps.is_cuda and wq.is_contiguous() and exps.is_contiguous()
    assert exps.numel() * 16 == wq.numel(), "exponents do not belong to this nibble image"     # 2 bytes per 16 rows x 64 elements / 16 = 32 B per 512 B


def gemm_packed_fp4(a, wq, exps, n, bias=None, out=None, epilogue=EPI_NONE, residual=None, norm_eps=None, split_k=1, workspace=None,
                    a_packed=False, c_packed=False, rows=None):
    """gemm_packed over an MXFP4 image (pack_weight_fp4: nibbles + block exponents): out = epi(rstd?(a) * (a @ w_deq^T) + bias), bit for bit
    what gemm_packed gives on pack_weight(w_deq)."""
    _chk_fp4(wq, exps)
    dt = _x16(a, bias, residual, out)
    M, K = a.shape
    if rows is not None:
        M = rows
    n_out = n // 2 if epilogue == EPI_SWIGLU else n
    if out is None:
        out = torch.empty((M, n_out), device=a.device, dtype=dt)
    _lib.check(_fn("padt_gemm_packed_fp4", dt)(_stream(), _p(a), a.stride(0), _p(wq), wq.shape[1] * 2, _p(exps), _p(bias), _p(out), out.stride(0),
                                               _p(residual), residual.stride(0) if residual is not None else 0, M, n, K, epilogue,
                                               -1.0 if norm_eps is None else float(norm_eps), int(split_k), _p(workspace),
                                               (1 if a_packed else 0) | (2 if c_packed else 0)), "padt_gemm_packed_fp4")
    return out


def gemm_packed_resid32_fp4(a, wq, exps, n, x32, xb_packed, split_k=1, workspace=None, a_packed=True, rows=None):
    """gemm_packed_resid32 over an MXFP4 image: x32[rows, n] += a @ w_deq^T in place, xb_packed = X(x32) in the packed activation layout."""
    _chk_fp4(wq, exps)
    dt = _x16(a, xb_packed)
    M, K = a.shape
    if rows is not None:
        M = rows
    assert x32.dtype == torch.float32 and x32.stride(-1) == 1
    _lib.check(_fn("padt_gemm_packed_resid32_fp4", dt)(_stream(), _p(a), a.stride(0), _p(wq), wq.shape[1] * 2, _p(exps), _p(x32), x32.stride(0),
                                                       _p(xb_packed), xb_packed.stride(0), M, n, K, int(split_k), _p(workspace),
                                                       1 if a_packed else 0), "padt_gemm_packed_resid32_fp4")
    return x32


def attn_varlen(q, k, v, out, cu_q, cu_k, max_seqlen_q, n_heads, n_kv_heads, head_dim, causal=False, scale=None, rope=None):
    """q/k/v/out: 2-D (tokens, row) bf16 views whose row holds the heads contiguously; cu_*: int32 device tensors.
    rope=(cos, sin) fp32 [tokens][>= head_dim/2]: rotate q and k inside the kernel (self-attention, max_seqlen_q < 256)."""
    dt = _x16(q, k, v, out)
    assert cu_q.dtype == torch.int32 and cu_k.dtype == torch.int32
    nseg = cu_q.numel() - 1
    scale = head_dim ** -0.5 if scale is None else scale
    _lib.check(_fn("padt_attn_varlen", dt)(_stream(), _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out),
                                    out.stride(0), _p(cu_q), _p(cu_k), nseg, int(max_seqlen_q), n_heads, n_kv_heads,
                                    head_dim, float(scale), 1 if causal else 0, _p(rope[0]) if rope else 0,
                                    _p(rope[1]) if rope else 0, rope[0].stride(0) if rope else 0), "padt_attn_varlen")
    return out


def decode_attn_workspace(batch, n_kv_heads, head_dim, s_max):
    return _lib.load().padt_decode_attn_workspace(batch, n_kv_heads, head_dim, s_max)


def new_decode_workspace(batch, n_kv_heads, head_dim, s_max, device):
    """Split-attention partials; one per stream that decodes concurrently."""
    return torch.zeros(decode_attn_workspace(batch, n_kv_heads, head_dim, s_max), dtype=torch.uint8, device=device)


def decode_attn(q, k_cache, vt_cache, lens, out, workspace, n_heads, n_kv_heads, head_dim, s_max, max_len, scale=None):
    dt = _x16(q, k_cache, vt_cache, out)
    scale = head_dim ** -0.5 if scale is None else scale
    _lib.check(_fn("padt_decode_attn", dt)(_stream(), _p(q), _p(k_cache), _p(vt_cache), _p(lens), _p(out), _p(workspace),
                                    q.shape[0], n_heads, n_kv_heads, head_dim, s_max, int(max_len), float(scale)),
               "padt_decode_attn")
    return out


def rope_table(pos3, inv_freq, out, head_dim, sections):
    lib = _lib.load()
    assert pos3.dtype == torch.int32 and out.dtype == torch.float32
    _lib.check(lib.padt_rope_table(_stream(), _p(pos3), _p(inv_freq), _p(out), pos3.shape[1], head_dim, sections[0], sections[1]),
               "padt_rope_table")
    return out


def decode_attn_rope(qkv, rope_cs, slot, k_cache, vt_cache, out, workspace, n_heads, n_kv_heads, head_dim, s_max, max_len,
                     scale=None, out_packed=False, cache_packed=False):
    """cache_packed: k_cache / vt_cache hold the fragment-packed images (pack_k_cache / pack_vt_cache, written by llm_qkv_post(cache_packed=True))
    → the one-launch kernel (no workspace needed); 2 / 3 force one / two blocks per (kv head, sample) (True = 1: chosen from Hkv x batch)."""
    dt = _x16(qkv, k_cache, vt_cache, out)
    scale = head_dim ** -0.5 if scale is None else scale
    _lib.check(_fn("padt_decode_attn_rope", dt)(_stream(), _p(qkv), qkv.stride(0), _p(rope_cs), _p(slot), _p(k_cache), _p(vt_cache),
                                         _p(out), _p(workspace), qkv.shape[0], n_heads, n_kv_heads, head_dim, s_max,
                                         int(max_len), float(scale), 1 if out_packed else 0, int(cache_packed)), "padt_decode_attn_rope")
    return out


def pack_k_cache(kc):
    """Row-major K cache (B, Hkv, S, D) → the fragment-packed image [S/16][D/32][fq 4][frow 16][8] (same shape, padt_decode_attn_rope)."""
    B, G, S, D = kc.shape
    return kc.view(B, G, S // 16, 16, D // 32, 4, 8).permute(0, 1, 2, 4, 5, 3, 6).contiguous().view(B, G, S, D)


def unpack_k_cache(kp):
    B, G, S, D = kp.shape
    return kp.view(B, G, S // 16, D // 32, 4, 16, 8).permute(0, 1, 2, 5, 3, 4, 6).reshape(B, G, S, D)


def pack_vt_cache(vt):
    """Transposed V cache (B, Hkv, D, S) → the fragment-packed image [D/16][S/32][fq 4][frow 16][run 2][4] (same shape)."""
    B, G, D, S = vt.shape
    return vt.view(B, G, D // 16, 16, S // 32, 2, 4, 4).permute(0, 1, 2, 4, 6, 3, 5, 7).contiguous().view(B, G, D, S)


def unpack_vt_cache(vp):
    B, G, D, S = vp.shape
    return vp.view(B, G, D // 16, S // 32, 4, 16, 2, 4).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(B, G, D, S)


def rmsnorm(x, w, out=None, eps=1e-6, add=None, add_div=1, D=None, gelu=False):
    dt = _x16(x, w, add, out)
    D = D if D is not None else x.shape[1]
    if out is None:
        out = torch.empty((x.shape[0], D), device=x.device, dtype=dt)
    _lib.check(_fn("padt_rmsnorm", dt)(_stream(), _p(x), x.stride(0), _p(add), add.stride(0) if add is not None else 0, add_div,
                                _p(w), _p(out), out.stride(0), x.shape[0], D, float(eps), 1 if gelu else 0), "padt_rmsnorm")
    return out


def layernorm(x, w, b, out=None, eps=1e-5):
    dt = _x16(x, w, b, out)
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_fn("padt_layernorm", dt)(_stream(), _p(x), x.stride(0), _p(w), _p(b), _p(out), out.stride(0), x.shape[0],
                                  x.shape[1], float(eps)), "padt_layernorm")
    return out


def rope_half_(x, cos, sin, n_heads, head_dim):
    """in place on the first n_heads*head_dim columns of x (T, row)."""
    dt = _x16(x)
    assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.stride(-1) == 1 and sin.stride() == cos.stride()
    _lib.check(_fn("padt_rope_half", dt)(_stream(), _p(x), x.stride(0), _p(cos), _p(sin), cos.stride(0), x.shape[0], n_heads,
                                  head_dim), "padt_rope_half")
    return x


def gather_rows(src, idx, out=None, D=None):
    lib = _lib.load()
    assert idx.dtype == torch.int32 and src.stride(-1) == 1
    D = D if D is not None else src.shape[1]
    n = idx.numel()
    if out is None:
        out = torch.empty((n, D), device=src.device, dtype=src.dtype)
    if src.dtype in (BF16, F16):                                     # a 16-byte-vector copy: the operand type does not matter
        assert out.dtype == src.dtype
        _lib.check(lib.padt_gather_rows(_stream(), _p(src), src.stride(0), _p(idx), _p(out), out.stride(0), n, D),
                   "padt_gather_rows")
    elif src.dtype == torch.float32:
        _lib.check(lib.padt_gather_rows_f32(_stream(), _p(src), src.stride(0), _p(idx), _p(out), out.stride(0), n, D),
                   "padt_gather_rows_f32")
    else:
        raise TypeError(src.dtype)
    return out


def add_rows(a, b, out=None):
    dt = _x16(a, b, out)
    if out is None:
        out = torch.empty_like(a)
    _lib.check(_fn("padt_add_rows", dt)(_stream(), _p(a), a.stride(0), _p(b), b.stride(0), b.shape[0], _p(out), out.stride(0),
                                 a.shape[0], a.shape[1]), "padt_add_rows")
    return out


def cast_f32_x16(x, D_pad=None, out=None, dtype=BF16, scale=1.0):
    """out = X(scale * x) for fp32 rows x, X = dtype (or out's); scale = stream_scale(dtype) writes the mirror of an fp32 residual stream."""
    assert x.dtype == torch.float32 and x.stride(-1) == 1
    D = x.shape[1]
    D_pad = D_pad or D
    if out is None:
        out = torch.empty((x.shape[0], D_pad), device=x.device, dtype=dtype)
    dt = _x16(out)
    _lib.check(_fn("padt_cast_f32_bf16", dt)(_stream(), _p(x), x.stride(0), _p(out), out.stride(0), x.shape[0], D, D_pad, float(scale)),
               "padt_cast_f32_bf16")
    return out


def cast_f32_bf16(x, D_pad=None, out=None):
    return cast_f32_x16(x, D_pad, out, BF16)


def cast_x16_f32(x, out=None):
    dt = _x16(x)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    _lib.check(_fn("padt_cast_bf16_f32", dt)(_stream(), _p(x), x.stride(0), _p(out), out.stride(0), x.shape[0], x.shape[1]), "padt_cast_bf16_f32")
    return out


cast_bf16_f32 = cast_x16_f32


def rmsnorm_f32(x32, w, out=None, eps=1e-6):
    """bf16 RMSNorm of fp32 rows (the norms that read the fp32 residual stream)."""
    dt = _x16(w, out)
    assert x32.dtype == torch.float32 and x32.stride(-1) == 1
    if out is None:
        out = torch.empty(x32.shape, device=x32.device, dtype=dt)
    _lib.check(_fn("padt_rmsnorm_f32", dt)(_stream(), _p(x32), x32.stride(0), _p(w), _p(out), out.stride(0), x32.shape[0], x32.shape[1], float(eps)),
               "padt_rmsnorm_f32")
    return out


_KIND = {torch.float32: 0, BF16: 1, F16: 2}


def check_finite(x, flags, rows_per_flag=None, rows=None):
    """flags[row // rows_per_flag] |= 1 (int32 device tensor, caller zeroes it) for every row of the 2-D tensor x that holds +-inf or NaN
    (padt_check_finite: the fp16-operand safety net).  rows_per_flag None → one flag for the whole tensor."""
    assert x.is_cuda and x.dim() == 2 and x.stride(1) == 1 and x.dtype in _KIND, (x.dtype, x.shape, x.stride())
    assert flags.dtype == torch.int32 and flags.is_cuda and flags.is_contiguous()
    rows = x.shape[0] if rows is None else int(rows)
    rpf = max(rows, 1) if rows_per_flag is None else int(rows_per_flag)
    assert flags.numel() >= (rows + rpf - 1) // rpf
    _lib.check(_lib.load().padt_check_finite(_stream(), _p(x), x.stride(0), rows, x.shape[1], _KIND[x.dtype], _p(flags), rpf), "padt_check_finite")
    return flags


def sigmoid_f32_(x):
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.is_contiguous()
    _lib.check(lib.padt_sigmoid_f32(_stream(), _p(x), x.numel()), "padt_sigmoid_f32")
    return x


def embed_tokens(ids, img_index, table, proto, image_embeds, out=None, err_flag=None):
    lib = _lib.load()
    dt = _x16(table, proto, image_embeds, out)                       # rows are copied: one entry point serves both operand types
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    T, D = ids.numel(), table.shape[1]
    if out is None:
        out = torch.empty((T, D), device=table.device, dtype=dt)
    _lib.check(lib.padt_embed_tokens(_stream(), _p(ids), _p(img_index), _p(table), _p(proto), _p(image_embeds), _p(out),
                                     T, table.shape[0], 0 if proto is None else proto.shape[0], D, _p(err_flag)),
               "padt_embed_tokens")
    return out


def llm_qkv_post(qkv, pos3, inv_freq, q_out, k_cache, vt_cache, n_heads, n_kv_heads, head_dim, s_max, sections,
                 sample=None, slot=None, lens=None, k_pack=None, cache_packed=False):
    dt = _x16(qkv, q_out, k_cache, vt_cache, k_pack)
    assert pos3.dtype == torch.int32 and pos3.is_contiguous() and inv_freq.dtype == torch.float32
    _lib.check(_fn("padt_llm_qkv_post", dt)(_stream(), _p(qkv), qkv.stride(0), _p(pos3), _p(sample), _p(slot), _p(lens),
                                     _p(inv_freq), _p(q_out), q_out.stride(0), _p(k_pack),
                                     k_pack.stride(0) if k_pack is not None else 0, _p(k_cache), _p(vt_cache),
                                     qkv.shape[0], n_heads, n_kv_heads, head_dim, s_max, sections[0], sections[1], 1 if cache_packed else 0),
               "padt_llm_qkv_post")


def llm_qkv_post_shared(qkv, pos3, inv_freq, q_out, k_cache, vt_cache, k_join, v_join, dst_off, dst_sample, dst_slot, dst_row,
                        n_heads, n_kv_heads, head_dim, s_max, sections, cache_packed=False):
    """llm_qkv_post with fan-out (padt_llm_qkv_post_shared): token t's roped K / V go to the cache images (session row dst_sample[n], slot
    dst_slot[n]) and join-buffer rows dst_row[n] of every n in [dst_off[t], dst_off[t+1]); a destination out of range is skipped."""
    dt = _x16(qkv, q_out, k_cache, vt_cache, k_join, v_join)
    T = qkv.shape[0]
    assert pos3.dtype == torch.int32 and pos3.is_contiguous() and pos3.shape == (3, T) and inv_freq.dtype == torch.float32
    assert qkv.shape[1] == (n_heads + 2 * n_kv_heads) * head_dim and q_out.shape == (T, n_heads * head_dim)
    assert k_join.shape == v_join.shape and k_join.shape[1] == n_kv_heads * head_dim
    assert k_cache.is_contiguous() and vt_cache.is_contiguous() and k_cache.numel() == vt_cache.numel()
    assert k_cache.numel() % (n_kv_heads * s_max * head_dim) == 0
    batch = k_cache.numel() // (n_kv_heads * s_max * head_dim)
    for t in (dst_off, dst_sample, dst_slot, dst_row):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
    assert dst_off.numel() == T + 1 and dst_sample.numel() == dst_slot.numel() == dst_row.numel()
    # no alignment assertion: on a base that is not 16-byte aligned the entry point takes the kernel's scalar branch (same bits)
    _lib.check(_fn("padt_llm_qkv_post_shared", dt)(_stream(), _p(qkv), qkv.stride(0), _p(pos3), _p(inv_freq), _p(q_out), q_out.stride(0),
                                            _p(k_join), k_join.stride(0), _p(v_join), v_join.stride(0), k_join.shape[0], _p(k_cache),
                                            _p(vt_cache), _p(dst_off), _p(dst_sample), _p(dst_slot), _p(dst_row), T, n_heads, n_kv_heads,
                                            head_dim, s_max, batch, sections[0], sections[1], 1 if cache_packed else 0),
               "padt_llm_qkv_post_shared")


def kv_prefix_fanout(k_pre, v_pre, pre_off, mem_image, mem_row, mem_join, max_p, k_cache, vt_cache, k_join, v_join, n_kv_heads, head_dim,
                     s_max, cache_packed=False):
    """Cached prompt-prefix rows → cache images and join rows (padt_kv_prefix_fanout): k_pre / v_pre (n_pre, Hkv * D) are one layer's roped
    K rows / V rows of the prefixes, image u at rows [pre_off[u], pre_off[u+1]); member m = (mem_image[m], mem_row[m], mem_join[m]) gets
    them at slots [0, P) of session row mem_row[m] and join rows [mem_join[m], mem_join[m] + P).  max_p: the longest prefix (host int)."""
    dt = _x16(k_pre, v_pre, k_cache, vt_cache, k_join, v_join)
    kv = n_kv_heads * head_dim
    assert k_pre.shape == v_pre.shape and k_pre.dim() == 2 and k_pre.shape[1] == kv and k_pre.stride(1) == v_pre.stride(1) == 1
    assert k_pre.stride(0) == v_pre.stride(0)
    assert k_join.shape == v_join.shape and k_join.shape[1] == kv and k_join.stride(1) == v_join.stride(1) == 1
    assert k_cache.is_contiguous() and vt_cache.is_contiguous() and k_cache.numel() == vt_cache.numel()
    assert k_cache.numel() % (kv * s_max) == 0
    batch = k_cache.numel() // (kv * s_max)
    for t in (pre_off, mem_image, mem_row, mem_join):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
    assert pre_off.numel() >= 2 and mem_image.numel() == mem_row.numel() == mem_join.numel()
    # no alignment assertion: on a base that is not 16-byte aligned the entry point takes the kernel's scalar branch (same bits)
    _lib.check(_fn("padt_kv_prefix_fanout", dt)(_stream(), _p(k_pre), _p(v_pre), k_pre.stride(0), k_pre.shape[0], _p(pre_off), pre_off.numel() - 1,
                                                _p(mem_image), _p(mem_row), _p(mem_join), mem_image.numel(), int(max_p), _p(k_cache), _p(vt_cache),
                                                _p(k_join), k_join.stride(0), _p(v_join), v_join.stride(0), k_join.shape[0], n_kv_heads, head_dim,
                                                s_max, batch, 1 if cache_packed else 0),
               "padt_kv_prefix_fanout")


def mask_scatter(e2, mask_tok, cu_patch, obj_w, masks, n_obj, total_patches, dm):
    lib = _lib.load()
    _chk_bf16(e2, mask_tok)
    assert masks.dtype == torch.float32 and masks.is_contiguous()
    _lib.check(lib.padt_mask_scatter(_stream(), _p(e2), e2.stride(0), _p(mask_tok), mask_tok.stride(0), _p(cu_patch),
                                     _p(obj_w), _p(masks), n_obj, total_patches, masks.shape[1], masks.shape[2], dm),
               "padt_mask_scatter")
    return masks


def vrt_head_nblk(vocab, n_proto):
    return _lib.load().padt_vrt_head_nblk(vocab, n_proto)


def _head_call(name, hidden, table, proto, vrt_off, part_val, part_idx, eos, mode_table, step, logits, table_packed, B, gen_cfg, seen, extra):
    """The argument list every padt_vrt_head* entry point starts with, then `extra`."""
    _lib.check(_fn(name, _x16(hidden, table, proto, table_packed))(
        _stream(), _p(hidden), hidden.stride(0), _p(table), table.shape[0], _p(proto), proto.shape[0], _p(vrt_off), _p(mode_table), _p(step),
        _p(logits), logits.stride(0) if logits is not None else 0, _p(part_val), _p(part_idx), B, hidden.shape[1], eos, _p(table_packed),
        _p(gen_cfg), _p(seen), seen.shape[1] if seen is not None else 0, *extra), name)


def vrt_head(hidden, table, proto, vrt_off, part_val, part_idx, eos, mode_table=None, step=None, logits=None,
             table_packed=None, rows=None, gen_cfg=None, seen=None, ban=None, part_sum=None):
    """table_packed: pack_weight(table) — then `hidden` is a fragment-packed activation buffer holding `rows` valid rows.
    ban: int32 (rows, words) bitmap of banned table rows (gen_rules) → padt_vrt_head_ban; None is padt_vrt_head itself.
    part_sum: fp32 (nblk * rows) → padt_vrt_head_lse: also each block's Σ exp(logit - block max) per row (greedy_step(part_sum=, logprobs=))."""
    B = hidden.shape[0] if rows is None else rows
    name, extra = "padt_vrt_head", ()
    if ban is not None:
        assert ban.dtype == torch.int32 and ban.is_cuda and ban.dim() == 2 and ban.is_contiguous() and ban.shape[0] >= B
        name, extra = "padt_vrt_head_ban", (_p(ban), ban.shape[1])
    if part_sum is not None:
        assert part_sum.dtype == torch.float32 and part_sum.is_cuda and part_sum.is_contiguous()
        assert part_sum.numel() >= (table.shape[0] + proto.shape[0] + 15) // 16 * B
        name, extra = "padt_vrt_head_lse", ((_p(ban), ban.shape[1]) if ban is not None else (0, 0)) + (_p(part_sum),)
    _head_call(name, hidden, table, proto, vrt_off, part_val, part_idx, eos, mode_table, step, logits, table_packed, B, gen_cfg, seen, extra)


def seen_init(ids, rows, seen):
    """ids int64 (n,), rows int32 (n,) device tensors: set bit ids[i] in seen[rows[i]] (prompt tokens of a generate call)."""
    assert ids.dtype == torch.int64 and rows.dtype == torch.int32 and ids.numel() == rows.numel() and seen.dtype == torch.int32
    _lib.check(_lib.load().padt_seen_init(_stream(), _p(ids), _p(rows), ids.numel(), _p(seen), seen.shape[1]), "padt_seen_init")


GEN_RULES_INTS = 4096      # the packed rule table: fixed size, so a session's copy never moves (captured graphs read it)
GEN_RULES_MAX_NGRAM = 16
GEN_RULES_MAX_WORD = 16


def _rule_ids(name, ids, vocab_size):
    out = []
    for i in ids:
        try:
            if isinstance(i, bool):
                raise TypeError
            i = operator.index(i)                                    # Python / numpy integers and one-element integer tensors
        except TypeError:
            raise ValueError(f"{name}: token ids must be integers, got {i!r}") from None
        if i < 0:
            raise ValueError(f"{name}: token ids must be non-negative, got {i}")
        if vocab_size is not None and i >= vocab_size:
            raise NotImplementedError(f"{name}: id {i} is not a text id (< {vocab_size}): VRT ids are numbered per batch and cannot be named in a rule")
        out.append(i)
    return out


def gen_rules_key(no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, eos_ids=(), vocab_size=None):
    """The canonical form of HF's four pure-ban generate arguments: (n, static ids, begin ids, words) — sorted tuples without duplicates, static
    = suppress_tokens and the 1-token bad words (HF's NoBadWordsLogitsProcessor drops those equal to an EOS id: so does this), words = the
    bad words of two ids and more — or None when nothing is banned.  Raises by argument name: NotImplementedError above the kernel's caps
    (n-gram size / word length 16, the packed table GEN_RULES_INTS ints) and for ids that are not text ids, ValueError for malformed values."""
    n = 0 if no_repeat_ngram_size is None else no_repeat_ngram_size
    try:
        n = -1 if isinstance(n, bool) else operator.index(n)
    except TypeError:
        n = -1
    if n < 0:
        raise ValueError(f"no_repeat_ngram_size has to be a non-negative integer, got {no_repeat_ngram_size!r}")
    if n > GEN_RULES_MAX_NGRAM:
        raise NotImplementedError(f"no_repeat_ngram_size={n}: at most {GEN_RULES_MAX_NGRAM} on the MI355X path")
    static = set(_rule_ids("suppress_tokens", suppress_tokens if suppress_tokens is not None else (), vocab_size))
    begin = set(_rule_ids("begin_suppress_tokens", begin_suppress_tokens if begin_suppress_tokens is not None else (), vocab_size))
    words = set()
    eos = {int(e) for e in eos_ids}
    for wd in (bad_words_ids if bad_words_ids is not None else ()):
        if isinstance(wd, (int, str)) or len(wd) == 0:
            raise ValueError(f"bad_words_ids has to be a list of non-empty lists of token ids, got {bad_words_ids!r}")
        wd = _rule_ids("bad_words_ids", wd, vocab_size)
        if len(wd) > GEN_RULES_MAX_WORD:
            raise NotImplementedError(f"bad_words_ids: a bad word of {len(wd)} ids; at most {GEN_RULES_MAX_WORD} on the MI355X path")
        if len(wd) == 1:
            if wd[0] not in eos:
                static.add(wd[0])
        else:
            words.add(tuple(wd))
    key = (int(n), tuple(sorted(static)), tuple(sorted(begin)), tuple(sorted(words)))
    size = 4 + len(key[1]) + len(key[2]) + len(key[3]) + sum(1 + len(w) for w in key[3])
    if size > GEN_RULES_INTS:
        raise NotImplementedError(f"bad_words_ids / suppress_tokens / begin_suppress_tokens: the packed rule table takes {size} ints; "
                                  f"at most {GEN_RULES_INTS} on the MI355X path")
    return key if (n or key[1] or key[2] or key[3]) else None


def gen_rules_tensor(no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, eos_ids=(), vocab_size=None,
                     key=None):
    """→ the int32 CPU rule table padt_gen_rules reads (GEN_RULES_INTS ints, zero-padded; layout in include/padt_hip.h) for the arguments as
    gen_rules_key() canonicalises them, or for an already canonical `key`."""
    if key is None:
        key = gen_rules_key(no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens, eos_ids, vocab_size)
    n, static, begin, words = key if key is not None else (0, (), (), ())
    t = [n, len(static), len(begin), len(words), *static, *begin]
    o = len(t) + len(words)
    offs, recs = [], []
    for w in words:
        offs.append(o + len(recs))
        recs += [len(w), *w]
    t += offs + recs
    assert len(t) <= GEN_RULES_INTS
    return torch.tensor(t + [0] * (GEN_RULES_INTS - len(t)), dtype=torch.int32)


def gen_rules_unpack(table):
    """Inverse of gen_rules_tensor → the canonical (n, static ids, begin ids, words)."""
    t = table.tolist()
    n, ns, nb, nw = t[:4]
    o = 4 + ns + nb
    return (n, tuple(t[4: 4 + ns]), tuple(t[4 + ns: o]), tuple(tuple(t[f + 1: f + 1 + t[f]]) for f in t[o: o + nw]))


def gen_rules(rules, hist, hist_len, tokens, step, ban, n_cols):
    """ban[b] = the step's bitmap of banned table rows for every row b of hist (padt_gen_rules): rules int32 (GEN_RULES_INTS,) device copy of
    gen_rules_tensor, hist int32 (B, >= hist_len) prompt ids, tokens int64 (B, T) the generated ids, step the device step counter."""
    assert rules.dtype == torch.int32 and rules.is_cuda and rules.is_contiguous() and rules.numel() >= GEN_RULES_INTS
    assert hist.dtype == torch.int32 and hist.stride(1) == 1 and hist_len.dtype == torch.int32 and hist_len.numel() >= hist.shape[0]
    assert tokens.dtype == torch.int64 and tokens.stride(1) == 1 and tokens.shape[0] >= hist.shape[0] and step.dtype == torch.int32
    assert ban.dtype == torch.int32 and ban.is_contiguous() and ban.shape[0] >= hist.shape[0]
    _lib.check(_lib.load().padt_gen_rules(_stream(), _p(rules), _p(hist), hist.stride(0), _p(hist_len), _p(tokens), tokens.stride(0), _p(step),
                                          _p(ban), ban.shape[1], int(n_cols), hist.shape[0]), "padt_gen_rules")
    return ban


TOKEN_AUTOMATON_MAGIC = 0x54413031
TOKEN_AUTOMATON_MAX_STATES = 4096      # the packed automaton's caps: a session's copy has a fixed size, so it never moves (captured graphs read it)
TOKEN_AUTOMATON_MAX_EDGES = 32768
TOKEN_AUTOMATON_INTS = 5 + TOKEN_AUTOMATON_MAX_STATES + 2 * TOKEN_AUTOMATON_MAX_EDGES


def token_automaton_tensor(automaton=None, key=None):
    """→ the int32 CPU table padt_token_automaton reads (layout in include/padt_hip.h; 5 + S + 2 E ints) for a generation.TokenAutomaton or
    its `key` = (start, per-state tuples of (key, next state) sorted by key: the classes -3 / -2 / -1 first, then the text ids).
    NotImplementedError above TOKEN_AUTOMATON_MAX_STATES states / TOKEN_AUTOMATON_MAX_EDGES edges."""
    start, states = automaton.key if key is None else key
    S, E = len(states), sum(len(s) for s in states)
    if S > TOKEN_AUTOMATON_MAX_STATES or E > TOKEN_AUTOMATON_MAX_EDGES:
        raise NotImplementedError(f"token_automaton: {S} states / {E} edges; the packed table holds at most {TOKEN_AUTOMATON_MAX_STATES} states "
                                  f"and {TOKEN_AUTOMATON_MAX_EDGES} edges on the MI355X path")
    offs, flat = [0], []
    for s in states:
        for k, nx in s:
            flat += [int(k), int(nx)]
        offs.append(len(flat) // 2)
    return torch.tensor([TOKEN_AUTOMATON_MAGIC, S, E, int(start), *offs, *flat], dtype=torch.int32)


def token_automaton(table, gen_cfg, vrt_off, tokens, step, unfinished, state, ban, n_cols, vocab, rules_ban=None):
    """ban[b] = the step's bitmap for every row b of `state`: every column of [0, n_cols) banned except those the row's automaton state
    allows (padt_token_automaton).  table int32 device copy of token_automaton_tensor (trailing slack allowed), gen_cfg the device
    generation config (its EOS ids), vrt_off int32 (>= B + 1,), tokens int64 (>= B, T) the generated ids, step the device step counter,
    unfinished int32 (>= B,), state int32 (B, 2) = (state, valid_for_step) — fill with -1 to reset —, ban int32 (>= B, words) with
    32 * words >= n_cols; rules_ban: gen_rules' bitmap of this step (another buffer of ban's shape), OR-ed in.  → ban."""
    for t in (table, vrt_off, step, unfinished, state, ban):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    B = state.shape[0]
    assert table.dim() == 1 and table.numel() >= 5
    assert gen_cfg.is_cuda and gen_cfg.is_contiguous() and gen_cfg.numel() * gen_cfg.element_size() >= 20
    assert state.dim() == 2 and state.shape[1] == 2 and vrt_off.numel() >= B + 1 and unfinished.numel() >= B and step.numel() >= 1
    assert tokens.dtype == torch.int64 and tokens.is_cuda and tokens.dim() == 2 and tokens.stride(1) == 1 and tokens.shape[0] >= B
    assert ban.dim() == 2 and ban.shape[0] >= B and 0 < int(vocab) <= int(n_cols) <= 32 * ban.shape[1]
    if rules_ban is not None:
        assert rules_ban.dtype == torch.int32 and rules_ban.is_cuda and rules_ban.is_contiguous() and rules_ban.dim() == 2
        assert rules_ban.shape[0] >= B and rules_ban.shape[1] == ban.shape[1] and rules_ban.data_ptr() != ban.data_ptr()
    _lib.check(_lib.load().padt_token_automaton(_stream(), _p(table), table.numel(), _p(gen_cfg), _p(vrt_off), _p(tokens), tokens.stride(0),
                                                _p(step), _p(unfinished), _p(state), _p(ban), ban.shape[1], _p(rules_ban), int(n_cols),
                                                int(vocab), B), "padt_token_automaton")
    return ban


# The generation-config slots.  csrc/gen_cfg.h (struct GenCfg, with a static_assert on every offset) is the layout's single definition;
# this is its pack format, one 4-byte item per slot.
GEN_CFG_FMT = "<f4iiIfifii4f"
GEN_CFG_INTS = 16
assert struct.calcsize(GEN_CFG_FMT) == 4 * GEN_CFG_INTS


def gen_cfg_tensor(repetition_penalty=1.0, eos_ids=(), device="cuda", do_sample=False, seed=0, temperature=1.0, top_k=0, top_p=1.0,
                   write_back=False, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """Device copy of the generation-config slots the head / greedy / sampling kernels read:
    {float penalty; int eos[4]; int do_sample; unsigned seed; float temperature; int top_k; float top_p; int write_back; int pad;
    float min_p; float typical_p; float epsilon_cutoff; float eta_cutoff} — the last four read by warp_sample_rows alone, off at 0 / 1 / 0 / 0.
    write_back: sample_token overwrites its rows with the warped scores (output_scores / stopping criteria under sampling)."""
    eos = list(eos_ids)[:4] + [-1] * (4 - min(4, len(eos_ids)))
    raw = struct.pack(GEN_CFG_FMT, float(repetition_penalty), *eos, 1 if do_sample else 0, int(seed) & 0xFFFFFFFF, float(temperature),
                      int(top_k), float(top_p), 1 if write_back else 0, 0, float(min_p), float(typical_p), float(epsilon_cutoff),
                      float(eta_cutoff))
    return torch.frombuffer(bytearray(raw), dtype=torch.int32).clone().to(device)


def sample_token(logits, n_rows_table, gen_cfg, step, part_val, part_idx, batch, vocab=0, vrt_off=None, row_base=None):
    """One multinomial draw per row from the warped fp32 logits (padt_sample_token) into the (value, index) partial layout; with gen_cfg's
    write_back the rows [0, n_rows_table) are overwritten with the warped scores (l / T kept, -inf elsewhere).  row_base int32 [>= batch]
    (with vrt_off int32 [>= batch + 1] and vocab; padt_sample_token_keyed): the first row of each row's own batch in a merged decode group —
    the generator is then keyed by the row and column numbers the batch has alone, as warp_sample_rows keys its own."""
    assert logits.dtype == torch.float32 and logits.stride(-1) == 1
    if row_base is None:
        assert vrt_off is None and vocab == 0, "vocab / vrt_off key the generator through row_base only: pass all three or none"
        _lib.check(_lib.load().padt_sample_token(_stream(), _p(logits), logits.stride(0), int(n_rows_table), _p(gen_cfg), _p(step), _p(part_val),
                                                 _p(part_idx), int(batch)), "padt_sample_token")
        return
    assert row_base.dtype == torch.int32 and row_base.is_contiguous() and row_base.numel() >= batch
    assert vrt_off is not None and vrt_off.dtype == torch.int32 and vrt_off.is_contiguous() and vrt_off.numel() >= batch + 1
    _lib.check(_lib.load().padt_sample_token_keyed(_stream(), _p(logits), logits.stride(0), int(n_rows_table), _p(gen_cfg), _p(step),
                                                   _p(part_val), _p(part_idx), int(batch), int(vocab), _p(vrt_off), _p(row_base)),
               "padt_sample_token_keyed")


def warp_sample_rows(rows, n_cols, gen_cfg, step, part_val, part_idx, batch, vocab=0, vrt_off=None, row_base=None):
    """HF's MinP → Typical → Epsilon → Eta warpers, in place, over the fp32 rows sample_token left with write_back (dropped columns of
    [0, n_cols) become -inf, kept ones keep their bits), and one multinomial draw per row from what stays into the (value, index) partial
    layout (padt_warp_sample_rows_f32); the four values are gen_cfg's last slots (gen_cfg_tensor).  row_base int32 [>= batch] (with vrt_off
    int32 [>= batch + 1] and vocab): the first row of each row's own batch in a merged decode group — the generator is then keyed by the row
    and column numbers the batch has alone."""
    assert rows.dtype == torch.float32 and rows.is_cuda and rows.dim() == 2 and rows.stride(1) == 1 and rows.shape[0] >= batch and rows.shape[1] >= n_cols
    assert gen_cfg.dtype == torch.int32 and gen_cfg.is_contiguous() and gen_cfg.numel() >= GEN_CFG_INTS
    assert part_val.dtype == torch.float32 and part_val.numel() >= batch and part_idx.dtype == torch.int32 and part_idx.numel() >= batch
    if row_base is not None:
        assert row_base.dtype == torch.int32 and row_base.is_contiguous() and row_base.numel() >= batch
        assert vrt_off is not None and vrt_off.dtype == torch.int32 and vrt_off.is_contiguous() and vrt_off.numel() >= batch + 1
    _lib.check(_lib.load().padt_warp_sample_rows_f32(_stream(), _p(rows), rows.stride(0), int(n_cols), _p(gen_cfg), _p(step), _p(part_val),
                                                     _p(part_idx), int(batch), int(vocab), _p(vrt_off) if row_base is not None else None,
                                                     _p(row_base)), "padt_warp_sample_rows_f32")


def argmax_rows(scores, n_cols, part_val, part_idx, batch):
    """Arg-max per fp32 score row (ties → lowest index) into the (value, index) partial layout (padt_argmax_rows_f32): the hooked decode loop."""
    assert scores.dtype == torch.float32 and scores.stride(-1) == 1
    _lib.check(_lib.load().padt_argmax_rows_f32(_stream(), _p(scores), scores.stride(0), int(n_cols), _p(part_val), _p(part_idx), int(batch)),
               "padt_argmax_rows_f32")


def token_logprob_rows(rows, n_cols, part_idx, unfinished, step, logprobs, batch):
    """logprobs[b][*step] = unfinished[b] ? log_softmax(rows[b][:n_cols])[part_idx[b]] : 0 (padt_token_logprob_rows_f32): the token log-prob
    where the selection came from sample_token / argmax_rows; runs between that kernel and greedy_step (which clears `unfinished`)."""
    assert rows.dtype == torch.float32 and rows.is_cuda and rows.dim() == 2 and rows.stride(1) == 1 and rows.shape[0] >= batch and rows.shape[1] >= n_cols
    assert part_idx.dtype == torch.int32 and part_idx.numel() >= batch and unfinished.dtype == torch.int32 and unfinished.numel() >= batch
    assert step.dtype == torch.int32 and logprobs.dtype == torch.float32 and logprobs.dim() == 2 and logprobs.is_contiguous() and logprobs.shape[0] >= batch
    _lib.check(_lib.load().padt_token_logprob_rows_f32(_stream(), _p(rows), rows.stride(0), int(n_cols), _p(part_idx), _p(unfinished), _p(step),
                                                       _p(logprobs), logprobs.shape[1], int(batch)), "padt_token_logprob_rows_f32")


TOPK_ROWS_MAX_K = 32


def __getattr__(name):
    # TOPK_ROWS_CHUNK: columns per stage-1 block of padt_topk_logprob_rows_f32 — the kernel file's constant, read from the library on first use
    if name == "TOPK_ROWS_CHUNK":
        globals()[name] = int(_lib.load().padt_topk_rows_chunk())      # cached: this hook is not entered for it again
        return globals()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def topk_rows_workspace(n_cols, k, batch):
    """Bytes of the workspace topk_logprob_rows needs for `batch` rows of `n_cols` columns and `k` candidates (padt_topk_rows_workspace)."""
    return int(_lib.load().padt_topk_rows_workspace(int(n_cols), int(k), int(batch)))


def topk_logprob_rows(rows, n_cols, unfinished, step, workspace, batch, top_idx=None, top_val=None, vrt_off=None, vocab=0, patch_lp=None):
    """At t = *step, per row b < batch of the fp32 score rows (padt_topk_logprob_rows_f32; between the selection kernel and greedy_step):
    top_idx[b, t, j] / top_val[b, t, j] (int32 / fp32 (>= batch, t_max, k), both or neither) = the column with the j-th largest value of
    rows[b, :n_cols] (equal values: the lower column first) and its log_softmax; -1 / -inf once the finite columns run out.
    patch_lp[b, t, j] (fp32 (>= batch, t_max, p_cap), with vrt_off int32 [>= batch + 1] and vocab) = log_softmax(row)[vocab + vrt_off[b] + j] for
    the row's own vrt_off[b + 1] - vrt_off[b] patches, -inf beyond.  Finished rows get -1 / -inf everywhere; the rows are only read.
    workspace: a uint8 tensor of at least topk_rows_workspace(n_cols, k, batch) bytes."""
    assert rows.dtype == torch.float32 and rows.is_cuda and rows.dim() == 2 and rows.stride(1) == 1 and rows.shape[0] >= batch and rows.shape[1] >= n_cols
    assert unfinished.dtype == torch.int32 and unfinished.numel() >= batch and step.dtype == torch.int32 and step.numel() >= 1
    assert (top_idx is None) == (top_val is None), "topk_logprob_rows: top_idx and top_val go together"
    k, t_max = 0, None
    if top_idx is not None:
        assert top_idx.dtype == torch.int32 and top_val.dtype == torch.float32 and top_idx.is_cuda and top_val.is_cuda
        assert top_idx.dim() == 3 and top_idx.shape == top_val.shape and top_idx.is_contiguous() and top_val.is_contiguous() and top_idx.shape[0] >= batch
        t_max, k = int(top_idx.shape[1]), int(top_idx.shape[2])
    p_cap = 0
    if patch_lp is not None:
        assert patch_lp.dtype == torch.float32 and patch_lp.is_cuda and patch_lp.dim() == 3 and patch_lp.is_contiguous() and patch_lp.shape[0] >= batch
        assert t_max is None or patch_lp.shape[1] == t_max, "topk_logprob_rows: top_idx and patch_lp disagree on t_max"
        assert vrt_off is not None and vrt_off.dtype == torch.int32 and vrt_off.is_cuda and vrt_off.is_contiguous() and vrt_off.numel() >= batch + 1
        t_max, p_cap = int(patch_lp.shape[1]), int(patch_lp.shape[2])
    assert t_max is not None, "topk_logprob_rows: nothing asked (no top_idx / top_val and no patch_lp)"
    assert workspace.dtype == torch.uint8 and workspace.is_cuda and workspace.is_contiguous()
    lib = _lib.load()
    assert k > TOPK_ROWS_MAX_K or workspace.numel() >= lib.padt_topk_rows_workspace(int(n_cols), k, int(batch)), "topk_logprob_rows: workspace too small"
    _lib.check(lib.padt_topk_logprob_rows_f32(_stream(), _p(rows), rows.stride(0), int(n_cols), k, _p(unfinished), _p(step), t_max,
                                                      _p(top_idx), _p(top_val), _p(vrt_off) if patch_lp is not None else 0, int(vocab),
                                                      _p(patch_lp), p_cap, _p(workspace), int(batch)), "padt_topk_logprob_rows_f32")


def _step_call(name, part_val, part_idx, nblk, hidden, hidden_buf, unfinished, tokens_out, cur_tok, step, slot, lens, pos3, eos, pad, advance,
               gen_cfg, seen, extra):
    """The argument list every step entry point (padt_greedy_step, _lp, padt_forced_step) starts with, then `extra`."""
    B, D = hidden.shape
    _lib.check(getattr(_lib.load(), name)(
        _stream(), _p(part_val), _p(part_idx), nblk, B, D, eos, pad, tokens_out.shape[1], _p(unfinished), _p(tokens_out), _p(cur_tok), _p(step),
        _p(slot), _p(lens), _p(pos3), _p(hidden), _p(hidden_buf), 1 if advance else 0, _p(gen_cfg), _p(seen),
        seen.shape[1] if seen is not None else 0, *extra), name)


def greedy_step(part_val, part_idx, nblk, hidden, hidden_buf, unfinished, tokens_out, cur_tok, step, slot, lens, pos3,
                eos, pad, advance=True, gen_cfg=None, seen=None, part_sum=None, logprobs=None):
    """part_sum / logprobs (both or neither): vrt_head(part_sum=)'s block sums and the fp32 (B, T_max) buffer that gets the selected token's
    log-prob at the device step counter (padt_greedy_step_lp)."""
    name, extra = "padt_greedy_step", ()
    if part_sum is not None or logprobs is not None:
        assert part_sum is not None and logprobs is not None, "greedy_step: part_sum and logprobs go together"
        B = hidden.shape[0]
        assert part_sum.dtype == torch.float32 and part_sum.is_cuda and part_sum.is_contiguous() and part_sum.numel() >= nblk * B
        assert logprobs.dtype == torch.float32 and logprobs.is_cuda and logprobs.is_contiguous() and logprobs.shape == (B, tokens_out.shape[1])
        name, extra = "padt_greedy_step_lp", (_p(part_sum), _p(logprobs))
    _step_call(name, part_val, part_idx, nblk, hidden, hidden_buf, unfinished, tokens_out, cur_tok, step, slot, lens, pos3, eos, pad, advance,
               gen_cfg, seen, extra)


def _chk_forced(forced, B):
    assert forced.dtype == torch.int32 and forced.is_cuda and forced.dim() == 2 and forced.is_contiguous() and forced.shape[0] >= B


def vrt_head_probe(hidden, table, proto, vrt_off, part_val, part_idx, eos, part_sum, forced, probe_val, step, mode_table=None, logits=None,
                   table_packed=None, rows=None, gen_cfg=None, seen=None, ban=None):
    """vrt_head(part_sum=) that also writes probe_val[b] = the processed logit of column forced[b][*step] (padt_vrt_head_probe): forced int32
    (rows, t_forced) table columns, negative = a free step (nothing written for the row); probe_val fp32 (rows,); step the device counter."""
    B = hidden.shape[0] if rows is None else rows
    assert part_sum.dtype == torch.float32 and part_sum.is_cuda and part_sum.is_contiguous()
    assert part_sum.numel() >= (table.shape[0] + proto.shape[0] + 15) // 16 * B
    _chk_forced(forced, B)
    assert probe_val.dtype == torch.float32 and probe_val.is_cuda and probe_val.is_contiguous() and probe_val.numel() >= B
    assert step is not None and step.dtype == torch.int32
    if ban is not None:
        assert ban.dtype == torch.int32 and ban.is_cuda and ban.dim() == 2 and ban.is_contiguous() and ban.shape[0] >= B
    _head_call("padt_vrt_head_probe", hidden, table, proto, vrt_off, part_val, part_idx, eos, mode_table, step, logits, table_packed, B, gen_cfg,
               seen, (_p(ban), ban.shape[1] if ban is not None else 0, _p(part_sum), _p(forced), forced.shape[1], _p(probe_val)))


def vrt_head_bias(hidden, table, proto, vrt_off, part_val, part_idx, eos, bias=None, decay=None, step=None, mode_table=None, logits=None,
                  table_packed=None, rows=None, gen_cfg=None, seen=None, ban=None, part_sum=None, forced=None, probe_val=None):
    """vrt_head / vrt_head_probe with the score edits of generate(logit_bias=, patch_bias=, exponential_decay_length_penalty=)
    (padt_vrt_head_bias): bias fp32 (table rows + proto rows,) added to the raw logit before the repetition penalty; decay fp32 (t,) — an EOS
    column's v becomes v + |v| * decay[*step] after the mask and the bans.  The head is the one the other wrappers pick: forced (+ part_sum,
    probe_val) → the probe head, part_sum → the LSE head, else the plain one; bias = decay = None is that head, bit for bit."""
    B = hidden.shape[0] if rows is None else rows
    n_cols = table.shape[0] + proto.shape[0]
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_cuda and bias.dim() == 1 and bias.is_contiguous() and bias.numel() >= n_cols
    if decay is not None:
        assert decay.dtype == torch.float32 and decay.is_cuda and decay.dim() == 1 and decay.is_contiguous() and decay.numel() > 0
        assert step is not None and step.dtype == torch.int32
    if ban is not None:
        assert ban.dtype == torch.int32 and ban.is_cuda and ban.dim() == 2 and ban.is_contiguous() and ban.shape[0] >= B
    if part_sum is not None:
        assert part_sum.dtype == torch.float32 and part_sum.is_cuda and part_sum.is_contiguous() and part_sum.numel() >= (n_cols + 15) // 16 * B
    if forced is not None:
        _chk_forced(forced, B)
        assert part_sum is not None and step is not None and step.dtype == torch.int32
        assert probe_val is not None and probe_val.dtype == torch.float32 and probe_val.is_cuda and probe_val.is_contiguous() and probe_val.numel() >= B
    _head_call("padt_vrt_head_bias", hidden, table, proto, vrt_off, part_val, part_idx, eos, mode_table, step, logits, table_packed, B, gen_cfg,
               seen, (_p(ban), ban.shape[1] if ban is not None else 0, _p(part_sum), _p(forced), forced.shape[1] if forced is not None else 0,
                      _p(probe_val) if forced is not None else 0, _p(bias), _p(decay), decay.numel() if decay is not None else 0))


COUNT_MAX_RADIUS = 7            # patch_suppression: (2 * 7 + 1) ** 2 = 225 window cells, one thread each of padt_count_update's 256
COUNT_DTYPE = torch.int16       # the count tables' element as torch holds it: the kernels read the 16 bits UNSIGNED, saturating at 65535
COUNT_SAT = 65535               # (profiles/count_penalties.md §1); count_values() gives the numbers


def count_values(t):
    """A count table (COUNT_DTYPE) → its unsigned values, int32."""
    assert t.dtype == COUNT_DTYPE
    return t.to(torch.int32) & 0xffff


def _chk_counts(cnt_text, cnt_patch, near, B, vocab, n_proto):
    for t in (cnt_text, cnt_patch, near):
        assert t.dtype == COUNT_DTYPE and t.is_cuda
    assert cnt_text.dim() == 2 and cnt_text.stride(1) == 1 and cnt_text.shape[0] >= B and cnt_text.shape[1] >= vocab
    assert cnt_text.stride(0) >= vocab and cnt_text.stride(0) % 4 == 0 and cnt_text.data_ptr() % 8 == 0
    assert cnt_patch.dim() == 1 and cnt_patch.stride(0) == 1 and cnt_patch.numel() >= n_proto
    assert near.dim() == 1 and near.stride(0) == 1 and near.numel() >= n_proto


def count_update(tokens, step, unfinished, vrt_off, grid, radius, cnt_text, cnt_patch, near, vocab, n_proto):
    """After greedy_step / forced_step, in front of stop_match: every row the bookkeeping kernel left unfinished adds the token it just
    generated to its counts — cnt_text[b][tok] for a text id, cnt_patch[tok - vocab] for one of its own patches — and, when that token closed a
    run of VRT tokens, 1 per run token to near[] on the clipped radius[b] window of its grid[b] = (hp, wp) (padt_count_update;
    generation.count_state is the specification).  uint16 tables, saturating; radius int32 (B,), < 0 = no suppression for the row; grid
    int32 (B, 2).  Where the host can see it (CPU tensors are not read back), hp * wp == the row's patch count is the caller's to check."""
    B = radius.numel()
    _chk_i32(step, n=1)
    _chk_i32(unfinished, radius, n=B)
    _chk_i32(vrt_off, n=B + 1)
    _chk_i32(grid, n=2 * B)
    assert grid.dim() == 2 and grid.shape[1] == 2
    _chk_counts(cnt_text, cnt_patch, near, B, int(vocab), int(n_proto))
    assert tokens.dtype == torch.int64 and tokens.is_cuda and tokens.dim() == 2 and tokens.stride(1) == 1 and tokens.shape[0] >= B
    _lib.check(_lib.load().padt_count_update(_stream(), _p(tokens), tokens.stride(0), _p(step), _p(unfinished), _p(vrt_off), _p(grid), _p(radius),
                                             _p(cnt_text), cnt_text.stride(0), int(vocab), _p(cnt_patch), _p(near), int(n_proto), B),
               "padt_count_update")


def vrt_head_counts(hidden, table, proto, vrt_off, part_val, part_idx, eos, cnt_text, cnt_patch, near, cpen, bias=None, decay=None, step=None,
                    mode_table=None, logits=None, table_packed=None, rows=None, gen_cfg=None, seen=None, ban=None, part_sum=None, forced=None,
                    probe_val=None):
    """vrt_head_bias (bias / decay optional) with the count edits of generate(frequency_penalty=, presence_penalty=, patch_suppression=)
    (padt_vrt_head_counts; generation.count_penalty_row is the specification): count_update's three uint16 tables and cpen fp32 (3, rows) =
    per row f, p and the suppression penalty (0: off, inf: a ban)."""
    B = hidden.shape[0] if rows is None else rows
    n_cols = table.shape[0] + proto.shape[0]
    _chk_counts(cnt_text, cnt_patch, near, B, table.shape[0], proto.shape[0])
    assert cpen.dtype == torch.float32 and cpen.is_cuda and cpen.is_contiguous() and cpen.shape == (3, B)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_cuda and bias.dim() == 1 and bias.is_contiguous() and bias.numel() >= n_cols
    if decay is not None:
        assert decay.dtype == torch.float32 and decay.is_cuda and decay.dim() == 1 and decay.is_contiguous() and decay.numel() > 0
        assert step is not None and step.dtype == torch.int32
    if ban is not None:
        assert ban.dtype == torch.int32 and ban.is_cuda and ban.dim() == 2 and ban.is_contiguous() and ban.shape[0] >= B
    if part_sum is not None:
        assert part_sum.dtype == torch.float32 and part_sum.is_cuda and part_sum.is_contiguous() and part_sum.numel() >= (n_cols + 15) // 16 * B
    if forced is not None:
        _chk_forced(forced, B)
        assert part_sum is not None and step is not None and step.dtype == torch.int32
        assert probe_val is not None and probe_val.dtype == torch.float32 and probe_val.is_cuda and probe_val.is_contiguous() and probe_val.numel() >= B
    _head_call("padt_vrt_head_counts", hidden, table, proto, vrt_off, part_val, part_idx, eos, mode_table, step, logits, table_packed, B, gen_cfg,
               seen, (_p(ban), ban.shape[1] if ban is not None else 0, _p(part_sum), _p(forced), forced.shape[1] if forced is not None else 0,
                      _p(probe_val) if forced is not None else 0, _p(bias), _p(decay), decay.numel() if decay is not None else 0,
                      _p(cnt_text), cnt_text.stride(0), _p(cnt_patch), _p(near), _p(cpen)))


def forced_step(part_val, part_idx, nblk, hidden, hidden_buf, unfinished, tokens_out, cur_tok, step, slot, lens, pos3, eos, pad, forced, n_cols,
                advance=True, gen_cfg=None, seen=None, part_sum=None, logprobs=None, probe_val=None):
    """greedy_step with the caller's tokens (padt_forced_step): an unfinished row b with 0 <= forced[b][*step] < n_cols takes that column as its
    token, every other row is the free step.  part_sum / logprobs / probe_val (all or none): vrt_head_probe's outputs and the (B, T_max)
    log-prob buffer — a forced row gets (probe - max) - log Σ, -inf for a -inf column."""
    B = hidden.shape[0]
    _chk_forced(forced, B)
    lp = (part_sum, logprobs, probe_val)
    if any(t is not None for t in lp):
        assert all(t is not None for t in lp), "forced_step: part_sum, logprobs and probe_val go together"
        assert part_sum.dtype == torch.float32 and part_sum.is_cuda and part_sum.is_contiguous() and part_sum.numel() >= nblk * B
        assert logprobs.dtype == torch.float32 and logprobs.is_cuda and logprobs.is_contiguous() and logprobs.shape == (B, tokens_out.shape[1])
        assert probe_val.dtype == torch.float32 and probe_val.is_cuda and probe_val.is_contiguous() and probe_val.numel() >= B
    _step_call("padt_forced_step", part_val, part_idx, nblk, hidden, hidden_buf, unfinished, tokens_out, cur_tok, step, slot, lens, pos3, eos, pad,
               advance, gen_cfg, seen, (_p(part_sum), _p(logprobs), _p(forced), forced.shape[1], _p(probe_val), int(n_cols)))


def forced_override(part_idx, forced, step, unfinished, n_cols, batch):
    """Row path of forced tokens (padt_forced_override): part_idx[b] = forced[b][*step] for the unfinished rows with an entry in [0, n_cols),
    after sample_token / warp_sample_rows / argmax_rows and before token_logprob_rows / forced_step."""
    _chk_forced(forced, batch)
    assert part_idx.dtype == torch.int32 and part_idx.is_cuda and part_idx.numel() >= batch
    assert unfinished.dtype == torch.int32 and unfinished.numel() >= batch and step.dtype == torch.int32
    _lib.check(_lib.load().padt_forced_override(_stream(), _p(part_idx), _p(forced), forced.shape[1], _p(step), _p(unfinished), int(n_cols),
                                                int(batch)), "padt_forced_override")


def collect_summary(err, unfinished, nf_rows, nf_batch, n_batch, tokens, done, eos, gen_cfg, out):
    """One launch: out = [err, any(unfinished), nf_rows…, nf_batch[:n_batch]…, first_eos step per row…] (padt_collect_summary)."""
    n_rows = unfinished.numel()
    assert out.dtype == torch.int32 and out.numel() >= 2 + 2 * n_rows + n_batch and tokens.dtype == torch.int64 and tokens.is_contiguous()
    _lib.check(_lib.load().padt_collect_summary(_stream(), _p(err), _p(unfinished), _p(nf_rows), _p(nf_batch), n_rows, int(n_batch), _p(tokens),
                                                tokens.shape[1], int(done), int(eos), _p(gen_cfg), _p(out)), "padt_collect_summary")
    return out


STOP_RULES_MAGIC = 0x53523031
STOP_RULES_MAX_SEQS = 32        # the packed stop sequences' caps: a session's copy has a fixed size, so it never moves (captured graphs read it)
STOP_RULES_MAX_LEN = 32
STOP_RULES_INTS = 2 + STOP_RULES_MAX_SEQS + STOP_RULES_MAX_SEQS * STOP_RULES_MAX_LEN
STOP_REASONS = (None, "eos", "stop", "length", "criteria")      # finish_reason codes; "criteria" is written by the hooked loop alone


def _chk_i32(*ts, n=0):
    for t in ts:
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() >= n


def stop_ban(gen_cfg, eos, step, min_tokens, ban_out, n_cols, ban_in=None):
    """ban_out[b] = ban_in[b] (None: zeros) plus, while *step < min_tokens[b], the bits of `eos` and gen_cfg's EOS list (padt_stop_ban):
    generate(min_tokens=) as the ban bitmap the head reads.  min_tokens int32 (B,), ban_out / ban_in int32 (>= B, words), two buffers.  → ban_out."""
    B = min_tokens.numel()
    _chk_i32(step, min_tokens, ban_out)
    assert gen_cfg.is_cuda and gen_cfg.is_contiguous() and gen_cfg.numel() * gen_cfg.element_size() >= 20
    assert ban_out.dim() == 2 and ban_out.shape[0] >= B and 0 < int(n_cols) <= 32 * ban_out.shape[1]
    if ban_in is not None:
        _chk_i32(ban_in)
        assert ban_in.dim() == 2 and ban_in.shape[0] >= B and ban_in.shape[1] == ban_out.shape[1] and ban_in.data_ptr() != ban_out.data_ptr()
    _lib.check(_lib.load().padt_stop_ban(_stream(), _p(gen_cfg), int(eos), _p(step), _p(min_tokens), _p(ban_in), _p(ban_out), ban_out.shape[1],
                                         int(n_cols), B), "padt_stop_ban")
    return ban_out


def stop_match(table, gen_cfg, eos, tokens, step, min_tokens, max_tokens, unfinished, finish_step, finish_reason, stop_index):
    """After greedy_step / forced_step: every row b of finish_reason without a recorded finish is tested for an EOS id, a completed stop
    sequence (the lowest index; only once the row holds min_tokens[b] tokens) and its budget max_tokens[b], in this order; a finish clears
    unfinished[b] and writes finish_step / finish_reason / stop_index (padt_stop_match).  table: the device copy of generation.stop_table."""
    B = finish_reason.numel()
    _chk_i32(step, n=1)
    _chk_i32(min_tokens, max_tokens, unfinished, finish_step, finish_reason, stop_index, n=B)
    _chk_i32(table, n=STOP_RULES_INTS)
    assert gen_cfg.is_cuda and gen_cfg.is_contiguous() and gen_cfg.numel() * gen_cfg.element_size() >= 20
    assert tokens.dtype == torch.int64 and tokens.is_cuda and tokens.dim() == 2 and tokens.stride(1) == 1 and tokens.shape[0] >= B
    _lib.check(_lib.load().padt_stop_match(_stream(), _p(table), table.numel(), _p(gen_cfg), int(eos), _p(tokens), tokens.stride(0), _p(step),
                                           _p(min_tokens), _p(max_tokens), _p(unfinished), _p(finish_step), _p(finish_reason), _p(stop_index), B),
               "padt_stop_match")


def collect_summary_stop(err, unfinished, nf_rows, nf_batch, n_batch, tokens, done, eos, gen_cfg, finish_step, finish_reason, stop_index, out):
    """collect_summary's record, then finish_step, finish_reason and stop_index of every row (padt_collect_summary_stop): one launch."""
    n_rows = unfinished.numel()
    assert out.dtype == torch.int32 and out.numel() >= 2 + 5 * n_rows + n_batch and tokens.dtype == torch.int64 and tokens.is_contiguous()
    _chk_i32(finish_step, finish_reason, stop_index, n=n_rows)
    _lib.check(_lib.load().padt_collect_summary_stop(_stream(), _p(err), _p(unfinished), _p(nf_rows), _p(nf_batch), n_rows, int(n_batch),
                                                     _p(tokens), tokens.shape[1], int(done), int(eos), _p(gen_cfg), _p(finish_step),
                                                     _p(finish_reason), _p(stop_index), _p(out)), "padt_collect_summary_stop")
    return out


DECODE_ROWS_MAX = 128           # rows of one decode step: what padt_gemm_packed_* and the fragment-packed activation buffers take
BEAM_MAX_WIDTH = 8              # generate(beam_width=): the widest beam padt_beam_step / padt_beam_reorder_kv keep in registers
BEAM_CFG_MAGIC = 0x424d3031
BEAM_CFG_INTS = 8
BEAM_STATE_F32 = ("live", "st_score", "st_lp")                               # per sample [B][K]
BEAM_STATE_I32 = ("st_end", "st_parent", "st_tok", "sent")                   # per sample [B][K]


def beam_cfg_tensor(K, keep, early, t_last, never_max) -> torch.Tensor:
    """The packed beam config padt_beam_step reads (BEAM_CFG_INTS int32, CPU; layout in include/padt_hip.h): early — 0 False, 1 True,
    2 "never"; t_last — the call's last step; never_max — the early-stop heuristic divides by the length table's entry of t_last."""
    return torch.tensor([BEAM_CFG_MAGIC, int(K), int(keep), int(early), int(t_last), 1 if never_max else 0, 0, 0], dtype=torch.int32)


class BeamState:
    """The device state of a beam search over B samples of K beams and t_max steps (padt_beam_step's arrays, by the header's names): the
    live scores and the finished store [B][K], flags [B][2], the steps' records beam_tok / beam_parent / beam_lp [t_max][B * K], perm and p0
    [B * K], the config and the length table.  reset() puts it before step 0: live = [0, -inf, ...], an empty store, every sample open."""

    def __init__(self, B, K, t_max, device, own=None):
        """own(name, numel, dtype) → a flat zeroed device tensor that stays at its address (a session's allocator: every array but `flags`
        has a size that does not depend on K, and `flags` is asked for at 2 * B * K, so one set of buffers serves every width)."""
        self.B, self.K, self.t_max = int(B), int(K), int(t_max)
        R = self.B * self.K
        own = own or (lambda name, n, dt: torch.zeros(n, device=device, dtype=dt))

        def z(name, shape, dt, n=None):
            numel = 1
            for d in shape:
                numel *= d
            return own(name, numel if n is None else n, dt)[:numel].view(shape)
        for n in BEAM_STATE_F32:
            setattr(self, n, z(n, (self.B, self.K), torch.float32))
        for n in BEAM_STATE_I32:
            setattr(self, n, z(n, (self.B, self.K), torch.int32))
        self.flags = z("flags", (self.B, 2), torch.int32, n=2 * R)
        self.beam_tok, self.beam_parent = (z(n, (self.t_max, R), torch.int32) for n in ("beam_tok", "beam_parent"))
        self.beam_lp = z("beam_lp", (self.t_max, R), torch.float32)
        self.perm, self.p0 = z("perm", (R,), torch.int32), z("p0", (R,), torch.int32)
        self.cfg = z("cfg", (BEAM_CFG_INTS,), torch.int32)
        self.len_table = z("len_table", (self.t_max,), torch.float32)
        self.len_table.fill_(1.0)
        self.reset()

    def reset(self):
        self.live.fill_(float("-inf"))
        self.live[:, 0] = 0.0
        self.st_score.fill_(float("-inf"))
        for t in (self.st_lp, self.st_tok, self.sent, self.beam_tok, self.beam_parent, self.beam_lp, self.p0):
            t.zero_()
        self.st_end.fill_(-1)
        self.st_parent.fill_(-1)
        self.st_tok.fill_(-1)
        self.flags[:, 0] = 1
        self.flags[:, 1] = 0
        self.perm.copy_(torch.arange(self.B * self.K, device=self.perm.device, dtype=torch.int32) % self.K)


def beam_step(st, top_idx, top_val, hidden, hidden_buf, unfinished, cur_tok, step, slot, lens, pos3, vrt_off, eos, pad, vocab, n_cols,
              advance=True, gen_cfg=None, err=None, rep_lp=None):
    """One beam-search step of every sample of `st` (a BeamState), in the place of greedy_step (padt_beam_step): reads the rows' entries of
    top_idx / top_val (B * K, t_top, keep) at the device step counter, updates the state, files the step's records and does greedy_step's
    chores for the B * K rows (hidden rows, slot / lens / pos3, unfinished of a done sample's rows, the step counter).  rep_lp (fp32
    (B * K, keep), beam_cand_lp's): the log-probs recorded for the candidates instead of top_val's; the scores add top_val's either way."""
    R, D = hidden.shape
    assert R == st.B * st.K and hidden.is_contiguous() and hidden_buf.is_contiguous() and hidden_buf.shape == (st.t_max, R, D), "beam_step: rows"
    assert top_idx.dtype == torch.int32 and top_val.dtype == torch.float32 and top_idx.is_contiguous() and top_val.is_contiguous()
    assert top_idx.dim() == 3 and top_idx.shape == top_val.shape and top_idx.shape[0] == R
    _chk_i32(step, n=1)
    _chk_i32(unfinished, slot, lens, n=R)
    _chk_i32(vrt_off, n=R + 1)
    assert pos3.dtype == torch.int32 and pos3.is_contiguous() and pos3.shape == (3, R) and cur_tok.dtype == torch.int64 and cur_tok.numel() == R
    _lib.check(_lib.load().padt_beam_step(
        _stream(), _p(top_idx), _p(top_val), top_idx.shape[1], top_idx.shape[2], st.B, st.K, D, st.t_max, _p(st.cfg), _p(st.len_table), _p(gen_cfg),
        int(eos), int(pad), int(vocab), int(n_cols), _p(vrt_off), _p(st.live), _p(st.st_score), _p(st.st_lp), _p(st.st_end), _p(st.st_parent),
        _p(st.st_tok), _p(st.sent), _p(st.flags), _p(st.beam_tok), _p(st.beam_parent), _p(st.beam_lp), _p(st.perm), _p(cur_tok), _p(unfinished),
        _p(step), _p(slot), _p(lens), _p(pos3), _p(hidden), _p(hidden_buf), 1 if advance else 0, _p(err), _p(rep_lp)), "padt_beam_step")


def beam_cand_lp(part_val, part_idx, part_sum, nblk, rows, n_cols, top_idx, step, out):
    """out[b, j] = log_softmax(rows[b])[top_idx[b, *step, j]] as padt_greedy_step_lp / padt_forced_step compute it from the LSE head's block
    partials (padt_beam_cand_lp): what a beam step records as a candidate's token log-prob.  rows fp32 (R, >= n_cols), out fp32 (R, keep)."""
    R, keep = top_idx.shape[0], top_idx.shape[2]
    assert rows.dtype == torch.float32 and rows.is_cuda and rows.dim() == 2 and rows.stride(1) == 1 and rows.shape[0] >= R
    assert part_val.dtype == torch.float32 and part_sum.dtype == torch.float32 and part_idx.dtype == torch.int32
    assert part_val.numel() >= nblk * R and part_sum.numel() >= nblk * R and part_idx.numel() >= nblk * R
    assert top_idx.dtype == torch.int32 and top_idx.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= R * keep
    _lib.check(_lib.load().padt_beam_cand_lp(_stream(), _p(part_val), _p(part_idx), _p(part_sum), int(nblk), R, _p(rows), rows.stride(0), int(n_cols),
                                             _p(top_idx), top_idx.shape[1], keep, _p(step), _p(out)), "padt_beam_cand_lp")
    return out



def beam_kv_table(k_images, vt_images) -> torch.Tensor:
    """The device table of cache image pointers beam_reorder_kv reads: int64 (layers, 2) = (K image, V^T image) of every layer.  The images
    must stay allocated while the table is in use (a session builds it once over its own caches)."""
    assert len(k_images) == len(vt_images) and len(k_images) > 0
    for k, v in zip(k_images, vt_images):
        assert k.is_cuda and v.is_cuda and k.is_contiguous() and v.is_contiguous() and k.element_size() == 2 and v.element_size() == 2
        assert k.dim() == 4 and k.shape[:2] == v.shape[:2] and k.shape[2] == v.shape[3] and k.shape[3] == v.shape[2], "beam_kv_table: (B, Hkv, S, D) / (B, Hkv, D, S)"
        assert k.shape == k_images[0].shape
    return torch.tensor([[k.data_ptr(), v.data_ptr()] for k, v in zip(k_images, vt_images)], dtype=torch.int64).to(k_images[0].device)


def beam_reorder_kv(table, perm, p0, slot, B, K, n_kv_heads, head_dim, s_max, t_max, rows=None):
    """The packed KV caches of every layer follow the beams (padt_beam_reorder_kv): slots [p0, slot) of row sample * K + c get the former
    bits of row sample * K + perm[c], in place, for the images `table` (beam_kv_table) names.  rows: the images' row count (checked against
    B * K when given)."""
    assert table.dtype == torch.int64 and table.is_cuda and table.is_contiguous() and table.dim() == 2 and table.shape[1] == 2
    _chk_i32(perm, p0, slot, n=int(B) * int(K))
    assert rows is None or int(rows) == int(B) * int(K), "beam_reorder_kv: the images hold B * K rows"
    _lib.check(_lib.load().padt_beam_reorder_kv(_stream(), _p(table), table.shape[0], _p(perm), _p(p0), _p(slot), int(B), int(K), int(n_kv_heads),
                                                int(head_dim), int(s_max), int(t_max)), "padt_beam_reorder_kv")


def beam_finalize(st, n_best, hidden_buf, out_off, pad, vocab):
    """generation.beam_backtrace on the device (padt_beam_finalize) → dict(tokens (B * n_best, t_max) int64, logprobs (same) fp32, scores
    (B * n_best,) fp32, lengths int32, src_row (B * n_best, t_max) int32, hidden (t_max, B * n_best, D) — zero behind a hypothesis's end).
    out_off: int32 (B * n_best,) — the patch offset of every returned row in the returned batch's VRT numbering."""
    n, dev = st.B * int(n_best), hidden_buf.device
    D = hidden_buf.shape[2]
    assert hidden_buf.is_contiguous() and hidden_buf.shape[:2] == (st.t_max, st.B * st.K)
    _chk_i32(out_off, n=n)
    out = dict(tokens=torch.empty((n, st.t_max), device=dev, dtype=torch.int64), logprobs=torch.empty((n, st.t_max), device=dev, dtype=torch.float32),
               scores=torch.empty(n, device=dev, dtype=torch.float32), lengths=torch.empty(n, device=dev, dtype=torch.int32),
               src_row=torch.empty((n, st.t_max), device=dev, dtype=torch.int32), hidden=torch.zeros((st.t_max, n, D), device=dev, dtype=hidden_buf.dtype))
    _lib.check(_lib.load().padt_beam_finalize(
        _stream(), _p(st.st_score), _p(st.st_lp), _p(st.st_end), _p(st.st_parent), _p(st.st_tok), _p(st.beam_tok), _p(st.beam_parent), _p(st.beam_lp),
        st.B, st.K, int(n_best), D, st.t_max, int(pad), int(vocab), _p(out_off), _p(hidden_buf), _p(out["hidden"]), _p(out["tokens"]),
        _p(out["logprobs"]), _p(out["scores"]), _p(out["lengths"]), _p(out["src_row"])), "padt_beam_finalize")
    return out


def assemble_sequences(input_ids, tokens, n_steps, vocab, proto_row0):
    """→ (B, L + n_steps) int64: [input_ids | tokens[:, :n_steps]] with session-global VRT ids shifted back by proto_row0 (padt.py:751)."""
    assert input_ids.dtype == torch.int64 and input_ids.stride(1) == 1 and tokens.dtype == torch.int64 and tokens.stride(1) == 1
    B, L = input_ids.shape
    out = torch.empty((B, L + int(n_steps)), dtype=torch.int64, device=tokens.device)
    _lib.check(_lib.load().padt_assemble_sequences(_stream(), _p(input_ids), input_ids.stride(0), L, _p(tokens), tokens.stride(0), int(n_steps),
                                                   int(vocab), int(proto_row0), _p(out), B), "padt_assemble_sequences")
    return out


def logit_mask(vrt_off, vocab, table_rows, proto_row0, batch):
    """→ (batch, table_rows) bool past_logit_mask (padt.py:196-201) from the session's prototype row offsets of the batch's rows."""
    assert vrt_off.dtype == torch.int32 and vrt_off.numel() >= batch + 1
    out = torch.empty((batch, table_rows), dtype=torch.uint8, device=vrt_off.device)
    _lib.check(_lib.load().padt_logit_mask(_stream(), _p(vrt_off), int(vocab), int(table_rows), int(proto_row0), _p(out), int(batch)), "padt_logit_mask")
    return out.view(torch.bool)


def stash_step_f32(src, step, dst):
    """dst[*step] = src (fp32, whole buffer) under the device step counter (padt_stash_step_f32): per-step score rows for output_scores."""
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous() and dst[0].numel() == src.numel()
    _lib.check(_lib.load().padt_stash_step_f32(_stream(), _p(src), src.numel(), _p(step), dst.shape[0], _p(dst)), "padt_stash_step_f32")
    return dst


def mask_upsample_binarize(masks, src_h, src_w, dst_h, dst_w, max_h, max_w, want_logits=False, out=None, up=None):
    """masks (n_obj, Hm, Wm) fp32 logits; src/dst sizes int32 device tensors (n_obj,) → uint8 (n_obj, max_h, max_w)
    [, fp32 up-sampled logits].  (max_h, max_w) are the launch extents: an object larger than them is cropped to them, and mask_rle on the
    result reports it.  out / up: caller-owned (n_obj, max_h, max_w) planes (any object and row stride) to write instead of fresh zeros;
    up implies want_logits."""
    lib = _lib.load()
    assert masks.dtype == torch.float32 and masks.stride(-1) == 1
    n = masks.shape[0]
    want_logits = want_logits or up is not None
    if out is None:
        out = torch.zeros((n, max_h, max_w), dtype=torch.uint8, device=masks.device)
    if up is None and want_logits:
        up = torch.zeros((n, max_h, max_w), dtype=torch.float32, device=masks.device)
    assert out.dtype == torch.uint8 and out.shape == (n, max_h, max_w) and out.stride(2) == 1
    assert up is None or (up.dtype == torch.float32 and up.shape == (n, max_h, max_w) and up.stride(2) == 1)
    for t in (src_h, src_w, dst_h, dst_w):
        assert t.dtype == torch.int32 and t.numel() == n
    _lib.check(lib.padt_mask_upsample_binarize(_stream(), _p(masks), masks.stride(0), masks.stride(1), _p(src_h), _p(src_w),
                                               _p(dst_h), _p(dst_w), _p(out), out.stride(0), out.stride(1), _p(up),
                                               up.stride(0) if up is not None else 0, up.stride(1) if up is not None else 0,
                                               n, int(max_h), int(max_w)), "padt_mask_upsample_binarize")
    return (out, up) if want_logits else out


def _rle_caps(mh, mw, worst_case):
    """(runs, string bytes) capacity per object.  The worst case — every pixel its own run — is 4 + 2 bytes of scratch per PIXEL per object (an OVD batch
    of 56 objects at 640 x 640: 140 MB per call); a segmentation mask has a handful of runs per COLUMN, so the default bound is 128 runs per column
    (+ the zero-length first run; the noise-like masks random-init weights produce have ~80), 5 bytes per run (counts below 2^24).  A mask beyond it is reported (n_counts < 0) and the caller falls back to the
    host statement for that batch."""
    if worst_case:
        return mh * mw + 2, 2 * mh * mw + 16
    runs = min(mh * mw + 2, 128 * mw + 2)
    return runs, 5 * runs + 16


_RLE_SCRATCH = {}                                                     # (device, n, cap_c, cap_s) → buffers, reused by the next call of that shape on the stream


def mask_rle_launch(bin_masks, dst_h, dst_w, worst_case=False):
    """Enqueue padt_mask_rle for (n_obj, max_h, max_w) uint8 masks on the current stream; → handle for mask_rle_fetch (no host sync here, so a
    caller can put its other device work and copies behind the same single wait).  Scratch: bounded capacities (_rle_caps), one cached set per shape
    (a handle is valid until the next launch of the same shape: fetch first — postprocess does)."""
    lib = _lib.load()
    assert bin_masks.dtype == torch.uint8 and bin_masks.is_cuda and bin_masks.dim() == 3 and bin_masks.stride(2) == 1
    n, mh, mw = bin_masks.shape
    if n == 0:
        return None
    dev = bin_masks.device
    cap_c, cap_s = _rle_caps(mh, mw, worst_case)
    key = (dev, n, cap_c, cap_s)
    buf = _RLE_SCRATCH.get(key)
    if buf is None:
        if len(_RLE_SCRATCH) >= 8:
            _RLE_SCRATCH.clear()
        buf = dict(counts=torch.empty((n, cap_c), dtype=torch.int32, device=dev), strs=torch.empty((n, cap_s), dtype=torch.uint8, device=dev),
                   n_counts=torch.empty(n, dtype=torch.int32, device=dev), str_len=torch.empty(n, dtype=torch.int32, device=dev),
                   packed=torch.empty(n * cap_s, dtype=torch.uint8, device=dev), offsets=torch.empty(n + 1, dtype=torch.int32, device=dev))
        _RLE_SCRATCH[key] = buf
    h = dict(buf, n=n, masks=bin_masks, worst_case=worst_case)
    _lib.check(lib.padt_mask_rle(_stream(), _p(bin_masks), bin_masks.stride(0), bin_masks.stride(1), _p(dst_h), _p(dst_w), n, mh, _p(h["counts"]), cap_c,
                                 _p(h["strs"]), cap_s, _p(h["n_counts"]), _p(h["str_len"]), _p(h["packed"]), h["packed"].numel(), _p(h["offsets"])),
               "padt_mask_rle")
    return h


def mask_rle_fetch(h, want_counts=False, on_overflow="raise"):
    """→ list of n_obj ASCII COCO `counts` strings [, list of count lists]: the offset table, then exactly the string bytes.  A mask beyond the
    bounded scratch (or beyond max_h / ld_row): PaDTHipError, or None with on_overflow="none" (the caller computes the batch on the host)."""
    if h is None:
        return ([], []) if want_counts else []
    n = h["n"]
    off = h["offsets"].cpu().tolist()
    if off[-1] < 0:
        if on_overflow == "none":
            return None
        raise _lib.PaDTHipError("padt_mask_rle: capacity exceeded (n_counts %s)" % h["n_counts"].cpu().tolist())
    raw = h["packed"][: off[-1]].cpu().numpy().tobytes()
    out = [raw[off[i]: off[i + 1]].decode("ascii") for i in range(n)]
    if want_counts:
        nc = h["n_counts"].cpu().tolist()
        cc = h["counts"].cpu()
        return out, [cc[i, : nc[i]].tolist() for i in range(n)]
    return out


def mask_rle(bin_masks, dst_h, dst_w, want_counts=False):
    """COCO RLE `counts` strings of binarised masks, computed on the device (padt_mask_rle): bin_masks (n_obj, max_h, max_w) uint8 as
    mask_upsample_binarize returns them, dst_h / dst_w int32 device tensors (n_obj,).  → list of n_obj ASCII strings [, list of count lists].
    Two small device-to-host copies (the offset table, then exactly the string bytes) instead of the masks themselves."""
    r = mask_rle_fetch(mask_rle_launch(bin_masks, dst_h, dst_w), want_counts, on_overflow="none")
    if r is None:                                                     # noise-like masks beyond the bounded scratch: once more with the worst-case capacities
        r = mask_rle_fetch(mask_rle_launch(bin_masks, dst_h, dst_w, worst_case=True), want_counts)
    return r


def patchify_normalize(img_u8, lut, out, patch=14, merge=2, temporal=2):
    """img_u8 (H, W, 3) uint8 device tensor → rows of `out` ((H/patch)*(W/patch), 3*temporal*patch*patch), fp32 or bf16."""
    assert img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.shape[2] == 3
    assert lut.dtype == torch.float32 and lut.shape == (3, 256) and out.stride(1) == 1
    H, W = img_u8.shape[:2]
    _lib.check(_fn("padt_patchify_normalize", out.dtype)(_stream(), _p(img_u8), H, W, _p(lut), _p(out), out.stride(0),
                                                         1 if out.dtype in (BF16, F16) else 0, patch, merge, temporal), "padt_patchify_normalize")
    return out


# ------------------------------------------------------------------------------------------------ split-precision decoder ops
F32 = torch.float32
OUT_NONE, OUT_F32, OUT_SPLIT = 0, 1, 2


def gemm_hp(a_split, w2, bias=None, out=None, epilogue=EPI_NONE, residual=None, out_mode=OUT_F32, M=None, w_packed=None, lo_off=None):
    """Split-precision GEMM (include/padt_hip.h "hp decoder"): a_split (M, 2K) bf16 rows [hi | lo], w2 (N, 2K) = [W | W].
    out_mode OUT_F32 → fp32 (M, N) [+ fp32 residual, in place allowed]; OUT_SPLIT → bf16 (M, 2N) rows [hi | lo]; epilogue EPI_SWIGLU (OUT_SPLIT only,
    weight rows [gate16 | up16]-interleaved) → bf16 (M, 2 * N/2) split rows of silu(gate) * up.
    w_packed (few rows only): the pack_weight() image of W — the rows are then packed too (one padt_pack_rows launch) so that every wave load of
    either operand is 1 KiB contiguous (padt_gemm_split_rows, layout 3).
    lo_off (OUT_SPLIT only): column of `out` at which the lo half starts (default: right after the hi half; a multiple of 4, >= the hi width)."""
    lib = _lib.load()
    _chk_bf16(a_split, w2, bias)
    M = a_split.shape[0] if M is None else M
    N, K2 = w2.shape
    assert a_split.shape[1] == K2, (a_split.shape, w2.shape)
    n_out = N // 2 if epilogue == EPI_SWIGLU else N
    if out_mode == OUT_F32:
        assert epilogue != EPI_SWIGLU
        if out is None:
            out = torch.empty((M, (N + 3) // 4 * 4), device=a_split.device, dtype=F32)
        assert out.dtype == F32 and out.stride(-1) == 1
        if residual is not None:
            assert residual.dtype == F32 and epilogue == EPI_RESID
        lo_off = 0
    else:
        assert residual is None and n_out % 4 == 0
        if out is None:
            out = torch.empty((M, 2 * n_out), device=a_split.device, dtype=BF16)
        lo_off = n_out if lo_off is None else int(lo_off)
        assert out.dtype == BF16 and lo_off >= n_out and out.shape[1] >= lo_off + n_out
    if M <= 64 and K2 % 16 == 0 and ((out_mode == OUT_F32 and epilogue in (EPI_NONE, EPI_RESID)) or epilogue == EPI_SWIGLU):
        # few rows (a decode step): bound by the weight stream — read W once and multiply it with the hi and the lo fragments (padt_gemm_split_rows)
        K = K2 // 2
        if w_packed is not None and K % 32 == 0 and N % 16 == 0 and a_split.stride(0) == K2:
            ap = torch.empty(((M + 15) // 16 * 16, K2), device=a_split.device, dtype=BF16)
            pack_rows(a_split, ap, M, to_packed=True)
            _lib.check(lib.padt_gemm_split_rows(_stream(), _p(ap), K2, 16 * K, _p(w_packed), w_packed.stride(0), _p(bias), _p(out), out.stride(0), lo_off,
                                                _p(residual), residual.stride(0) if residual is not None else 0, M, N, K, epilogue, 3), "padt_gemm_split_rows")
            return out
        _lib.check(lib.padt_gemm_split_rows(_stream(), _p(a_split), a_split.stride(0), K, _p(w2), w2.stride(0), _p(bias), _p(out), out.stride(0), lo_off,
                                            _p(residual), residual.stride(0) if residual is not None else 0, M, N, K, epilogue, 0), "padt_gemm_split_rows")
        return out
    if GEMM_LOG is not None:
        GEMM_LOG.append(("hp", a_split, w2, bias, out, epilogue, residual, out_mode, M))
    _tg_note("hp", M, N, K2 // 2)                                    # algorithmic K: the MFMA pipe executes 2K (hi and lo operands)
    _lib.check(lib.padt_gemm_bf16_ex(_stream(), _p(a_split), a_split.stride(0), _p(w2), w2.stride(0), _p(bias), _p(out), out.stride(0),
                                     _p(residual), residual.stride(0) if residual is not None else 0, M, N, K2, epilogue,
                                     1 if out_mode == OUT_F32 else 0, 0, 1 if residual is not None else 0, lo_off), "padt_gemm_bf16_ex")
    return out


def norm_split(x, w=None, eps=1e-6, act=0, idx=None, add=None, add_div=1, pos=None, y0_mode=OUT_SPLIT, y1_mode=OUT_NONE, chunk=None,
               rows=None, D=None, y0=None, y1=None):
    """→ (y0, y1) of padt_norm_split; x bf16 or fp32 (rows, >= D); modes OUT_NONE / OUT_F32 / OUT_SPLIT (split rows are 2*D wide).
    y0 / y1: caller-owned outputs of the mode's type and width (any row stride the entry point accepts) instead of fresh ones."""
    lib = _lib.load()
    assert x.dtype in (BF16, F32) and x.stride(-1) == 1
    D = x.shape[1] if D is None else D
    rows = (idx.numel() if idx is not None else x.shape[0]) if rows is None else rows
    chunk = D if chunk is None else chunk

    def mk(mode, y):
        if mode == OUT_NONE:
            return None
        shape, dt = (rows, D if mode == OUT_F32 else 2 * D), F32 if mode == OUT_F32 else BF16
        if y is None:
            return torch.empty(shape, device=x.device, dtype=dt)
        assert y.dtype == dt and y.shape == shape and y.stride(-1) == 1, (y.dtype, y.shape, y.stride())
        return y
    y0, y1 = mk(y0_mode, y0), mk(y1_mode, y1)
    if add is not None:
        assert add.dtype == F32 and add.stride(-1) == 1
    if pos is not None:
        assert pos.dtype == F32 and pos.stride(-1) == 1
    if idx is not None:
        assert idx.dtype == torch.int32
    _lib.check(lib.padt_norm_split(_stream(), _p(x), x.stride(0), 1 if x.dtype == F32 else 0, _p(idx), _p(add),
                                   add.stride(0) if add is not None else 0, add_div, _p(w), float(eps), int(act), _p(pos),
                                   pos.stride(0) if pos is not None else 0, pos.shape[0] if pos is not None else 1,
                                   _p(y0), y0.stride(0) if y0 is not None else 0, y0_mode, _p(y1), y1.stride(0) if y1 is not None else 0,
                                   y1_mode, rows, D, chunk), "padt_norm_split")
    return y0, y1


def swiglu_split(gu, I, out=None):
    """fp32 rows [gate(I) | up(I)] → split rows [hi(I) | lo(I)] of silu(gate) * up (padt_swiglu_split)."""
    assert gu.dtype == F32 and gu.stride(-1) == 1 and gu.shape[1] >= 2 * I
    if out is None:
        out = torch.empty((gu.shape[0], 2 * I), device=gu.device, dtype=BF16)
    _lib.check(_lib.load().padt_swiglu_split(_stream(), _p(gu), gu.stride(0), int(I), _p(out), out.stride(0), gu.shape[0]), "padt_swiglu_split")
    return out


def layernorm_f32(x, w, b, eps=1e-5, out=None):
    """fp32 LayerNorm rows (bf16 weight / bias) → fp32 rows (padt_layernorm_f32)."""
    assert x.dtype == F32 and x.stride(-1) == 1
    _chk_bf16(w, b)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=F32)
    _lib.check(_lib.load().padt_layernorm_f32(_stream(), _p(x), x.stride(0), _p(w), _p(b), float(eps), _p(out), out.stride(0), x.shape[0], x.shape[1]),
               "padt_layernorm_f32")
    return out


def rope_half_f32_(x, cos, sin, n_heads, head_dim):
    """in place on the first n_heads*head_dim columns of the fp32 rows x (T, row)."""
    assert x.dtype == F32 and cos.dtype == F32 and sin.dtype == F32 and cos.stride(-1) == 1 and sin.stride() == cos.stride()
    _lib.check(_lib.load().padt_rope_half_f32(_stream(), _p(x), x.stride(0), _p(cos), _p(sin), cos.stride(0), x.shape[0], n_heads,
                                              head_dim), "padt_rope_half_f32")
    return x


def scatter_rows_f32(src, idx, dst, D=None):
    """dst[idx[i]] = src[i] for fp32 rows (distinct int32 indices)."""
    assert src.dtype == F32 and dst.dtype == F32 and idx.dtype == torch.int32 and src.stride(-1) == 1 and dst.stride(-1) == 1
    D = src.shape[1] if D is None else D
    _lib.check(_lib.load().padt_scatter_rows_f32(_stream(), _p(src), src.stride(0), _p(idx), _p(dst), dst.stride(0), idx.numel(), D), "padt_scatter_rows_f32")
    return dst


def attn_f32(q, k, v, cu_q, cu_k, max_q, max_k, n_heads, head_dim, scale=None, out=None, kv_group=1, causal=False, len_k=None, mfma=False):
    """fp32 varlen attention → split rows (Tq, 2*n_heads*head_dim) bf16.  kv_group: q heads per kv head (GQA); causal: bottom-right aligned
    mask; len_k (int32 device, per segment): key counts for segments that start at cu_k[s] and are not packed back to back (a KV cache)."""
    assert q.dtype == F32 and k.dtype == F32 and v.dtype == F32 and cu_q.dtype == torch.int32 and cu_k.dtype == torch.int32
    Dm = n_heads * head_dim
    if out is None:
        out = torch.empty((q.shape[0], 2 * Dm), device=q.device, dtype=BF16)
    scale = head_dim ** -0.5 if scale is None else scale
    fn = _lib.load().padt_attn_f32_mfma if mfma else _lib.load().padt_attn_f32     # mfma: v_mfma_f32_16x16x4_f32 (head_dim 80 / 128)
    _lib.check(fn(_stream(), _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0), Dm,
                                         _p(cu_q), _p(cu_k), cu_q.numel() - 1, int(max_q), int(max_k), n_heads, head_dim, float(scale), int(kv_group),
                                         1 if causal else 0, _p(len_k)),
               "padt_attn_f32")
    return out


def mask_scatter_f32(e2, mask_tok, cu_patch, obj_w, masks, n_obj, total_patches, dm):
    assert e2.dtype == F32 and mask_tok.dtype == F32 and masks.dtype == F32 and masks.is_contiguous()
    _lib.check(_lib.load().padt_mask_scatter_f32(_stream(), _p(e2), e2.stride(0), _p(mask_tok), mask_tok.stride(0), _p(cu_patch), _p(obj_w),
                                                 _p(masks), n_obj, total_patches, masks.shape[1], masks.shape[2], dm), "padt_mask_scatter_f32")
    return masks


def resample_pass_u8(img, out, bounds, kk, horizontal):
    """One pass of Pillow's 8-bit resample (csrc/resize.hip): img / out (H, W, C) uint8 device tensors, bounds (n, 2) / kk (n, ksize) int32."""
    assert img.dtype == torch.uint8 and out.dtype == torch.uint8 and img.is_contiguous() and out.is_contiguous()
    assert bounds.dtype == torch.int32 and kk.dtype == torch.int32 and bounds.is_contiguous() and kk.is_contiguous()
    n = out.shape[1] if horizontal else out.shape[0]
    assert bounds.shape == (n, 2) and kk.shape[0] == n and img.shape[2] == out.shape[2]
    _lib.check(_lib.load().padt_resample_pass_u8(_stream(), _p(img), img.shape[0], img.shape[1], img.shape[2], _p(out), out.shape[0],
                                                 out.shape[1], _p(bounds), _p(kk), kk.shape[1], 1 if horizontal else 0), "padt_resample_pass_u8")
    return out


def pack_results(out, n, cap, mask_hw, sample_idx, valid_h, valid_w, boxes, scores, masks):
    """One batch's vl_decode output → the fixed-capacity int32 exchange record `out` (padt_pack_results), on the current stream."""
    assert out.dtype == torch.int32 and out.is_contiguous() and out.is_cuda
    H, Wd = (masks.shape[1], masks.shape[2]) if masks is not None else (0, 0)
    if n:
        assert sample_idx.dtype == torch.int32 and boxes.dtype == torch.float32 and scores.dtype == torch.float32
        assert boxes.stride(-1) == 1 and (masks is None or (masks.dtype == torch.float32 and masks.stride(-1) == 1))
        assert masks is None or (valid_h.dtype == torch.int64 and valid_w.dtype == torch.int64)
    _lib.check(_lib.load().padt_pack_results(_stream(), _p(out), out.numel(), int(n), int(cap), int(mask_hw), _p(sample_idx), _p(valid_h), _p(valid_w),
                                             _p(boxes), boxes.stride(0) if n else 0, _p(scores), scores.stride(0) if n else 0,
                                             _p(masks) if n else 0, masks.stride(0) if masks is not None else 0,
                                             masks.stride(1) if masks is not None else 0, int(H), int(Wd)), "padt_pack_results")
    return out


def memset(t, value=0):
    lib = _lib.load()
    _lib.check(lib.padt_memset(_stream(), _p(t), value, t.numel() * t.element_size()), "padt_memset")
    return t
