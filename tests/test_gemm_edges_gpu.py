"""Every GEMM entry point on strided windows in poisoned buffers, and the row / column locality of non-finite operands.

The parity tests of test_kernels_gpu.py / test_kernels_f16_gpu.py / test_decoder_hp_gpu.py hand the GEMMs tightly sized, contiguous randn
tensors: a tail read that goes one chunk too far lands on the next row's finite numbers (and is multiplied by a zero-filled chunk of the
other operand), a stray store lands in allocator slack, and all strides are equal.  Here every operand is a WINDOW (tests/edge_util.py) in a
larger allocation, at least 256 rows and 128 elements away from each of its ends, every 2-D window of a launch at a row stride of its own:
  * what is poisoned: NaN around A, W (row-major, or the fragment-packed image as a slab), bias, a separate residual R, row_scale, col_scale,
    the fp8 weight scales and the cos / sin tables (e4m3 bytes: the NaN code 0x7F); the finite sentinel -1234 around every output — C, the
    fp32 stream x32 (also when it is the in-place residual), the 16-bit mirror xb, the lo half of a split (hi | lo) output and the gap
    [N, lo_off) in front of it, packed C.  Packed activations: NaN behind the ceil(B / 16) blocks AND in the stale rows B .. 16 ceil(B / 16) - 1
    of the last block (rows < B are asserted; what the stale rows produce is unspecified and is not stored).
  * what is asserted, for every case (three()): the kernel runs twice on windows of identical strides, with NaN and then with zeros around
    its inputs.  (1) the result window of the NaN run meets the reference; (2) it is bit-identical to the zero run; (3) every element
    outside every output window still holds the sentinel, after both runs.
  * tolerances are the suite's, unchanged, the ones the entry point's parity test uses: close_bf16 / close_f16 at ulps = 1 for gemm,
    gemm_rope, gemm_fp8 (fp16 output: 2) and the bf16 decode projections (gemm_rmsnorm, gemm_packed, gemm_packed_fp8), ulps = 1.5 for the fp16 decode
    projections; close_f32 at rel = 2e-5 (out_f32) / 3e-5 (fp32 streams), the mirror EXACTLY X(stream_scale * x32); gemm_fp8's fp32 stream
    within 3e-5 of the magnitude sum; split_close for split (hi | lo) outputs and rel_err < 5e-5 for gemm_hp's fp32 output.  References are
    the fp32 (gemm_hp: fp64) PyTorch statement on the exact operands the kernel is given.
  * locality (test_nonfinite_values_stay_in_their_row_and_column): contiguous clean operands plus ONE planted value.  NaN at A[r, k] → row r
    of every output of every epilogue is NaN, every other row bit-identical to the clean run; +inf at A[r, k] → row r of the plain output
    non-finite, other rows bit-identical; NaN at W[n, k] → output column n (SwiGLU: the column fed by that gate / up row) NaN, every other
    column bit-identical.  This is what makes the per-batch range guard of a merged decode group sound.  The RoPE epilogue rotates column
    PAIRS, so a NaN weight row reaches its partner column too: it is exercised under the A-side plants only.
The cases are the smallest shapes that reach each dispatch branch ("GEMM contract").  One thing no assertion here can see, by the very
locality asserted above: a read of A rows past M (W rows past N) that stays inside the allocation — it feeds accumulator rows (columns) that are
never stored.  The K-direction guards and every store-side bound are visible: without stage_tile's `k < K` select every 128^2-tile output is NaN
(assertions 1 and 2), without store_frag's `m >= M` bound or with the peeled tail's mirror advanced by the stream's stride assertion 3 fails.
"""
import pytest
import torch

from edge_util import MIN_COLS, MIN_ROWS, SENTINEL, Arena, Failures, same_bits, three
from test_decoder_hp_gpu import rel_err, split_close
from test_kernels_f16_gpu import close_f16
from test_kernels_gpu import close_bf16, close_f32, interleave_gate_up

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
X16 = pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
R0, C0 = MIN_ROWS, MIN_COLS            # every window starts 256 rows and 128 elements into its backing (16-byte aligned for every type)
DECODE_ULPS = {BF: 1.0, F16: 1.5}      # gemm_rmsnorm / gemm_packed*: what test_kernels_gpu.py / test_kernels_f16_gpu.py use
silu, gelu = torch.nn.functional.silu, torch.nn.functional.gelu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


@pytest.fixture
def knobs(ops):
    yield ops.gemm_knobs
    ops.gemm_knobs(mode256=1, mf=0, peel=1, colsplit=1, group_m=8)


# ------------------------------------------------------------------------------------------------------------ helpers
def rnd(dt, *shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


def pos(*shape, seed=0):
    """fp32 scales in [0.5, 1.5)"""
    g = torch.Generator(device="cpu").manual_seed(77 + seed)
    return (0.5 + torch.rand(*shape, generator=g)).cuda()


def blank(rows, cols, dt):
    return torch.full((rows, cols), 3.0, dtype=dt, device="cuda")


def close16(out, ref, what, ulps=1.0):
    (close_bf16 if out.dtype == BF else close_f16)(out, ref, what, ulps=ulps)


def swiglu_ref(lin):
    """fp32 rows over [gate16 | up16]-interleaved weight rows → silu(gate) * up"""
    y = lin.view(lin.shape[0], lin.shape[1] // 32, 2, 16)
    return (silu(y[:, :, 0]) * y[:, :, 1]).reshape(lin.shape[0], lin.shape[1] // 2)


# ------------------------------------------------------------------------------------------------------------ ops.gemm epilogues
EPIS = ["none", "gelu", "resid", "resid_inplace", "swiglu", "f32", "row_scale"]


def gemm_case(ops, fails, dt, M, N, K, epi, tag, distinct=False):
    """One epilogue of ops.gemm on windows.  distinct: assert that all 2-D operands have pairwise different row strides."""
    a, w, b = rnd(dt, M, K, seed=1), rnd(dt, N, K, scale=0.05, seed=2), rnd(dt, N, seed=3)
    r, rs = rnd(dt, M, N, seed=4), pos(M, seed=5)
    lin = a.float() @ w.float().T
    if epi == "swiglu":
        n2 = N // 2
        w_in = interleave_gate_up(w[:n2].contiguous(), w[n2:].contiguous())
        b_in = interleave_gate_up(b[:n2].reshape(n2, 1), b[n2:].reshape(n2, 1)).view(-1)
        ref = silu(lin[:, :n2] + b[:n2].float()) * (lin[:, n2:] + b[n2:].float())
    else:
        w_in, b_in = w, b
        ref = {"none": lin + b.float(), "gelu": gelu(lin + b.float()), "resid": lin + b.float() + r.float(),
               "resid_inplace": lin + b.float() + r.float(), "f32": lin, "row_scale": lin * rs[:, None] + b.float()}[epi]

    def body(ar):
        A, W, Bv = ar.inp(a), ar.inp(w_in), ar.inp(b_in)
        if epi == "resid":
            R, C = ar.inp(r), ar.out(blank(M, N, dt))
            assert R.stride(0) != C.stride(0)
            ops.gemm(A, W, Bv, out=C, epilogue=ops.EPI_RESID, residual=R)
        elif epi == "resid_inplace":
            C = ar.out(r)
            ops.gemm(A, W, Bv, out=C, epilogue=ops.EPI_RESID, residual=C)
        elif epi == "swiglu":
            C = ar.out(blank(M, N // 2, dt))
            ops.gemm(A, W, Bv, out=C, epilogue=ops.EPI_SWIGLU)
        elif epi == "f32":
            C = ar.out(blank(M, N, F32))
            ops.gemm(A, W, None, out=C, out_f32=True)
        elif epi == "row_scale":
            C = ar.out(blank(M, N, dt))
            ops.gemm(A, W, Bv, out=C, row_scale=ar.inp(rs))
        else:
            C = ar.out(blank(M, N, dt))
            ops.gemm(A, W, Bv, out=C, epilogue=ops.EPI_GELU if epi == "gelu" else ops.EPI_NONE)
        if distinct:
            lds = [A.stride(0), W.stride(0), C.stride(0)] + ([R.stride(0)] if epi == "resid" else [])
            assert len(set(lds)) == len(lds) and A.stride(0) != K and W.stride(0) != K, lds
        return {"C": C}

    def check(got):
        if epi == "f32":
            close_f32(got["C"], ref, tag, rel=2e-5)
        else:
            close16(got["C"], ref, tag)
    three(fails, tag, body, check)


@X16
@pytest.mark.parametrize("K", [72, 2056])
@pytest.mark.parametrize("N", [37, 40])
@pytest.mark.parametrize("M", [5, 20, 40, 64])
def test_skinny_kernel_on_windows(ops, dt, M, N, K):
    """gemm_skinny_kernel through ops.gemm: MT = 1 / 2 / 4 and the full 64 rows; the scalar ragged-N path (37) and a ragged last 16-column
    block (40); K = 72 leaves one 8-wide chunk in the last 32-wide K-step (an odd K-step pair), K = 2056 takes NW = 8 (ksteps >= 64) with a
    chunk tail again.  SwiGLU needs N % 32 == 0: N = 64 there."""
    fails = Failures()
    for epi in EPIS:
        gemm_case(ops, fails, dt, M, 64 if epi == "swiglu" else N, K, epi, f"skinny {epi} {M}x{N}x{K}")
    fails.done()


@X16
@pytest.mark.parametrize("M,N,K,n_glu", [(300, 260, 136, 288), (129, 37, 72, 64)])
def test_tile128_kernel_on_windows(ops, dt, M, N, K, n_glu):
    """gemm_tile_kernel (mode256 on auto, shapes too small for the 256 kernel): (300, 260, 136) = one interior tile on the fast path plus
    ragged M and N tiles, with a K tail inside BK = 64; (129, 37, 72) = one row and a scalar N tail in the second tile row.  SwiGLU at the
    next multiple of 32 columns that keeps a ragged N tile (288 = 2 tiles + 32; 64)."""
    fails = Failures()
    for epi in EPIS:
        gemm_case(ops, fails, dt, M, n_glu if epi == "swiglu" else N, K, epi, f"tile128 {epi} {M}x{N}x{K}")
    fails.done()


def rope_case(ops, fails, dt, M, N, K, tag):
    """ops.gemm_rope: 2 heads of head_dim 40 rotated (rope_cols = 80), the other columns pass through; cos / sin tables (M, 20) at ld_cs > D."""
    from padt_amd.weights import interleave_rope_rows
    nh, D = 2, 40
    a, w, b, rs = rnd(dt, M, K, seed=11), rnd(dt, N, K, scale=0.05, seed=12), rnd(dt, N, seed=13), pos(M, seed=14)
    ang = torch.rand(M, D // 2, generator=torch.Generator().manual_seed(15)).cuda() * 6.28
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    lin = (a.float() @ w.float().T) * rs[:, None] + b.float()
    qk = lin[:, : nh * D].view(M, nh, D)
    rot = torch.cat([-qk[..., D // 2:], qk[..., : D // 2]], -1)
    c2, s2 = torch.cat([cos, cos], -1)[:, None], torch.cat([sin, sin], -1)[:, None]
    ref = lin.clone()
    ref[:, : nh * D] = (qk * c2 + rot * s2).reshape(M, -1)
    wi, bi = interleave_rope_rows(w, nh, D), interleave_rope_rows(b, nh, D)
    idx = torch.arange(nh * D).view(nh, 2, D // 2).transpose(1, 2).reshape(-1).cuda()      # interleaved column j holds original column idx[j]

    def body(ar):
        A, W, Bv, C, RS = ar.inp(a), ar.inp(wi), ar.inp(bi), ar.out(blank(M, N, dt)), ar.inp(rs)
        Cs = ar.inp(cos)
        Sn = ar.inp(sin, ld=Cs.stride(0))                           # the entry point takes ONE table stride
        lds = [A.stride(0), W.stride(0), C.stride(0), Cs.stride(0)]
        assert len(set(lds)) == 4 and Cs.stride(0) > D, lds
        ops.gemm_rope(A, W, Bv, C, Cs, Sn, nh * D, D, row_scale=RS)
        return {"C": C}

    def check(got):
        un = got["C"].clone()
        un[:, idx] = got["C"][:, : nh * D]
        close16(un, ref, tag)
    three(fails, tag, body, check)


def resid32_case(ops, fails, dt, M, N, K, tag):
    """ops.gemm_resid32: the fp32 stream in place (sentinel around it) and its 16-bit mirror at ldc2 > N, both at strides of their own."""
    s = ops.stream_scale(dt)
    a, w, b = rnd(dt, M, K, seed=21), rnd(dt, N, K, scale=0.05, seed=22), rnd(dt, N, seed=23)
    x0 = rnd(F32, M, N, scale=3.0, seed=24)
    ref = x0 + a.float() @ w.float().T + b.float()

    def body(ar):
        A, W, Bv, X, XB = ar.inp(a), ar.inp(w), ar.inp(b), ar.out(x0), ar.out(blank(M, N, dt))
        lds = [A.stride(0), W.stride(0), X.stride(0), XB.stride(0)]
        assert len(set(lds)) == 4 and XB.stride(0) > N, lds
        ops.gemm_resid32(A, W, Bv, X, XB)
        return {"x32": X, "xb": XB}

    def check(got):
        close_f32(got["x32"], ref, tag, rel=3e-5)
        assert torch.equal(got["xb"], (got["x32"] * s).to(dt)), f"{tag}: mirror != X(stream_scale * stream)"
    three(fails, tag, body, check)


def split_operands(M, K, seed):
    """fp32 activations as the (M, 2K) bf16 rows [hi | lo] gemm_hp consumes, and the fp64 values they hold exactly."""
    a = rnd(F32, M, K, seed=seed)
    hi = a.to(BF)
    a_s = torch.cat([hi, (a - hi.float()).to(BF)], dim=1).contiguous()
    return a_s, a_s[:, :K].double() + a_s[:, K:].double()


def hp_split_case(ops, fails, M, N, K, glu, tag, w_packed=False, slab_a=False):
    """ops.gemm_hp writing a split (hi | lo) output with lo_off > the hi width: the gap [width, lo_off) is guarded like everything outside.
    glu: the split SwiGLU over [gate16 | up16]-interleaved weight rows (N weight rows → N / 2 columns)."""
    from padt_amd.weights import interleave16
    a_s, a64 = split_operands(M, K, 31)
    if glu:
        I = N // 2
        wg, wu = rnd(BF, I, K, scale=0.05, seed=32), rnd(BF, I, K, scale=0.05, seed=33)
        bg, bu = rnd(BF, I, scale=0.1, seed=34), rnd(BF, I, scale=0.1, seed=35)
        w, b = interleave16(wg, wu).contiguous(), interleave16(bg, bu).contiguous()
        ref = silu(a64 @ wg.double().T + bg.double()) * (a64 @ wu.double().T + bu.double())
        width = I
    else:
        w, b = rnd(BF, N, K, scale=0.05, seed=32), rnd(BF, N, scale=0.1, seed=34)
        ref = a64 @ w.double().T + b.double()
        width = N
    w2 = torch.cat([w, w], dim=1).contiguous()
    lo_off = width + 20

    def body(ar):
        A, W2, Bv = ar.inp(a_s, slab=slab_a), ar.inp(w2), ar.inp(b)
        C = ar.out(torch.full((M, lo_off + width), SENTINEL, dtype=BF, device="cuda"), spec=[(0, 0, M, width), (0, lo_off, M, width)])
        kw = dict(w_packed=ar.inp(ops.pack_weight(w), slab=True)) if w_packed else {}
        ops.gemm_hp(A, W2, Bv, out=C, epilogue=ops.EPI_SWIGLU if glu else ops.EPI_NONE, out_mode=ops.OUT_SPLIT, lo_off=lo_off, **kw)
        return {"hi": C[:, :width], "lo": C[:, lo_off:]}

    def check(got):
        split_close(got["hi"].float() + got["lo"].float(), ref, tag)
    three(fails, tag, body, check)


@X16
@pytest.mark.parametrize("peel", [0, 2])
@pytest.mark.parametrize("mf", [2, 3, 4])
def test_tile256_kernel_on_windows(ops, knobs, dt, mf, peel):
    """gemm_tile256_kernel forced (mode256 = 2) at every tile height: M = 2 tile rows + 24 (a ragged third tile row with peel = 0; with
    peel = 2 those 24 rows leave through the skinny kernel, whose seven pointers — A, C, R as fp32 or 16-bit, row_scale, the mirror,
    cos / sin — are advanced by `done` rows of their OWN stride: every 2-D operand here has a stride of its own), N = 300 (one full and one
    ragged column tile), K = 128.  Plus SwiGLU at N = 320, the fp32 stream with its mirror, the RoPE epilogue, and — bf16 only, as the
    entry point is — the split (hi | lo) output and the split SwiGLU of gemm_hp with a gap in front of the lo half."""
    knobs(mode256=2, mf=mf, peel=peel)
    M, N, K = 2 * 64 * mf + 24, 300, 128
    fails = Failures()
    for epi in ["none", "gelu", "resid", "resid_inplace", "f32", "row_scale"]:
        gemm_case(ops, fails, dt, M, N, K, epi, f"tile256 mf{mf} peel{peel} {epi}", distinct=True)
    gemm_case(ops, fails, dt, M, 320, K, "swiglu", f"tile256 mf{mf} peel{peel} swiglu", distinct=True)
    resid32_case(ops, fails, dt, M, N, K, f"tile256 mf{mf} peel{peel} resid32")
    rope_case(ops, fails, dt, M, N, K, f"tile256 mf{mf} peel{peel} rope")
    if dt == BF:
        hp_split_case(ops, fails, M, N, K // 2, False, f"tile256 mf{mf} peel{peel} hp split")          # the kernel's K is 2 x 64
        hp_split_case(ops, fails, M, 320, K // 2, True, f"tile256 mf{mf} peel{peel} hp split swiglu")
    fails.done()


@X16
@pytest.mark.parametrize("mf", [2, 3, 4])
def test_tile256_column_split_on_windows(ops, knobs, dt, mf):
    """The column split (colsplit = 2: the last two tile columns as a second launch at a column offset of W, bias, C, R and the mirror)."""
    knobs(mode256=2, mf=mf, peel=0, colsplit=2)
    M, N, K = 64 * mf + 8, 1024, 64
    fails = Failures()
    for epi in ["none", "gelu", "resid", "f32", "row_scale", "swiglu"]:
        gemm_case(ops, fails, dt, M, N, K, epi, f"colsplit mf{mf} {epi}", distinct=True)
    resid32_case(ops, fails, dt, M, N, K, f"colsplit mf{mf} resid32")
    if dt == BF:
        hp_split_case(ops, fails, M, N, K // 2, True, f"colsplit mf{mf} hp split swiglu")
    fails.done()


# ------------------------------------------------------------------------------------------------------------ decode projections
@X16
@pytest.mark.parametrize("M", [3, 20, 64])
def test_gemm_rmsnorm_on_windows(ops, dt, M):
    """ops.gemm_rmsnorm (the fused norm reads A's K tail for the sum of squares too): N = 96 plain, N = 64 SwiGLU, K = 264."""
    K = 264
    fails = Failures()
    for N, glu in ((96, False), (64, True)):
        x, w, b = rnd(dt, M, K, seed=41), rnd(dt, N, K, scale=0.05, seed=42), rnd(dt, N, seed=43)
        xf = x.float()
        lin = (xf @ w.float().T) * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) + b.float()
        ref = swiglu_ref(lin) if glu else lin
        tag = f"gemm_rmsnorm {M}x{N}x{K}{' swiglu' if glu else ''}"

        def body(ar):
            A, W, Bv, C = ar.inp(x), ar.inp(w), ar.inp(b), ar.out(blank(M, N // 2 if glu else N, dt))
            assert len({A.stride(0), W.stride(0), C.stride(0)}) == 3
            ops.gemm_rmsnorm(A, W, Bv, out=C, epilogue=ops.EPI_SWIGLU if glu else ops.EPI_NONE, eps=1e-6)
            return {"C": C}
        three(fails, tag, body, lambda got: close16(got["C"], ref, tag, ulps=DECODE_ULPS[dt]))
    fails.done()


def packed_rows(ops, ar, x, B, out=False):
    """x (B, cols) row-major → its fragment-packed buffer, ceil(B / 16) blocks as a slab.  Input: the stale rows B .. 16 ceil(B / 16) - 1 of the
    last block hold the arena's poison (NaN / zeros) like everything behind the blocks.  Output: stale rows hold the sentinel."""
    B16 = (B + 15) // 16 * 16
    fill = SENTINEL if out else (float("nan") if ar.poison else 0.0)
    full = torch.full((B16, x.shape[1]), fill, dtype=x.dtype, device="cuda")
    full[:B] = x
    img = torch.empty_like(full)
    ops.pack_rows(full, img, B16, to_packed=True)
    return ar.out(img, slab=True) if out else ar.inp(img, slab=True)


def unpacked(ops, buf, B):
    un = torch.zeros(B, buf.shape[1], device="cuda", dtype=buf.dtype)
    ops.pack_rows(buf, un, B, to_packed=False)
    return un


@X16
@pytest.mark.parametrize("K", [264, 2080])
@pytest.mark.parametrize("N", [96, 704])
@pytest.mark.parametrize("B", [5, 40, 72])
@pytest.mark.parametrize("fp8", [False, True], ids=["w16", "w8"])
def test_packed_weight_projections_on_windows(ops, dt, fp8, B, N, K):
    """ops.gemm_packed / ops.gemm_packed_fp8 (MT = 1 / 4 / 8): A's K tail lies inside the last K-step (264 = 8 x 32 + 8; the fp8 image pairs
    K-steps: 2080 = 32 x 64 + 32) while the image's own zero padding — part of the image, not outside it — covers the weight side.
    Epilogues 0, 0 + norm + bias, 2 in place, 3 + norm; split-K 2 and 4 (epilogues 0 and 2); row-major A and C, and packed A / C / R."""
    ul = DECODE_ULPS[dt]
    x, w, b, r = rnd(dt, B, K, seed=51), rnd(dt, N, K, scale=0.05, seed=52), rnd(dt, N, seed=53), rnd(dt, B, N, seed=54)
    wi = interleave_gate_up(w[: N // 2].contiguous(), w[N // 2:].contiguous())
    if fp8:
        q, sc, w = ops.quantize_fp8_rows(w, deq_dtype=dt)             # w := the dequantised matrix, exact in both 16-bit types
        qi, sci, wi = ops.quantize_fp8_rows(wi, deq_dtype=dt)
        img, img_i = ops.pack_weight_fp8(q), ops.pack_weight_fp8(qi)
    else:
        img, img_i = ops.pack_weight(w), ops.pack_weight(wi)
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)
    lin, lin_i = xf @ w.float().T, xf @ wi.float().T
    variants = [("plain", 0, False, 1), ("norm+bias", 0, True, 1), ("resid", 2, False, 1), ("swiglu+norm", 3, True, 1),
                ("plain split2", 0, False, 2), ("plain split4", 0, False, 4), ("resid split2", 2, False, 2), ("resid split4", 2, False, 4)]
    fails = Failures()
    for name, epi, norm, split in variants:
        n_out = N // 2 if epi == 3 else N
        ref = {"plain": lin, "norm+bias": lin * rstd + b.float(), "resid": lin + r.float(), "swiglu+norm": swiglu_ref(lin_i * rstd)}[name.split(" ")[0]]
        for packed in (False, True):
            tag = f"gemm_packed{'_fp8' if fp8 else ''} {name} {'packed' if packed else 'row-major'} {B}x{N}x{K}"

            def body(ar):
                Wp = ar.inp(img_i if epi == 3 else img, slab=True)
                kw = dict(scales=ar.inp(sci if epi == 3 else sc)) if fp8 else {}
                if name == "norm+bias":
                    kw["bias"] = ar.inp(b)
                if split > 1:
                    kw.update(split_k=split, workspace=ops.new_splitk_workspace(N, split, "cuda"))
                if packed:
                    A = packed_rows(ops, ar, x, B)
                    C = packed_rows(ops, ar, r if epi == 2 else blank(B, n_out, dt), B, out=True)
                    kw.update(a_packed=True, c_packed=True, rows=B)
                else:
                    A, C = ar.inp(x), ar.out(r if epi == 2 else blank(B, n_out, dt))
                ops.gemm_packed(A, Wp, N, out=C, epilogue=epi, residual=C if epi == 2 else None, norm_eps=1e-6 if norm else None, **kw)
                return {"C": unpacked(ops, C, B) if packed else C}
            three(fails, tag, body, lambda got: close16(got["C"], ref, tag, ulps=ul))
    fails.done()


@X16
@pytest.mark.parametrize("K", [264, 2080])
@pytest.mark.parametrize("N", [96, 704])
@pytest.mark.parametrize("B", [5, 40, 72])
def test_packed_resid32_on_windows(ops, dt, B, N, K):
    """ops.gemm_packed_resid32: the fp32 stream in place in a row-major window, its mirror as a packed slab; 16-bit and fp8 weight images,
    split-K 1 / 2 / 4, packed and row-major A."""
    s = ops.stream_scale(dt)
    x, w = rnd(dt, B, K, seed=61), rnd(dt, N, K, scale=0.05, seed=62)
    x0 = rnd(F32, B, N, seed=63)
    q, sc, deq = ops.quantize_fp8_rows(w, deq_dtype=dt)
    fails = Failures()
    for fp8, split, a_packed in [(False, 1, True), (False, 2, True), (False, 4, True), (False, 1, False), (False, 4, False), (True, 1, True), (True, 2, False)]:
        img = ops.pack_weight_fp8(q) if fp8 else ops.pack_weight(w)
        ref = x0 + x.float() @ (deq if fp8 else w).float().T
        tag = f"gemm_packed_resid32 {'fp8 ' if fp8 else ''}split{split} {'packed' if a_packed else 'row-major'} A {B}x{N}x{K}"

        def body(ar):
            Wp = ar.inp(img, slab=True)
            A = packed_rows(ops, ar, x, B) if a_packed else ar.inp(x)
            X, XB = ar.out(x0), packed_rows(ops, ar, blank(B, N, dt), B, out=True)
            ops.gemm_packed_resid32(A, Wp, N, X, XB, scales=ar.inp(sc) if fp8 else None, split_k=split,
                                    workspace=ops.new_splitk_workspace(N, split, "cuda") if split > 1 else None, a_packed=a_packed, rows=B)
            return {"x32": X, "xb": unpacked(ops, XB, B)}

        def check(got):
            close_f32(got["x32"], ref, tag, rel=3e-5)
            assert torch.equal(got["xb"], (got["x32"] * s).to(dt)), f"{tag}: packed mirror != X(stream_scale * stream)"
        three(fails, tag, body, check)
    fails.done()


# ------------------------------------------------------------------------------------------------------------ fp8 MFMA
def _dequant8(q, scale):
    return q.view(torch.float8_e4m3fn).float() * scale[:, None]


@X16
@pytest.mark.parametrize("N,K", [(256, 128), (512, 256)])
@pytest.mark.parametrize("mf", [2, 3, 4])
def test_gemm_fp8_on_windows(ops, knobs, dt, mf, N, K):
    """ops.gemm_fp8 at every tile height, M = one tile row + 24: e4m3 operands at lda, ldw = larger multiples of 16 than K with the NaN code
    around them, row_scale / col_scale / bias in NaN-surrounded vectors; epilogues 0, 3 and 2 (fp32 stream + mirror).  dt is the type of
    the bias, the output and the mirror.  Operands and tolerance are the parity tests': bf16 output with one weight row 30 x the others at
    ulps = 1 (test_kernels_gpu.py), fp16 output with plain randn weights at ulps = 2 (test_kernels_f16_gpu.py: the fp8 MFMA's own summation
    error, 2^-15 of a dot product's magnitude sum, is an fp16 step of its own)."""
    knobs(mf=mf)
    M = 64 * mf + 24
    x, w, b = rnd(dt, M, K, seed=71), rnd(BF, N, K, scale=0.05, seed=72), rnd(dt, N, seed=73)
    if dt == BF:
        w[7] *= 30.0
    a8, rs = ops.quant_rows_fp8(x)
    w8, cs, _ = ops.quantize_fp8_rows(w)
    ref = _dequant8(a8, rs) @ _dequant8(w8, cs).T
    mag = _dequant8(a8, rs).abs() @ _dequant8(w8, cs).abs().T
    x0 = rnd(F32, M, N, seed=74)
    s = ops.stream_scale(dt)
    fails = Failures()
    for epi in (0, 3, 2):
        tag = f"gemm_fp8 mf{mf} epilogue {epi} {M}x{N}x{K}"

        def body(ar):
            A, W, RS, CS, Bv = ar.inp(a8), ar.inp(w8), ar.inp(rs), ar.inp(cs), ar.inp(b)
            assert A.stride(0) != W.stride(0) and A.stride(0) > K and A.stride(0) % 16 == 0 and W.stride(0) % 16 == 0
            if epi == 2:
                X, XB = ar.out(x0), ar.out(blank(M, N, dt))
                ops.gemm_fp8(A, W, CS, RS, bias=Bv, epilogue=ops.EPI_RESID, x32=X, xb=XB)
                return {"x32": X, "xb": XB}
            C = ar.out(blank(M, N // 2 if epi == 3 else N, dt))
            ops.gemm_fp8(A, W, CS, RS, bias=Bv, out=C, epilogue=epi)
            return {"C": C}

        def check(got):
            if epi == 2:
                err = (got["x32"] - (x0 + ref + b.float())).abs()
                bad = err > 3e-5 * mag + 1e-6
                assert not bad.any(), f"{tag}: {int(bad.sum())} outside 3e-5 of the magnitude sum, worst {(err / (mag + 1e-9)).max().item():.2e}"
                assert torch.equal(got["xb"], (got["x32"] * s).to(dt)), f"{tag}: mirror != X(stream_scale * stream)"
            else:
                close16(got["C"], swiglu_ref(ref + b.float()) if epi == 3 else ref + b.float(), tag, ulps=1.0 if dt == BF else 2.0)
        three(fails, tag, body, check)
    fails.done()


# ------------------------------------------------------------------------------------------------------------ split-precision few rows
@pytest.mark.parametrize("N", [4, 64])
@pytest.mark.parametrize("M", [9, 64])
def test_gemm_split_rows_on_windows(ops, M, N):
    """padt_gemm_split_rows through ops.gemm_hp (M <= 64): fp32 output plain and with the fp32 residual in place, the split SwiGLU (N = 64
    only: N % 32), each with and without the packed weight image (N % 16: N = 64 only).  With w_packed the wrapper packs the rows itself and
    takes that path only for rows at their natural stride (lda = 2K): A is a slab there — the nearest window the entry point accepts."""
    K = 320
    a_s, a64 = split_operands(M, K, 81)
    w, b = rnd(BF, N, K, scale=0.05, seed=82), rnd(BF, N, scale=0.1, seed=83)
    w2 = torch.cat([w, w], dim=1).contiguous()
    x0 = rnd(F32, M, N, seed=84)
    lin = a64 @ w.double().T + b.double()
    fails = Failures()
    for w_packed in ([False, True] if N % 16 == 0 else [False]):
        for resid in (False, True):
            tag = f"split_rows f32{' resid' if resid else ''}{' w_packed' if w_packed else ''} {M}x{N}x{K}"
            ref = lin + x0.double() if resid else lin

            def body(ar):
                A, W2, Bv = ar.inp(a_s, slab=w_packed), ar.inp(w2), ar.inp(b)
                C = ar.out(x0 if resid else blank(M, N, F32))
                kw = dict(w_packed=ar.inp(ops.pack_weight(w), slab=True)) if w_packed else {}
                ops.gemm_hp(A, W2, Bv, out=C, epilogue=ops.EPI_RESID if resid else ops.EPI_NONE, residual=C if resid else None, **kw)
                return {"C": C}

            def check(got):
                assert rel_err(got["C"], ref) < 5e-5, f"{tag}: rel err {rel_err(got['C'], ref):.2e}"
            three(fails, tag, body, check)
        if N % 32 == 0:
            hp_split_case(ops, fails, M, N, K, True, f"split_rows swiglu{' w_packed' if w_packed else ''} {M}x{N}x{K}", w_packed=w_packed, slab_a=w_packed)
    fails.done()


# ------------------------------------------------------------------------------------------------------------ non-finite locality
def _glu_col(n):
    return (n >> 5) * 16 + (n & 15)


def _plant(t, plant, side):
    """→ t, or a copy with the planted value at [row, k] when the plant is on this side ("A" / "W")"""
    if plant is None or plant[0] != side:
        return t
    t = t.clone()
    t[plant[1], plant[2]] = plant[3]
    return t


def _gemm_family(ops, dt, M, N, K, n_glu, extra=()):
    """ops.gemm under every epilogue → {name: (output, column map)}; extra: "resid32", "rope" (A-side plants only)."""
    def run(plant, plain_only):
        a, w, b = _plant(rnd(dt, M, K, seed=1), plant, "A"), rnd(dt, N, K, scale=0.05, seed=2), rnd(dt, N, seed=3)
        wp = _plant(w, plant, "W")
        r, rs = rnd(dt, M, N, seed=4), pos(M, seed=5)
        out = {"none": (ops.gemm(a, wp, b), None)}
        if plain_only:
            return out
        out["gelu"] = (ops.gemm(a, wp, b, epilogue=ops.EPI_GELU), None)
        out["resid"] = (ops.gemm(a, wp, b, epilogue=ops.EPI_RESID, residual=r), None)
        o32 = torch.zeros(M, N, device="cuda")
        out["f32"] = (ops.gemm(a, wp, None, out=o32, out_f32=True), None)
        out["row_scale"] = (ops.gemm(a, wp, b, row_scale=rs), None)
        wg = _plant(rnd(dt, n_glu, K, scale=0.05, seed=6), plant, "W")
        out["swiglu"] = (ops.gemm(a, wg, rnd(dt, n_glu, seed=7), epilogue=ops.EPI_SWIGLU), _glu_col)
        if "resid32" in extra:
            x32, xb = rnd(F32, M, N, seed=8), torch.zeros(M, (N + 7) // 8 * 8, device="cuda", dtype=dt)[:, :N]     # the mirror's stride: % 8
            ops.gemm_resid32(a, wp, b, x32, xb)
            out["x32"], out["xb"] = (x32, None), (xb, None)
        if "rope" in extra and (plant is None or plant[0] == "A"):
            cs = torch.rand(M, 20, generator=torch.Generator().manual_seed(9)).cuda()
            o = torch.zeros(M, N, device="cuda", dtype=dt)
            out["rope"] = (ops.gemm_rope(a, w, b, o, cs, cs.clone(), 80, 40, row_scale=rs), None)
        return out
    return run


def _norm_family(ops, dt):
    M, K = 20, 264

    def run(plant, plain_only):
        a = _plant(rnd(dt, M, K, seed=1), plant, "A")
        out = {"none": (ops.gemm_rmsnorm(a, _plant(rnd(dt, 96, K, scale=0.05, seed=2), plant, "W"), rnd(dt, 96, seed=3)), None)}
        if not plain_only:
            out["swiglu"] = (ops.gemm_rmsnorm(a, _plant(rnd(dt, 64, K, scale=0.05, seed=4), plant, "W"), None, epilogue=ops.EPI_SWIGLU), _glu_col)
        return out
    return run, M, 64, K


def _packed_family(ops, dt, fp8):
    """gemm_packed at split-K 4 (16-bit image; epilogues 0 and 2, what split-K has) or over the fp8 image (0 + norm, 2, 3 + norm; a NaN weight is
    the e4m3 NaN code in the image), packed activations, plus gemm_packed_resid32."""
    B, N, K = 40, 96, 2080 if not fp8 else 264
    B16 = 48

    def run(plant, plain_only):
        x = _plant(rnd(dt, B, K, seed=1), plant, "A")
        w, r = rnd(dt, N, K, scale=0.05, seed=2), rnd(dt, B, N, seed=3)
        xp = torch.zeros(B16, K, device="cuda", dtype=dt)
        ops.pack_rows(x, xp, B, to_packed=True)
        if fp8:
            q, sc, _ = ops.quantize_fp8_rows(w)
            if plant is not None and plant[0] == "W":
                q = q.clone()
                q[plant[1], plant[2]] = 0x7F
            img, kw = ops.pack_weight_fp8(q), dict(scales=sc)
        else:
            img, kw = ops.pack_weight(_plant(w, plant, "W")), dict(split_k=4)
        ws = lambda: {} if fp8 else dict(workspace=ops.new_splitk_workspace(N, 4, "cuda"))

        def go(epi, norm, res=None):
            c = torch.zeros(B16, N // 2 if epi == 3 else N, device="cuda", dtype=dt)
            if res is not None:
                ops.pack_rows(res, c, B, to_packed=True)
            ops.gemm_packed(xp, img, N, out=c, epilogue=epi, residual=c if epi == 2 else None, norm_eps=1e-6 if norm else None,
                            a_packed=True, c_packed=True, rows=B, **kw, **ws())
            return unpacked(ops, c, B)
        out = {"none": (go(0, fp8), None)}
        if plain_only:
            return out
        out["resid"] = (go(2, False, r), None)
        if fp8:
            out["swiglu"] = (go(3, True), _glu_col)
        x32, mir = rnd(F32, B, N, seed=4), torch.zeros(B16, N, device="cuda", dtype=dt)
        ops.gemm_packed_resid32(xp, img, N, x32, mir, rows=B, **kw, **ws())
        out["x32"], out["xb"] = (x32, None), (unpacked(ops, mir, B), None)
        return out
    return run, B, N, K


def _fp8_mfma_family(ops, dt):
    """The planted value goes into row_scale[r] / col_scale[n]: e4m3 operands made by quant_rows_fp8 do not carry an inf."""
    M, N, K = 64 * 3 + 24, 256, 128

    def run(plant, plain_only):
        a8, rs = ops.quant_rows_fp8(rnd(dt, M, K, seed=1))
        w8, cs, _ = ops.quantize_fp8_rows(rnd(BF, N, K, scale=0.05, seed=2))
        b = rnd(dt, N, seed=3)
        if plant is not None:
            (rs if plant[0] == "A" else cs)[plant[1]] = plant[3]
        out = {"none": (ops.gemm_fp8(a8, w8, cs, rs, bias=b), None)}
        if plain_only:
            return out
        out["swiglu"] = (ops.gemm_fp8(a8, w8, cs, rs, bias=b, epilogue=ops.EPI_SWIGLU), _glu_col)
        x32, xb = rnd(F32, M, N, seed=4), torch.zeros(M, N, device="cuda", dtype=dt)
        ops.gemm_fp8(a8, w8, cs, rs, bias=b, epilogue=ops.EPI_RESID, x32=x32, xb=xb)
        out["x32"], out["xb"] = (x32, None), (xb, None)
        return out
    return run, M, N, K


def _hp_family(ops, M, N, K, n_glu):
    """gemm_hp: few rows → padt_gemm_split_rows (fp32 plain / residual, split SwiGLU); more → the tile kernels (also the split output).  A plant
    on the A side goes into the hi half of the split rows."""
    def run(plant, plain_only):
        a_s = _plant(split_operands(M, K, 1)[0], plant, "A")
        w, b = _plant(rnd(BF, N, K, scale=0.05, seed=2), plant, "W"), rnd(BF, N, scale=0.1, seed=3)
        w2 = torch.cat([w, w], dim=1).contiguous()
        out = {"none": (ops.gemm_hp(a_s, w2, b)[:, :N], None)}
        if plain_only:
            return out
        x32 = rnd(F32, M, N, seed=4)
        out["resid"] = (ops.gemm_hp(a_s, w2, b, out=x32, epilogue=ops.EPI_RESID, residual=x32), None)
        if M > 64:
            sp = ops.gemm_hp(a_s, w2, b, out_mode=ops.OUT_SPLIT)
            out["hi"], out["lo"] = (sp[:, :N], None), (sp[:, N:], None)
        wg = _plant(rnd(BF, n_glu, K, scale=0.05, seed=5), plant, "W")
        g = ops.gemm_hp(a_s, torch.cat([wg, wg], dim=1).contiguous(), rnd(BF, n_glu, scale=0.1, seed=6), epilogue=ops.EPI_SWIGLU, out_mode=ops.OUT_SPLIT)
        out["glu hi"], out["glu lo"] = (g[:, : n_glu // 2], _glu_col), (g[:, n_glu // 2:], _glu_col)
        return out
    return run


FAMILIES = ["skinny MT4", "tile128", "tile256 mf3 peel2", "fused norm", "packed split-K 4", "packed fp8 weights", "fp8 MFMA", "split_rows", "gemm_hp tiles"]
BF16_ONLY = {"split_rows", "gemm_hp tiles"}                          # the split-precision entries have one operand type


def _family(ops, name, dt):
    """→ (run, M, weight rows that plain and SwiGLU weights both have, K)"""
    if name == "skinny MT4":
        return _gemm_family(ops, dt, 40, 40, 72, 64), 40, 40, 72
    if name == "tile128":
        return _gemm_family(ops, dt, 300, 260, 136, 288), 300, 260, 136
    if name == "tile256 mf3 peel2":
        ops.gemm_knobs(mode256=2, mf=3, peel=2)
        return _gemm_family(ops, dt, 2 * 192 + 24, 300, 128, 320, extra=("resid32", "rope")), 2 * 192 + 24, 300, 128
    if name == "fused norm":
        return _norm_family(ops, dt)
    if name == "packed split-K 4":
        return _packed_family(ops, dt, False)
    if name == "packed fp8 weights":
        return _packed_family(ops, dt, True)
    if name == "fp8 MFMA":
        return _fp8_mfma_family(ops, dt)
    if name == "split_rows":
        return _hp_family(ops, 9, 64, 320, 64), 9, 64, 320
    return _hp_family(ops, 300, 300, 64, 320), 300, 300, 64


@pytest.mark.parametrize("name,dt", [(f, t) for f in FAMILIES for t in ([BF] if f in BF16_ONLY else [BF, F16])],
                         ids=lambda v: v if isinstance(v, str) else {BF: "bf16", F16: "fp16"}[v])
def test_nonfinite_values_stay_in_their_row_and_column(ops, knobs, name, dt):
    """One planted non-finite value in otherwise clean, contiguous operands (the module docstring has the rules).  Rows: 0 and one of the
    ragged last tile / peeled tail / last row block; k: in the K tail's last chunk; weight rows: 1 and one of the last (ragged) block."""
    run, M, N, K = _family(ops, name, dt)
    clean = run(None, False)
    torch.cuda.synchronize()
    for nm, (o, _) in clean.items():
        assert torch.isfinite(o.float()).all(), f"{name} {nm}: the clean run is not finite"
    fails = Failures()
    nan, inf = float("nan"), float("inf")
    for r in (0, M - 2):
        for val in (nan, inf):
            got = run(("A", r, K - 3, val), val == inf)
            for nm, (o, _) in got.items():
                with fails.step(f"{name} {nm}: {val} at A[{r}, {K - 3}]"):
                    row = o[r].float()
                    assert bool(torch.isnan(row).all() if val != inf else (~torch.isfinite(row)).all()), \
                        f"{int(torch.isfinite(row).sum())} of {row.numel()} outputs of the row are finite"
                    keep = torch.arange(M, device="cuda") != r
                    assert same_bits(o[keep], clean[nm][0][keep]), \
                        f"rows {sorted(set((o != clean[nm][0]).nonzero()[:, 0].tolist()) - {r})[:8]} changed too"
    for n in (1, N - 2):
        got = run(("W", n, K - 3, nan), False)
        for nm, (o, colmap) in got.items():
            with fails.step(f"{name} {nm}: NaN at W[{n}, {K - 3}]"):
                c = n if colmap is None else colmap(n)
                assert bool(torch.isnan(o[:, c].float()).all()), f"column {c}: {int(torch.isfinite(o[:, c].float()).sum())} of {M} outputs are finite"
                keep = torch.arange(o.shape[1], device="cuda") != c
                assert same_bits(o[:, keep], clean[nm][0][:, keep]), \
                    f"columns {sorted(set((o != clean[nm][0]).nonzero()[:, 1].tolist()) - {c})[:8]} changed too"
    fails.done()
