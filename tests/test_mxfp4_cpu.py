"""MXFP4 weights, host side (ops.quantize_mxfp4_rows / pack_weight_fp4 / unpack_weight_fp4, weights.prepare_weights): the format's statement
sign * grid[code] * 2^e, the scale rule, the rounding rule, the exponent clamp of the fp16 image and the decode-image layout.  No GPU."""
import pytest
import torch

from padt_amd import ops

BF, F16 = torch.bfloat16, torch.float16
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
ROW_BIG, ROW_SMALL, ROW_TINY, ROW_ZERO_BLOCK = 3, 5, 7, 9


def matrix(dt):
    """64 x 256, N(0, 0.05^2), with one row x40, one x1e-3, one x1e-6 (block amax ≈ 1.5e-7: below what the fp16 exponent clamp allows) and one
    all-zero block — values representable in the 16-bit type the model would hold them in."""
    g = torch.Generator().manual_seed(4)
    w = torch.randn(64, 256, generator=g) * 0.05
    w[ROW_BIG] *= 40.0
    w[ROW_SMALL] *= 1e-3
    w[ROW_TINY] *= 1e-6
    w[ROW_ZERO_BLOCK, 32:64] = 0.0
    return w.to(dt)


def statement(codes, exps):
    """sign * grid[code] * 2^(E8M0 - 127) in fp64, written out here independently of the library's helper."""
    N, K = codes.shape[0], codes.shape[1] * 2
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).view(N, K).long()
    v = GRID[nib & 7] * (1.0 - 2.0 * ((nib >> 3) & 1).double())
    return (v.view(N, K // 32, 32) * torch.exp2(exps.double() - 127.0)[..., None]).view(N, K)


@pytest.mark.parametrize("dt", [BF, F16])
def test_quantiser_statement_scale_rule_and_error_bound(dt):
    w = matrix(dt)
    codes, exps, deq = ops.quantize_mxfp4_rows(w, dt)
    assert codes.dtype == torch.uint8 and codes.shape == (64, 128) and exps.dtype == torch.uint8 and exps.shape == (64, 8)
    assert deq.dtype == dt and deq.shape == w.shape
    assert int(exps.min()) >= 1 and int(exps.max()) <= 254                       # valid E8M0 (255 is NaN), and a normal fp32 scale
    st = statement(codes, exps)
    assert torch.equal(st, deq.double()), "w_deq is not sign * grid[code] * 2^e"
    assert torch.equal(st.to(dt).double(), st), "the dequantised matrix is not exactly representable in its 16-bit type"
    assert torch.equal(st, ops.dequantize_mxfp4(codes, exps))
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).view(64, 256)
    assert not (nib == 8).any(), "a zero must be stored as +0"
    wb, sb = w.double().view(64, 8, 32), st.view(64, 8, 32)
    amax, e = wb.abs().amax(-1), exps.double() - 127.0
    e_min = ops.mxfp4_min_exponent(dt)
    assert e_min == (-23 if dt == F16 else -126)
    clamped = (amax > 0) & (amax <= 3.0 * torch.exp2(e))                          # an un-clamped block has 3 * 2^e < amax <= 6 * 2^e
    zero = amax == 0
    assert bool(zero[ROW_ZERO_BLOCK, 1]) and int(zero.sum()) == 1
    assert (e[zero] == e_min).all() and (sb[zero] == 0).all()
    assert (e[clamped] == e_min).all()
    if dt == F16:                                                                # the clamp bites for fp16 only, and there on the whole x1e-6 row
        assert bool(clamped[ROW_TINY].all()) and int(clamped.sum()) == 8
    else:
        assert not clamped.any()
    free = ~clamped & ~zero
    assert (amax[free] <= 6.0 * torch.exp2(e[free])).all() and (amax[free] > 3.0 * torch.exp2(e[free])).all()   # e = ceil(log2(amax / 6))
    err = (sb - wb).abs().amax(-1)
    assert (5.0 * err[free] <= amax[free]).all(), "quantisation error above amax_block / 5"
    assert (err[clamped] <= 0.5 * 2.0 ** e_min).all()                            # clamped: amax <= 3 * 2^e, where the grid spacing is at most 1
    # rows of very different magnitude really got different exponents
    assert int(exps[ROW_BIG].min()) > int(exps[0].max()) > int(exps[ROW_SMALL].max())


@pytest.mark.parametrize("dt", [BF, F16])
@pytest.mark.parametrize("p2", [2.0 ** -9, 1.0, 8.0])
def test_ties_go_to_the_even_code(dt, p2):
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]                                    # codes 0, 2, 2, 4, 4, 6, 6
    w = torch.zeros(2, 32, dtype=torch.float64)
    w[:, 0] = 6.0                                                                  # pins the block scale at 2^0 (times p2)
    w[0, 1:8] = torch.tensor(ties)
    w[1, 1:8] = -torch.tensor(ties)
    w[:, 8:15] = w[:, 1:8] * (1 + 2.0 ** -7)                                       # just above a tie: the next grid point up
    w[:, 15:22] = w[:, 1:8] * (1 - 2.0 ** -7)
    codes, exps, deq = ops.quantize_mxfp4_rows((w * p2).to(dt), dt)
    assert (exps.double() - 127.0 == torch.log2(torch.tensor(p2))).all()
    d = deq.double() / p2
    up = [0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    dn = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0]
    for r, sgn in ((0, 1.0), (1, -1.0)):
        assert d[r, 1:8].tolist() == [sgn * v if v else 0.0 for v in want], d[r, 1:8]
        assert d[r, 8:15].tolist() == [sgn * v for v in up]
        assert d[r, 15:22].tolist() == [sgn * v if v else 0.0 for v in dn]
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).view(2, 32)
    assert nib[0, 1:8].tolist() == [0, 2, 2, 4, 4, 6, 6] and nib[1, 1:8].tolist() == [0, 10, 10, 12, 12, 14, 14]


@pytest.mark.parametrize("N,K", [(64, 256), (40, 96), (16, 64), (33, 2080)])
def test_pack_unpack_round_trip_and_layout(N, K):
    g = torch.Generator().manual_seed(N + K)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    exps = torch.randint(1, 255, (N, K // 32), generator=g, dtype=torch.uint8)
    img, ep = ops.pack_weight_fp4(codes, exps)
    Np, Kp = (N + 15) // 16 * 16, (K + 63) // 64 * 64
    assert img.shape == (Np, Kp // 2) and ep.shape == (Np // 16, Kp // 64, 16, 2) and img.is_contiguous() and ep.is_contiguous()
    c2, e2 = ops.unpack_weight_fp4(img, ep, N, K)
    assert torch.equal(c2, codes) and torch.equal(e2, exps)
    # the layout, spelled out for a few elements: tile (n16, kp) is 512 B, lane fq*16 + frow, byte half*4 + j/2, nibble j % 2
    flat = img.view(-1)
    for n, k in [(0, 0), (N - 1, K - 1), (N // 2, 37), (min(N - 1, 17), K - 33)]:
        n16, frow, kp, half, fq, j = n // 16, n % 16, k // 64, (k % 64) // 32, (k % 32) // 8, k % 8
        byte = int(flat[((n16 * (Kp // 64) + kp) * 64 + fq * 16 + frow) * 8 + half * 4 + j // 2])
        assert (byte >> (4 * (j % 2))) & 15 == (int(codes[n, k // 2]) >> (4 * (k % 2))) & 15, (n, k)
        assert int(ep[n16, kp, frow, half]) == int(exps[n, k // 32])
    # padding: zero codes
    full_c, full_e = ops.unpack_weight_fp4(img, ep, Np, Kp)
    assert (full_c[N:] == 0).all() and (full_c[:, K // 2:] == 0).all()
    assert int(full_e.min()) >= 1 and int(full_e.max()) <= 254


def test_k_must_be_whole_blocks():
    with pytest.raises(ValueError, match="multiple"):
        ops.quantize_mxfp4_rows(torch.zeros(16, 48))
    with pytest.raises(ValueError, match="multiple"):
        ops.quantize_mxfp4_rows(torch.zeros(16, 2072), F16)


def test_prepare_weights_rejects_fp4_act_and_unknown_modes():
    import padt_amd
    from padt_amd.weights import prepare_weights
    cfg = padt_amd.small_test_config()
    with pytest.raises(ValueError, match="fp4\\+act"):
        prepare_weights({}, cfg, device="cpu", llm_weights="fp4+act")
    with pytest.raises(ValueError, match="llm_weights must be"):
        prepare_weights({}, cfg, device="cpu", llm_weights="int4")
    with pytest.raises(ValueError, match="llm_weights must be"):
        prepare_weights({}, cfg, device="cpu", llm_weights="FP4")


def test_c_entry_points_validate_before_any_launch():
    """padt_gemm_packed_fp4 / padt_gemm_packed_resid32_fp4 and their fp16 twins: null images, K % 32, N % 16 and a misaligned exponent array
    are answered with -1 and a message naming the entry point, without touching a device."""
    import os
    from padt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from padt_amd.build import build
        build()
    lib = _lib.load()
    for sfx in ("", "_f16"):
        f, r = getattr(lib, "padt_gemm_packed_fp4" + sfx), getattr(lib, "padt_gemm_packed_resid32_fp4" + sfx)
        assert f(None, 16, 64, None, 64, 32, None, 16, 32, None, 0, 8, 32, 64, 0, -1.0, 1, None, 0) == -1           # no nibble image
        assert b"padt_gemm_packed_fp4" in lib.padt_last_error()
        assert f(None, 16, 64, 16, 64, None, None, 16, 32, None, 0, 8, 32, 64, 0, -1.0, 1, None, 0) == -1           # no exponents
        assert f(None, 16, 64, 16, 64, 32, None, 16, 32, None, 0, 8, 32, 40, 0, -1.0, 1, None, 0) == -1             # K % 32
        assert b"K % 32 == 0" in lib.padt_last_error()
        assert f(None, 16, 64, 16, 64, 32, None, 16, 24, None, 0, 8, 24, 64, 0, -1.0, 1, None, 0) == -1             # N % 16
        assert f(None, 16, 64, 16, 64, 34, None, 16, 32, None, 0, 8, 32, 64, 0, -1.0, 1, None, 0) == -1             # exponents not 16-byte aligned
        assert f(None, 16, 64, 16, 96, 32, None, 16, 32, None, 0, 8, 32, 64, 0, -1.0, 1, None, 0) == -1             # Kp % 64
        assert r(None, 16, 64, 16, 64, 32, 16, 32, None, 32, 8, 32, 64, 1, None, 1) == -1                            # no packed mirror
        assert b"padt_gemm_packed_resid32_fp4" in lib.padt_last_error()
        assert r(None, 16, 64, None, 64, 32, 16, 32, 16, 32, 8, 32, 64, 1, None, 1) == -1
        assert f(None, 16, 64, 16, 64, 32, None, 16, 32, None, 0, 0, 32, 64, 0, -1.0, 1, None, 0) == 0              # zero rows: a no-op success
