"""The mask tail of post-processing (padt_mask_upsample_binarize, padt_mask_scatter, padt_mask_scatter_f32) and the image front-end's
padt_patchify_normalize on windows in poisoned buffers (tests/edge_util.py; the rules of tests/test_row_edges_gpu.py apply):
  * index, offset and size tensors are NEVER poisoned — cu_patch, obj_w, src_h / src_w, dst_h / dst_w: their values are addresses.  They
    are passed contiguous and in range.
  * every window keeps edge_util's margins (256 rows, 128 elements), so an overrun by a row or a vector stays inside the allocation and
    fails an assertion instead of faulting.
Every case goes through three(): the NaN-poisoned run meets the reference, is bit-identical to the zero-filled run, and nothing outside
an output window changed (uint8 outputs: the byte sentinel 0xA5).  Tolerances are those of the parity tests: up-sampled logits within
2e-6 of the largest logit + 1e-6 of F.interpolate(mode="bilinear") on the valid region (computed on the CPU, as that test does: the
seeds' margin is a property of this very reference, tests/test_mask_edges_cpu.py), binary masks EXACTLY equal — the seeds leave no
reference logit within 1e-5 of the threshold, asserted here too —, mask_scatter at rel = 1e-5, patchify bit-exact in fp32 and its one
rounding in bf16 / fp16.

The up-sampler's launch extents (max_h, max_w) are the size of an output plane.  An object larger than them is CROPPED: the kernel
writes x < min(dst_w[o], max_w) only (rows are bounded by the grid), and padt_mask_rle on the result reports the object.
"""
import numpy as np
import pytest
import torch

import mask_edge_util as M
from edge_util import Failures, same_bits, three
from test_decoder_hp_gpu import rel_err
from test_kernels_gpu import close_f32

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
U8_INIT, F32_INIT = 9, 3.0                                           # what the output planes hold before the launch


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def i32(v):
    return torch.as_tensor(v, dtype=torch.int32).cuda().contiguous()


def upsample_case(ops, fails, objects, seed, extent, tag):
    """objects of mask_edge_util in ONE launch: masks, the byte planes and the logit planes are windows at strides of their own.  →
    the NaN run's (out, up) as contiguous tensors."""
    masks, refs = M.build(objects, seed)
    assert M.margin(refs) >= M.MARGIN, f"{tag}: a reference logit lies within {M.MARGIN} of the threshold — choose another seed"
    n, (mh, mw) = len(objects), extent
    hs, ws, dh, dw = (i32([o[k] for o in objects]) for k in range(4))
    kept = {}

    def body(ar):
        Mk = ar.inp(masks.view(n * M.HM, M.WM).cuda()).view(n, M.HM, M.WM)
        out = ar.out(torch.full((n * mh, mw), U8_INIT, dtype=torch.uint8, device="cuda")).view(n, mh, mw)
        up = ar.out(torch.full((n * mh, mw), F32_INIT, device="cuda")).view(n, mh, mw)
        assert len({Mk.stride(1), out.stride(1), up.stride(1)}) == 3
        ops.mask_upsample_binarize(Mk, hs, ws, dh, dw, mh, mw, out=out, up=up)
        return {"out": out, "up": up}

    def check(got):
        kept.update(got)
        for o, (_, _, h, w) in enumerate(objects):
            hh, ww = min(h, mh), min(w, mw)                          # an object beyond the launch extents is cropped
            ref = refs[o][:hh, :ww]
            err = (got["up"][o, :hh, :ww].cpu() - ref).abs().max().item()
            assert err <= 2e-6 * refs[o].abs().max().item() + 1e-6, f"{tag} object {o}: up-sampled logits off by {err:.3e}"
            diff = got["out"][o, :hh, :ww].cpu().bool() != (ref.sigmoid() > 0.5)
            assert not diff.any(), f"{tag} object {o}: {int(diff.sum())} binary pixels differ (no reference logit is within 1e-5 of the threshold)"
            pad = torch.ones(mh, mw, dtype=torch.bool, device="cuda")
            pad[:hh, :ww] = False
            assert bool((got["out"][o][pad] == U8_INIT).all()) and bool((got["up"][o][pad] == F32_INIT).all()), \
                f"{tag} object {o}: the padding of its plane changed"
    three(fails, tag, body, check)
    return kept, dh, dw


def test_mask_upsample_binarize_mixed_objects_on_windows(ops):
    """1 x 1, 4 x 4 and 37 x 21 sources in (40, 24) planes whose contents outside the valid regions are NaN (never to be read); destinations
    1 x 1, 19 x 50 (down), 97 x 300 (up, two x-blocks) and widths of exactly 256 and 257, in one launch."""
    fails = Failures()
    upsample_case(ops, fails, M.MIXED, M.SEED["mixed"], M.MIXED_EXTENT, "mixed sizes")
    fails.done()


def test_mask_upsample_binarize_crops_an_object_beyond_the_launch_extents(ops):
    """An object 2 taller and 3 wider than (max_h, max_w) = (20, 30): inside the extents it equals the cropped reference, outside every
    byte and float is untouched (its neighbour's plane and the margins included), and mask_rle on the result reports it."""
    fails = Failures()
    got, dh, dw = upsample_case(ops, fails, M.CROPPED, M.SEED["cropped"], M.CROPPED_EXTENT, "oversize object")
    with fails.step("mask_rle reports the cropped object"):
        h = ops.mask_rle_launch(got["out"].contiguous(), dh, dw)
        assert ops.mask_rle_fetch(h, on_overflow="none") is None
        nc = h["n_counts"].cpu().tolist()
        assert nc[0] == -1 and nc[1] > 0, nc
    fails.done()


@pytest.mark.parametrize("dm", [80, 20])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_mask_scatter_on_windows(ops, dt, dm):
    """padt_mask_scatter (bf16) / padt_mask_scatter_f32: e2 and mask_tok NaN-poisoned windows, masks a slab of 7.0 with sentinel rows around
    it; grids smaller than the (6, 8) plane and an object without patches in the middle (cu[2] == cu[3]).  Inside each grid the
    reference holds; everything else of the slab keeps its bits."""
    Hm, Wm = 6, 8
    grids = [(6, 8), (3, 5), (0, 1), (4, 4)]
    n_obj = len(grids)
    cu = [0]
    for h, w in grids:
        cu.append(cu[-1] + h * w)
    N = cu[-1]
    g = torch.Generator().manual_seed(21)
    e2, tok = torch.randn(4 * N, 4 * dm, generator=g).to(dt).cuda(), torch.randn(n_obj, dm, generator=g).to(dt).cuda()
    cu_t, w_t = i32(cu), i32([w for _, w in grids])
    ref = torch.full((n_obj, 4 * Hm, 4 * Wm), 7.0, dtype=torch.float64, device="cuda")
    inside = torch.zeros(n_obj, 4 * Hm, 4 * Wm, dtype=torch.bool, device="cuda")
    e = e2.double().view(N, 2, 2, 2, 2, dm)                           # patch, a, b, c, d, k
    for o, (h, w) in enumerate(grids):
        if h == 0:
            continue
        lg = (e[cu[o]: cu[o + 1]] * tok[o].double()).sum(-1)         # → plane[4 row + 2 a + c][4 col + 2 b + d]
        ref[o, : 4 * h, : 4 * w] = lg.view(h, w, 2, 2, 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(4 * h, 4 * w)
        inside[o, : 4 * h, : 4 * w] = True
    fails = Failures()
    tag = f"mask_scatter{'_f32' if dt == F32 else ''} dm={dm}"

    def body(ar):
        E, Tk = ar.inp(e2), ar.inp(tok)
        Mk = ar.out(torch.full((n_obj * 4 * Hm, 4 * Wm), 7.0, device="cuda"), slab=True).view(n_obj, 4 * Hm, 4 * Wm)
        assert E.stride(0) != Tk.stride(0) and E.stride(0) > 4 * dm
        (ops.mask_scatter_f32 if dt == F32 else ops.mask_scatter)(E, Tk, cu_t, w_t, Mk, n_obj, N, dm)
        return {"masks": Mk}

    def check(got):
        m = got["masks"]
        if dt == F32:
            assert rel_err(m[inside], ref[inside]) < 1e-5, f"{tag}: rel err {rel_err(m[inside], ref[inside]):.2e}"
        else:
            close_f32(m[inside], ref[inside].float(), tag, rel=1e-5)
        assert same_bits(m[~inside], torch.full_like(m[~inside], 7.0)), f"{tag}: logits outside the objects' grids changed"
    three(fails, tag, body, check)
    fails.done()


@pytest.mark.parametrize("dm", [8, 260])
def test_mask_scatter_f32_of_upcast_bf16_is_mask_scatter(ops, dm):
    """The two entry points are one kernel over the element type: on the fp32 upcast of bf16 inputs mask_scatter_f32 forms the same fp32
    products and adds them in the same order as mask_scatter on the bf16 inputs, so the planes are equal bit for bit — no tolerance.
    Three objects 1, 2 and 3 patches wide (3 x 1, 1 x 2, 2 x 3) in (3, 3) planes."""
    grids = [(3, 1), (1, 2), (2, 3)]
    n_obj, Hm, Wm = len(grids), 3, 3
    cu = [0]
    for h, w in grids:
        cu.append(cu[-1] + h * w)
    N = cu[-1]
    g = torch.Generator().manual_seed(22)
    e2, tok = torch.randn(4 * N, 4 * dm, generator=g).to(BF).cuda(), torch.randn(n_obj, dm, generator=g).to(BF).cuda()
    cu_t, w_t = i32(cu), i32([w for _, w in grids])
    m16 = ops.mask_scatter(e2, tok, cu_t, w_t, torch.full((n_obj, 4 * Hm, 4 * Wm), 7.0, device="cuda"), n_obj, N, dm)
    m32 = ops.mask_scatter_f32(e2.float(), tok.float(), cu_t, w_t, torch.full((n_obj, 4 * Hm, 4 * Wm), 7.0, device="cuda"), n_obj, N, dm)
    written = m16 != 7.0
    assert int(written.sum()) == 16 * N, "every patch writes its 16 logits (none of which is exactly the fill value)"
    assert same_bits(m32, m16), f"mask_scatter_f32 on upcast inputs differs from mask_scatter in {int((m32 != m16).sum())} logits"


@pytest.mark.parametrize("odt", [F32, BF, F16], ids=["fp32", "bf16", "fp16"])
def test_patchify_normalize_on_windows(ops, odt):
    """Images 28 x 28, 28 x 56 and 56 x 28 (a swap of H and W shows) as byte slabs — 0x7F and then 0 around them —, the table a slab, `out`
    a window of each output type; against oracle.patchify_normalize: fp32 bit-exact, 16-bit = its one rounding."""
    import padt_oracle as O
    from padt_amd import preprocess as P
    lut = torch.from_numpy(P.normalize_lut()).cuda()
    g = torch.Generator().manual_seed(22)
    fails = Failures()
    for H, W in ((28, 28), (28, 56), (56, 28)):
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        rows, gh, gw = O.patchify_normalize(img.numpy())
        ref = torch.from_numpy(np.ascontiguousarray(rows)).to(odt).cuda()
        assert ref.shape == (gh * gw, 1176) and (gh, gw) == (H // 14, W // 14)
        tag = f"patchify_normalize {H}x{W} {odt}"

        def body(ar):
            I = ar.inp(img.view(H, W * 3).cuda(), slab=True).view(H, W, 3)
            out = ar.out(torch.full((gh * gw, 1176), 3.0, dtype=odt, device="cuda"))
            ops.patchify_normalize(I, ar.inp(lut, slab=True), out)
            return {"out": out}

        def check(got):
            assert same_bits(got["out"], ref), f"{tag}: {int((got['out'] != ref).sum())} of {ref.numel()} values differ"
        three(fails, tag, body, check)
    fails.done()
