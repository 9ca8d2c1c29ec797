"""The objects of tests/test_mask_edges_gpu.py's up-sampler cases, built on the CPU (no GPU is needed to import this): logits, sizes and
the reference F.interpolate(..., mode="bilinear") of each object's valid region — so that the one property of the SEEDS the GPU test
relies on (no reference logit within 1e-5 of the threshold: the binary masks must then be equal without exempted pixels) is checked on
the CPU too (tests/test_mask_edges_cpu.py)."""
import torch

HM, WM = 40, 24                                                      # the plane of every object in `masks`
# (src_h, src_w, dst_h, dst_w): 1 x 1 and 4 x 4 sources, a down-sampling, an up-sampling over two x-blocks of 256, widths exactly 256 and 257
MIXED = [(1, 1, 1, 1), (4, 4, 97, 300), (37, 21, 19, 50), (37, 21, 5, 256), (4, 4, 7, 257), (1, 1, 3, 2)]
MIXED_EXTENT = (97, 300)
# one object 2 taller and 3 wider than the launch extents (20, 30), next to one that fits
CROPPED = [(8, 8, 22, 33), (4, 4, 20, 30)]
CROPPED_EXTENT = (20, 30)
SEED = {"mixed": 3, "cropped": 1}                                    # smallest |reference logit|: 4.6e-4 and 7.7e-3
MARGIN = 1e-5


def build(objects, seed):
    """→ masks (n, HM, WM) fp32 with NaN outside each object's valid src_h x src_w region, refs: the up-sampled logits (dst_h, dst_w) per object"""
    g = torch.Generator().manual_seed(seed)
    masks = torch.full((len(objects), HM, WM), float("nan"))
    refs = []
    for o, (hs, ws, h, w) in enumerate(objects):
        masks[o, :hs, :ws] = torch.randn(hs, ws, generator=g) * 3
        refs.append(torch.nn.functional.interpolate(masks[o][None, None, :hs, :ws], size=(h, w), mode="bilinear")[0, 0])
    return masks, refs


def margin(refs):
    """the smallest |logit| of the reference: the binary masks are decided by the sign wherever this is not within rounding of 0"""
    return min(r.abs().min().item() for r in refs)
