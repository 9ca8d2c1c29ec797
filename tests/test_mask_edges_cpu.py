"""What tests/test_mask_edges_gpu.py takes for granted about its own inputs, checked without a GPU: the seeds of the up-sampler objects
leave no reference logit within 1e-5 of the threshold (so the GPU test may demand exactly equal binary masks), the valid regions are
finite and everything else of the planes is NaN, and the oversize object really exceeds the launch extents by less than the windows'
margins."""
import torch

import mask_edge_util as M
from edge_util import MIN_COLS, MIN_ROWS


def test_seeds_leave_no_reference_logit_near_the_threshold():
    for name, objects in (("mixed", M.MIXED), ("cropped", M.CROPPED)):
        masks, refs = M.build(objects, M.SEED[name])
        assert M.margin(refs) >= M.MARGIN, (name, M.margin(refs))
        for o, (hs, ws, h, w) in enumerate(objects):
            assert refs[o].shape == (h, w) and torch.isfinite(refs[o]).all()
            valid = torch.zeros(M.HM, M.WM, dtype=torch.bool)
            valid[:hs, :ws] = True
            assert torch.isfinite(masks[o][valid]).all() and torch.isnan(masks[o][~valid]).all()
        again, _ = M.build(objects, M.SEED[name])
        assert torch.equal(torch.nan_to_num(again), torch.nan_to_num(masks))                   # the same objects on every machine


def test_objects_and_extents():
    mh, mw = M.MIXED_EXTENT
    assert max(o[2] for o in M.MIXED) == mh and max(o[3] for o in M.MIXED) == mw and mw > 256 and {256, 257} <= {o[3] for o in M.MIXED}
    ch, cw = M.CROPPED_EXTENT
    (_, _, h, w), fits = M.CROPPED
    assert (h - ch, w - cw) == (2, 3) and fits[2:] == (ch, cw)
    assert h - ch < MIN_ROWS and w - cw < MIN_COLS                   # an uncropped object would still stay inside the poisoned margins
