"""generate(top_logprobs=k, output_patch_logprobs=True) — host side: the C ABI of the two new entry points, their host validation, the
wrappers and the argument policy."""
import inspect

import pytest

from padt_amd import _lib


def test_new_entry_points_are_declared_with_the_documented_argument_lists():
    decl, twins = _lib.parse_header(), _lib.parse_header(_lib.HEADER_F16)
    assert decl["padt_topk_rows_workspace"][2] == ["n_cols", "k", "batch"]
    assert decl["padt_topk_logprob_rows_f32"][2] == ["stream", "rows_f32", "ld", "n_cols", "k", "unfinished", "step", "t_max", "top_idx", "top_val",
                                                     "vrt_off", "vocab", "patch_lp", "p_cap", "workspace", "batch"]
    assert decl["padt_topk_rows_chunk"][2] == []
    assert not any(name.startswith("padt_topk_") for name in twins)                       # fp32 rows: compiled once, no fp16 twin
    # the existing entry points keep their signatures
    assert decl["padt_vrt_head"][2][-1] == "seen_words" and decl["padt_vrt_head_ban"][2][-1] == "ban_words"
    assert decl["padt_vrt_head_lse"][2][-1] == "part_sum" and decl["padt_greedy_step"][2][-1] == "seen_words"
    assert decl["padt_greedy_step_lp"][2][-2:] == ["part_sum", "logprobs"] and decl["padt_token_logprob_rows_f32"][2][-1] == "batch"
    assert decl["padt_sample_token"][2][-1] == "batch" and decl["padt_argmax_rows_f32"][2][-1] == "batch"


def test_library_exports_the_symbols_and_validates_on_the_host():
    from padt_amd import ops
    lib = _lib.load()
    for name in ("padt_topk_rows_workspace", "padt_topk_logprob_rows_f32", "padt_topk_rows_chunk"):
        assert hasattr(lib, name)
    assert lib.padt_abi_version() == 4
    assert lib.padt_topk_rows_chunk() == ops.TOPK_ROWS_CHUNK
    # host-side validation happens before any launch: no device is needed to be refused.  Fake non-null pointers are never dereferenced.
    P = 4096

    def call(rows=P, ld=100, n_cols=100, k=5, unf=P, step=P, t_max=4, idx=P, val=P, off=0, vocab=0, patch=0, p_cap=0, ws=P, batch=2):
        return lib.padt_topk_logprob_rows_f32(0, rows, ld, n_cols, k, unf, step, t_max, idx, val, off, vocab, patch, p_cap, ws, batch)

    for bad in (dict(k=33), dict(ld=99), dict(rows=0), dict(ws=0), dict(idx=0), dict(k=0, idx=0, val=0), dict(patch=P, p_cap=8), dict(k=-1),
                dict(step=0), dict(n_cols=129 * ops.TOPK_ROWS_CHUNK, ld=129 * ops.TOPK_ROWS_CHUNK)):
        assert call(**bad) == -1 and b"padt_topk_logprob_rows_f32" in lib.padt_last_error(), bad
    assert b"k <= 32" in (call(k=33) and lib.padt_last_error())
    assert call(batch=0) == 0 and call(batch=0, rows=0, k=33) == 0                       # no rows: nothing to do


def test_workspace_size_is_positive_and_monotone():
    from padt_amd import ops
    C = ops.TOPK_ROWS_CHUNK
    w = ops.topk_rows_workspace
    assert w(1, 0, 1) > 0 and w(1, 1, 1) > w(1, 0, 1)
    cols, ks, bs = [1, C - 1, C, C + 1, 3 * C + 1, 152000, 250000], [0, 1, 5, 32], [1, 6, 65]
    for i, n in enumerate(cols):
        for j, k in enumerate(ks):
            for l, b in enumerate(bs):
                v = w(n, k, b)
                assert v > 0 and v % 8 == 0
                assert i == 0 or v >= w(cols[i - 1], k, b)
                assert j == 0 or v > w(n, ks[j - 1], b)
                assert l == 0 or v > w(n, k, bs[l - 1])
    assert w(C + 1, 5, 2) > w(C, 5, 2)                                                   # one more chunk


def test_wrappers_exist_with_the_documented_keywords():
    from padt_amd import ops
    p = inspect.signature(ops.topk_logprob_rows).parameters
    assert list(p)[:6] == ["rows", "n_cols", "unfinished", "step", "workspace", "batch"]
    assert all(p[n].default is None for n in ("top_idx", "top_val", "vrt_off", "patch_lp")) and p["vocab"].default == 0
    assert ops.TOPK_ROWS_MAX_K == 32 and callable(ops.topk_rows_workspace)
    # the wrappers this feature leaves alone keep their last keywords
    assert list(inspect.signature(ops.vrt_head).parameters)[-1] == "part_sum"
    assert list(inspect.signature(ops.greedy_step).parameters)[-2:] == ["part_sum", "logprobs"]


def test_generate_takes_the_two_parameters_and_still_rejects_a_misspelt_one():
    from padt_amd.modeling import PaDTForConditionalGeneration, check_generate_kwargs
    for fn in (PaDTForConditionalGeneration.generate, PaDTForConditionalGeneration.generate_launch):
        p = inspect.signature(fn).parameters
        assert p["top_logprobs"].default is None and p["output_patch_logprobs"].default is False
        assert p["output_token_logprobs"].default is False
    with pytest.raises(ValueError, match="top_logprob"):
        check_generate_kwargs({"top_logprob": 3}, 4, None, 3)
    with pytest.raises(ValueError, match="output_patch_logprob"):
        check_generate_kwargs({"output_patch_logprob": True}, 4, None, 3)


def test_top_logprobs_value_policy():
    import numpy as np
    from padt_amd.modeling import check_top_logprobs
    assert check_top_logprobs(None) == 0 and check_top_logprobs(0) == 0
    assert check_top_logprobs(1) == 1 and check_top_logprobs(32) == 32 and check_top_logprobs(np.int64(7)) == 7
    for bad in (-1, 2.0, "3", True, [3]):
        with pytest.raises(ValueError, match="top_logprobs"):
            check_top_logprobs(bad)
    with pytest.raises(NotImplementedError, match=r"top_logprobs=33.*top_logprobs=32"):
        check_top_logprobs(33)
