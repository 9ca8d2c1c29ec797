"""generate(output_token_logprobs=True) — host side: the C ABI of the three new entry points, the wrappers' keywords and the argument policy."""
import inspect

import pytest

from padt_amd import _lib


def test_new_entry_points_are_declared_with_the_documented_argument_lists():
    decl, twins = _lib.parse_header(), _lib.parse_header(_lib.HEADER_F16)
    ban, lse = decl["padt_vrt_head_ban"], decl["padt_vrt_head_lse"]
    assert lse[2] == ban[2] + ["part_sum"] and lse[1][: len(ban[1])] == ban[1]          # padt_vrt_head_ban's list plus part_sum
    assert twins["padt_vrt_head_lse_f16"][1:] == lse[1:]                                  # both operand twins
    step, lp = decl["padt_greedy_step"], decl["padt_greedy_step_lp"]
    assert lp[2] == step[2] + ["part_sum", "logprobs"] and lp[1][: len(step[1])] == step[1]
    assert "padt_greedy_step_lp_f16" not in twins and "padt_token_logprob_rows_f32_f16" not in twins   # type-independent: compiled once
    assert decl["padt_token_logprob_rows_f32"][2] == ["stream", "rows_f32", "ld", "n_cols", "part_idx", "unfinished", "step", "logprobs", "t_max",
                                                      "batch"]
    # the existing entry points keep their signatures
    assert decl["padt_vrt_head"][2][-1] == "seen_words" and ban[2][-1] == "ban_words" and step[2][-1] == "seen_words"


def test_library_exports_the_new_symbols_and_validates_on_the_host():
    lib = _lib.load()
    for name in ("padt_vrt_head_lse", "padt_vrt_head_lse_f16", "padt_greedy_step_lp", "padt_token_logprob_rows_f32"):
        assert hasattr(lib, name)
    # host-side validation happens before any launch: no device is needed to be refused
    assert lib.padt_token_logprob_rows_f32(0, 0, 8, 8, 0, 0, 0, 0, 4, 2) == -1 and b"padt_token_logprob_rows_f32" in lib.padt_last_error()
    assert lib.padt_token_logprob_rows_f32(0, 0, 8, 8, 0, 0, 0, 0, 4, 0) == 0
    assert lib.padt_greedy_step_lp(*([0] * 3), 1, 2, 8, *([0] * 18)) == -1 and b"part_sum and logprobs" in lib.padt_last_error()
    assert lib.padt_vrt_head_lse(*([0] * 14), 2, 8, *([0] * 8)) == -1 and b"part_sum is required" in lib.padt_last_error()


def test_wrappers_take_the_new_arguments_as_optional_keywords():
    from padt_amd import ops
    head, step = inspect.signature(ops.vrt_head).parameters, inspect.signature(ops.greedy_step).parameters
    assert head["part_sum"].default is None and list(head)[-1] == "part_sum"
    assert step["part_sum"].default is None and step["logprobs"].default is None and list(step)[-2:] == ["part_sum", "logprobs"]
    assert callable(ops.token_logprob_rows)


def test_generate_takes_the_flag_and_still_rejects_a_misspelt_one():
    from padt_amd.modeling import PaDTForConditionalGeneration, check_generate_kwargs
    for fn in (PaDTForConditionalGeneration.generate, PaDTForConditionalGeneration.generate_launch):
        assert inspect.signature(fn).parameters["output_token_logprobs"].default is False
    with pytest.raises(ValueError, match="output_token_logprob"):
        check_generate_kwargs({"output_token_logprob": True}, 4, None, 3)

