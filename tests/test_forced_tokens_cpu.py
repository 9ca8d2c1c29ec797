"""generate(forced_tokens=...) — host side: the table's normal form and its refusals, the options (GenOptions.forced / StepMode.forced), the
entry points that carry the argument, the new C-ABI declarations and ops wrappers, and score_completions' masking.  No GPU, no library call."""
import dataclasses
import inspect

import pytest
import torch

from padt_amd import _lib
from padt_amd.generation import (GenOptions, StepMode, check_forced_tokens, check_generate_kwargs, completion_logprobs, forced_tokens_active,
                                 resolve_options)

INF = float("inf")
V = 100                                                            # text vocabulary of the hand-made cases; the batch has 6 patch rows


# ------------------------------------------------------------------------------------------------------------ the table
def test_tensor_and_ragged_list_give_one_normal_form():
    want = torch.tensor([[3, 104, 7], [5, -1, -1]], dtype=torch.int32)
    for given in (torch.tensor([[3, 104, 7], [5, -1, -1]]), [[3, 104, 7], [5]], torch.tensor([[3, 104, 7], [5, -9, -2]], dtype=torch.int16),
                  [[3, torch.tensor(104), 7], (5, -4)], ((3, 104, 7), [5, -1, -1])):
        got = check_forced_tokens(given, 2, 4, V, [6, 6])
        assert got.dtype == torch.int32 and got.device.type == "cpu" and torch.equal(got, want), given
    assert tuple(check_forced_tokens([[], []], 2, 4, V, [6, 6]).shape) == (2, 0)
    assert torch.equal(check_forced_tokens([[105]], 1, 1, V, [6]), torch.tensor([[105]], dtype=torch.int32))      # the last table row
    assert torch.equal(check_forced_tokens([[10 ** 6]], 1, 1, V), torch.tensor([[10 ** 6]], dtype=torch.int32))   # no bound asked


@pytest.mark.parametrize("given,B,T", [
    ([[1, 2]], 2, 4),                                               # wrong batch size
    (torch.zeros(3, 2, dtype=torch.long), 2, 4),
    ([[1, 2, 3, 4, 5], [1]], 2, 4),                                 # n > max_new_tokens
    (torch.zeros(2, 5, dtype=torch.long), 2, 4),
    (torch.zeros(2, 3), 2, 4),                                      # not an integer dtype
    (torch.zeros(2, 3, dtype=torch.bool), 2, 4),
    ([[1.5], [2]], 2, 4),
    ([[True], [2]], 2, 4),
    ([["a"], [2]], 2, 4),
    (torch.zeros(6, dtype=torch.long), 2, 4),                       # not (B, n)
    (7, 2, 4),
    ([[1, 106], [2]], 2, 4),                                        # one past the table: V + 6 rows
    (torch.tensor([[1, 2], [3, 2 ** 31]]), 2, 4),
])
def test_every_refusal_names_the_argument(given, B, T):
    with pytest.raises(ValueError, match="forced_tokens"):
        check_forced_tokens(given, B, T, V, [6] * B)


def test_an_all_free_table_is_treated_as_absent():
    assert not forced_tokens_active(None)
    assert not forced_tokens_active(check_forced_tokens([[], []], 2, 4, V, [6, 6]))
    assert not forced_tokens_active(check_forced_tokens(torch.full((2, 3), -7), 2, 4, V, [6, 6]))
    assert forced_tokens_active(check_forced_tokens([[-1, -1, 0], []], 2, 4, V, [6, 6]))


# ------------------------------------------------------------------------------------------------------------ options
def test_the_option_defaults_off_and_selects_a_step_mode_of_its_own():
    assert GenOptions().forced is False and StepMode().forced is False
    base = GenOptions(eos_ids=(7,), token_logprobs=True)
    on = dataclasses.replace(base, forced=True)
    assert on.forced is True and base.forced is False
    assert on != base and hash(on) != hash(base) and on == dataclasses.replace(base, forced=True)      # batches merge only when both force or neither
    assert dataclasses.replace(on, keep_scores=True).forced is True                                    # survives a replace of another field
    assert dataclasses.replace(on, forced=False) == base
    assert on.step_mode() == base.step_mode()._replace(forced=True) and on.step_mode() != base.step_mode()
    assert on.step_mode(processors=True).forced and on.step_mode(reference=True).forced
    # the table is per-batch data: a re-run gets it next to the options, not from them
    assert "forced" not in on.generate_kwargs() and "forced_tokens" not in on.generate_kwargs()
    assert on.generate_kwargs() == base.generate_kwargs() and on.warper_kwargs() == base.warper_kwargs()
    assert "forced" not in inspect.signature(resolve_options).parameters


# ------------------------------------------------------------------------------------------------------------ entry points
def test_every_entry_point_takes_the_argument():
    from padt_amd import harness, pipeline
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    p = inspect.signature(M.generate).parameters
    assert "forced_tokens" not in p and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD      # a keyword out of **kwargs, like min_p
    assert "forced_tokens" in inspect.getdoc(M.generate) and "hooks" in inspect.signature(M.generate_launch).parameters
    assert "dict(forced=" in inspect.getdoc(M.generate_launch)
    for fn in (pipeline.rec_batch, pipeline.PipelinedRunner.submit):
        assert inspect.signature(fn).parameters["forced_tokens"].default is None
    sc = list(inspect.signature(M.score_completions).parameters)
    assert sc == ["self", "input_ids", "attention_mask", "pixel_values", "image_grid_thw", "completions", "generate_kwargs"]


def test_infer_dataset_hands_each_batch_its_own_table_to_the_runner(monkeypatch, tmp_path):
    from padt_amd import harness
    seen = []

    class Runner:
        def __init__(self, model, processor, **kw):
            pass

        def submit(self, input_ids, attention_mask, pixel_values, image_grid_thw, **kw):
            seen.append(kw)
            return []

        def flush(self):
            return []

    monkeypatch.setattr(harness, "PipelinedRunner", Runner)
    tables = {0: [[5, 6]], 1: None, 2: torch.tensor([[7]])}

    def prepare(samples):
        b = dict(input_ids=None, attention_mask=None, pixel_values=None, image_grid_thw=None, image_sizes=[(1, 1)], ids=[samples[0]])
        if samples[0] != 1:                                         # a batch without the entry forces nothing
            b["forced_tokens"] = tables[samples[0]]
        return b

    harness.infer_dataset(None, None, [0, 1, 2], prepare, str(tmp_path), batch_size=1)
    assert len(seen) == 3 and all("forced_tokens" in kw for kw in seen)
    assert seen[0]["forced_tokens"] is tables[0] and seen[1]["forced_tokens"] is None and seen[2]["forced_tokens"] is tables[2]


def test_the_bf16_rerun_passes_the_callers_table_on():
    """_non_finite_batch with a stub twin: the re-run's generate() gets the sub record's table, and none when the batch forced nothing"""
    import warnings
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    calls = []

    class Twin:
        def generate(self, **kw):
            calls.append(kw)
            return "out"

    me = object.__new__(M)
    me.operands, me.dtype, me.overflow_reruns, me.prefers_bf16, me._batches_seen, me._fallback = "auto", torch.float16, 0, False, 10, Twin()
    me.precision, me._sd_factory = "default", (lambda: None)
    table = check_forced_tokens([[4, 5], [6]], 2, 4, V)
    for forced in (table, None):
        group = dict(opts=dataclasses.replace(GenOptions(eos_ids=(7,), token_logprobs=True), forced=forced is not None), T_max=4, schedule=None,
                     sync_every=4, use_graph=True, lane=0)
        sub = dict(inputs=(None, None, None, None), input_ids=None, forced=forced)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert me._non_finite_batch(group, sub, True, True, False, False) == "out"
    assert calls[0]["forced_tokens"] is table and calls[0]["output_token_logprobs"] is True and "forced_tokens" not in calls[1]


def test_a_misspelt_keyword_still_raises_and_the_hf_names_stay_rejected():
    with pytest.raises(ValueError, match="forced_token"):
        check_generate_kwargs({"forced_token": [[1]]}, 4, None, 3)
    with pytest.raises(ValueError, match="force_tokens"):
        check_generate_kwargs({"force_tokens": [[1]]}, 4, None, 3)
    for name in ("forced_eos_token_id", "forced_bos_token_id", "sequence_bias", "labels"):
        with pytest.raises(NotImplementedError, match=name):
            check_generate_kwargs({name: 1}, 4, None, 3)
    with pytest.raises(NotImplementedError, match="min_new_tokens"):
        check_generate_kwargs({"min_new_tokens": 2}, 4, None, 3)
    with pytest.raises(ValueError, match="forced_tokens"):          # once popped by generate() it is no stray keyword; left in, it is one
        check_generate_kwargs({"forced_tokens": [[1]]}, 4, None, 3)


def test_new_entry_points_are_declared_with_the_documented_argument_lists():
    decl, twins = _lib.parse_header(), _lib.parse_header(_lib.HEADER_F16)
    assert decl["padt_vrt_head_probe"][2] == decl["padt_vrt_head_lse"][2] + ["forced", "t_forced", "probe_val"]
    assert twins["padt_vrt_head_probe_f16"][:2] == decl["padt_vrt_head_probe"][:2]
    assert decl["padt_forced_step"][2] == decl["padt_greedy_step_lp"][2] + ["forced", "t_forced", "probe_val", "n_cols"]
    assert decl["padt_forced_override"][2] == ["stream", "part_idx", "forced", "t_forced", "step", "unfinished", "n_cols", "batch"]
    assert "padt_forced_step_f16" not in twins and "padt_forced_override_f16" not in twins     # type-independent: compiled once


def test_ops_has_the_new_wrappers_with_the_documented_keywords():
    from padt_amd import ops
    p = list(inspect.signature(ops.vrt_head_probe).parameters)
    assert p[:7] == list(inspect.signature(ops.vrt_head).parameters)[:7] and p[7:11] == ["part_sum", "forced", "probe_val", "step"]
    assert set(p[11:]) == {"mode_table", "logits", "table_packed", "rows", "gen_cfg", "seen", "ban"}
    g = inspect.signature(ops.greedy_step).parameters
    f = inspect.signature(ops.forced_step).parameters
    assert list(f)[:14] == list(g)[:14] and list(f)[14:16] == ["forced", "n_cols"]
    assert all(f[n].default is None for n in ("gen_cfg", "seen", "part_sum", "logprobs", "probe_val")) and f["advance"].default is True
    assert list(inspect.signature(ops.forced_override).parameters) == ["part_idx", "forced", "step", "unfinished", "n_cols", "batch"]
    # the wrappers this feature leaves alone keep their keyword lists
    assert list(inspect.signature(ops.vrt_head).parameters)[-1] == "part_sum" and list(g)[-2:] == ["part_sum", "logprobs"]


# ------------------------------------------------------------------------------------------------------------ score_completions' masking
def test_completion_logprobs_keeps_forced_positions_up_to_the_first_eos():
    EOS, EOS2, PAD = 7, 9, 0
    lp = torch.tensor([[-1.0, -2.0, -4.0, -8.0, -16.0],
                       [-1.0, -2.0, -4.0, 0.0, 0.0],
                       [-1.0, -INF, -4.0, -8.0, -16.0],
                       [-1.0, -2.0, -4.0, -8.0, -16.0]])
    tok = torch.tensor([[11, 12, 13, 14, 15],                       # no EOS: steps 0, 1 and 3 forced, 2 free, 4 past the table
                        [11, 12, EOS2, PAD, PAD],                   # an EOS of the list at step 2 (counts), pads after it
                        [11, 12, 13, EOS, 15],                      # -inf at a forced step; EOS at step 3
                        [EOS, EOS, 12, 13, 14]])                    # EOS right away: only step 0 counts
    forced = check_forced_tokens([[11, 12, -1, 14], [11, 12, EOS2, 13], [11, 12, 13, EOS], [EOS, EOS, 12, 13]], 4, 5, V, [6] * 4)
    per, total = completion_logprobs(lp, tok, forced, [EOS, EOS2])
    assert per.dtype == lp.dtype and tuple(per.shape) == (4, 5) and tuple(total.shape) == (4,)
    assert per.tolist() == [[-1.0, -2.0, 0.0, -8.0, 0.0], [-1.0, -2.0, -4.0, 0.0, 0.0], [-1.0, -INF, -4.0, -8.0, 0.0], [-1.0, 0.0, 0.0, 0.0, 0.0]]
    assert total.tolist() == [-11.0, -7.0, -INF, -1.0] and not torch.isnan(per).any()
    # only the ids of the list end a completion
    per1, total1 = completion_logprobs(lp, tok, forced, [EOS])
    assert per1[1].tolist() == [-1.0, -2.0, -4.0, 0.0, 0.0] and total1[0] == -11.0
    # fewer steps returned than the table is wide (every row finished early): the table is cut, not the log-probs
    per2, total2 = completion_logprobs(lp[:, :2], tok[:, :2], forced, [EOS])
    assert per2.tolist() == [[-1.0, -2.0], [-1.0, -2.0], [-1.0, -INF], [-1.0, 0.0]] and total2.tolist() == [-3.0, -3.0, -INF, -1.0]
