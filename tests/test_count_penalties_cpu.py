"""generate(frequency_penalty=, presence_penalty=, patch_suppression=), host side: the argument checks, the row edit
(generation.count_penalty_row) against vLLM's literal apply_penalties expression bit for bit and in the specified order, count_state on
hand-written token rows, the options (GenOptions / StepMode, dict generation configs, the re-run), the C-ABI declarations and the entry points.
No GPU."""
import dataclasses
import inspect
import math
import warnings

import pytest
import torch

from padt_amd import _lib, ops
from padt_amd.generation import (COUNT_MAX_RADIUS, GenOptions, StepMode, check_count_penalties, check_patch_suppression, count_penalty_row,
                                 count_state, score_bias_row)
from test_score_bias_cpu import EOS, VOCAB, _resolved, _resolving_model

INF = float("inf")
NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_count_penalties_normal_form():
    assert check_count_penalties(None, None, 3) == (None, None)
    assert check_count_penalties(0, 0.0, 3) == (None, None)                    # off: the call without the arguments
    assert check_count_penalties([0, 0, 0], None, 3) == (None, None)
    assert check_count_penalties(2.0, None, 2) == ([2.0, 2.0], [0.0, 0.0])
    assert check_count_penalties(None, [-2, 0.5], 2) == ([0.0, 0.0], [-2.0, 0.5])
    assert check_count_penalties(torch.tensor([0.25, 1.0]), torch.tensor(1.5), 2) == ([0.25, 1.0], [1.5, 1.5])
    f, _ = check_count_penalties(0.1, None, 1)
    assert f == [float(torch.tensor(0.1, dtype=torch.float32))]                # what the device reads


@pytest.mark.parametrize("name", ["frequency_penalty", "presence_penalty"])
@pytest.mark.parametrize("given", [2.5, -2.0001, NAN, INF, -INF, "1", True, [1.0], [1.0, 2.0, 0.0], [1.0, NAN], [0.5, None], [[1.0, 1.0]]],
                         ids=repr)
def test_count_penalties_refusals_name_the_argument(name, given):
    with pytest.raises(ValueError, match=name):
        check_count_penalties(**{name: given, "B": 2, ("presence_penalty" if name == "frequency_penalty" else "frequency_penalty"): None})


def test_patch_suppression_normal_form():
    assert check_patch_suppression(None, 2) is None
    assert check_patch_suppression([None, None], 2) is None                    # nothing suppressed: the call without the argument
    assert check_patch_suppression((1, 2.5), 3) == [(1, 2.5)] * 3
    assert check_patch_suppression((0, INF), 2) == [(0, INF), (0, INF)]      # radius 0, a ban; B == 2 and still ONE pair
    assert check_patch_suppression([1, 2.5], 2) == [(1, 2.5)] * 2             # a dict config spells the pair as a list
    assert check_patch_suppression([None, (COUNT_MAX_RADIUS, 1)], 2) == [None, (7, 1.0)]
    assert check_patch_suppression([(2, 0.5), None, [3, INF]], 3) == [(2, 0.5), None, (3, INF)]


@pytest.mark.parametrize("exc, given, what", [
    (NotImplementedError, (8, 1.0), "at most 7"), (NotImplementedError, [None, (9, INF)], "at most 7.*|row 1"),
    (ValueError, (-1, 1.0), "radius"), (ValueError, [(1.5, 1.0), None], "radius"), (ValueError, [(True, 1.0), None], "radius"),
    (ValueError, (1, 0.0), "penalty"), (ValueError, (1, -3.0), "penalty"), (ValueError, (1, NAN), "penalty"), (ValueError, (1, -INF), "penalty"),
    (ValueError, (1, 1e-60), "penalty"), (ValueError, [(1, 1.0)], "1 entries"), (ValueError, [None, None, (1, 1.0)], "3 entries"),
    (ValueError, 3, "pair"), (ValueError, [(1, 2.0, 3.0), None], "pair"), (ValueError, "ab", "pair")], ids=repr)
def test_patch_suppression_refusals_name_the_argument(exc, given, what):
    with pytest.raises(exc, match="patch_suppression") as e:
        check_patch_suppression(given, 2)
    import re
    assert re.search(what, str(e.value)), str(e.value)


# ------------------------------------------------------------------------------------------------------------ the row edit
def _rows():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 64, generator=g) * 30
    x[0, :8] = torch.tensor([-INF, -0.0, 0.0, 3.0e38, -3.0e38, 1e-40, -1e-40, 1.0])
    x[1, ::3] = -INF
    x[2] = x[2] * 1e30
    x[3, 5] = -0.0
    counts = torch.randint(0, 4, (6, 64), generator=g)
    counts[:, 0:8] = torch.tensor([1024, 0, 0, 1, 1024, 1023, 0, 2])
    counts[3, 5] = 0
    counts[4] = torch.randint(0, 1025, (64,), generator=g)
    counts[5] = 0
    return x.float(), counts


@pytest.mark.parametrize("f, p", [(2.0, 1.0), (-2.0, -2.0), (0.3, 0.0), (0.0, -0.7), (1.1, 1.9), (-0.1, 2.0)])
def test_the_row_edit_is_vllms_apply_penalties_bit_for_bit(f, p):
    x, counts = _rows()
    got = count_penalty_row(x, counts=counts, frequency_penalty=f, presence_penalty=p)
    # vllm/model_executor/layers/utils.py apply_penalties, the two lines after the repetition penalty, literally
    logits = x.clone()
    frequency_penalties = torch.full((x.shape[0],), f, dtype=torch.float32)
    presence_penalties = torch.full((x.shape[0],), p, dtype=torch.float32)
    output_bin_counts = counts
    output_mask = output_bin_counts > 0
    logits -= frequency_penalties.unsqueeze(dim=1) * output_bin_counts
    logits -= presence_penalties.unsqueeze(dim=1) * output_mask
    assert not torch.isnan(got).any() and torch.equal(bits(got), bits(logits))
    assert bool((got[0, 0] == -INF)) and bool((got[1, ::3] == -INF).all())
    # per-row values as (B, 1) tensors: each row is the scalar call
    fr = torch.tensor([[f], [0.0], [f], [-f], [f], [2.0]])
    pr = torch.tensor([[p], [p], [0.0], [p], [-p], [2.0]])
    per = count_penalty_row(x, counts=counts, frequency_penalty=fr, presence_penalty=pr)
    for b in range(6):
        one = count_penalty_row(x[b], counts=counts[b], frequency_penalty=float(fr[b]), presence_penalty=float(pr[b]))
        assert torch.equal(bits(per[b]), bits(one))


def test_the_products_and_differences_round_separately():
    # s - f * c with one rounding (an FMA) differs from the two-step value here: the specification is the two-step one
    g = torch.Generator().manual_seed(11)
    s, f, c = torch.randn(4096, generator=g), 0.1, torch.randint(1, 1025, (4096,), generator=g)
    two = s - torch.tensor(f, dtype=torch.float32) * c.float()
    fma = (s.double() - torch.tensor(f, dtype=torch.float32).double() * c.double()).float()       # the product exact, one rounding
    got = count_penalty_row(s, counts=c, frequency_penalty=f)
    assert torch.equal(bits(got), bits(two))
    assert int((bits(two) != bits(fma)).sum()) > 100, "these values do not tell an FMA from two roundings"


def test_the_order_is_bias_repetition_counts_neighbourhood_bans_decay():
    x = torch.tensor([0.5, -4.0, 2.0, 1.5, 3.0, -1.0, 6.0, 0.25])
    counts = torch.tensor([3, 1, 0, 2, 0, 1, 0, 0])
    near = torch.tensor([0, 0, 0, 0, 0, 2, 1, 0])
    seen = torch.tensor([True, True, False, True, False, False, False, False])
    bias = torch.tensor([1.0, 0, 0, -0.5, 0, 0, 0, 0])
    banned = torch.tensor([False, False, False, False, True, False, False, False])
    kw = dict(counts=counts, frequency_penalty=0.5, presence_penalty=0.25, near=near, suppression_penalty=1.5, bias=bias, penalty=1.3, seen=seen,
              banned=banned, eos_ids=(7, 3), a_t=0.5)
    got = count_penalty_row(x, **kw)
    # by hand, one fp32 operation at a time
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    pen = f32(1.3)
    exp = []
    for c in range(8):
        s = f32(float(x[c])) + bias[c]
        if seen[c]:
            s = s * pen if s < 0 else s / pen
        s = s - f32(0.5) * counts[c].float()
        s = s - f32(0.25) * (counts[c] > 0).float()
        if near[c] > 0:
            s = s - near[c].float() * f32(1.5)
        if banned[c]:
            s = f32(-INF)
        if c in (7, 3) and s != -INF:
            s = s + s.abs() * f32(0.5)
        exp.append(s)
    assert torch.equal(bits(got), bits(torch.stack(exp)))
    # swapping the repetition penalty and the count edit changes bits: column 0 (seen, counted) tells the two orders apart
    swapped = score_bias_row(count_penalty_row(score_bias_row(x, bias=bias), counts=counts, frequency_penalty=0.5, presence_penalty=0.25),
                             penalty=1.3, seen=seen)
    ordered = count_penalty_row(x, counts=counts, frequency_penalty=0.5, presence_penalty=0.25, bias=bias, penalty=1.3, seen=seen)
    assert bits(swapped)[0] != bits(ordered)[0] and bits(ordered)[0] == bits(got)[0]
    assert float(ordered[0]) == float((f32(0.5) + 1.0) / pen - f32(0.5) * 3 - f32(0.25))


def test_suppression_bans_with_inf_and_leaves_the_rest_alone():
    x = torch.tensor([1.0, -INF, -0.0, 5.0, 2.0])
    near = torch.tensor([0, 3, 0, 1, 65535])
    got = count_penalty_row(x, near=near, suppression_penalty=INF)
    assert not torch.isnan(got).any()                                         # near == 0 is no operation: no 0 * inf
    assert torch.equal(bits(got), bits(torch.tensor([1.0, -INF, -0.0, -INF, -INF])))
    soft = count_penalty_row(x, near=near, suppression_penalty=0.5)
    assert torch.equal(bits(soft), bits(torch.tensor([1.0, -INF, -0.0, 4.5, 2.0 - 65535 * 0.5])))
    off = count_penalty_row(x, near=near, suppression_penalty=0.0)            # a row without suppression in a batch that has it
    assert torch.equal(bits(off), bits(x))
    rows = count_penalty_row(x.expand(2, 5), near=near.expand(2, 5), suppression_penalty=torch.tensor([[0.0], [INF]]))
    assert torch.equal(bits(rows[0]), bits(x)) and torch.equal(bits(rows[1]), bits(got))


# ------------------------------------------------------------------------------------------------------------ count_state by hand
V = 100           # text ids 0 .. 99; the row owns patches lo .. hi - 1, VRT ids V + lo ..


def vrt(j, lo=0):
    return V + lo + j


def test_count_state_counts_generated_tokens():
    toks = [5, 5, vrt(2), 7, 5, vrt(2), vrt(0), 99]
    count, near = count_state(toks, len(toks), V, 0, 6)
    assert count == {5: 3, 7: 1, 99: 1, vrt(2): 2, vrt(0): 1} and near == [0] * 6       # no radius: nothing suppressed
    assert count_state(toks, 2, V, 0, 6)[0] == {5: 2}                           # after n tokens; what lies behind n (a finished row's pads) is not counted
    assert count_state(toks, 0, V, 0, 6) == ({}, [0] * 6)
    # forced tokens are emitted tokens: the walk cannot tell them apart, and must not
    assert count_state([vrt(1), 7], 2, V, 0, 6)[0] == {vrt(1): 1, 7: 1}
    # a VRT id outside the row's own range counts nowhere
    assert count_state([vrt(0), vrt(9), 3], 3, V, 4, 8)[0] == {3: 1}


def test_count_state_an_open_run_suppresses_nothing_a_closed_one_does():
    grid = (3, 5)
    open_run = [7, vrt(7), vrt(8)]
    assert count_state(open_run, 3, V, 0, 15, grid, 1)[1] == [0] * 15
    closed = open_run + [4]                                                     # closed by a text id
    near = count_state(closed, 4, V, 0, 15, grid, 1)[1]
    #  patches 7 = (1, 2) and 8 = (1, 3), radius 1: rows 0-2, columns 1-3 and 2-4; the overlap (columns 2-3) counts both tokens
    assert near == [0, 1, 2, 2, 1] * 3
    assert count_state(open_run + [EOS], 4, V, 0, 15, grid, 1)[1] == near     # closed by EOS: any non-VRT id closes a run
    assert count_state(closed, 3, V, 0, 15, grid, 1)[1] == [0] * 15             # ... but not before it was generated
    # two runs over the same patch: near == 2 there
    two = [vrt(0), 1, vrt(0), 2]
    assert count_state(two, 4, V, 0, 15, grid, 0)[1] == [2] + [0] * 14
    assert count_state(two, 3, V, 0, 15, grid, 0)[1] == [1] + [0] * 14         # the second run is still open
    # a run interrupted by a foreign VRT id is still ONE run (a VRT token), and the foreign token adds nothing
    assert count_state([vrt(0), vrt(40), vrt(1), 3], 4, V, 0, 15, grid, 0)[1] == [1, 1] + [0] * 13


def test_count_state_windows_on_a_3x5_grid():
    grid = (3, 5)
    win = lambda j, r: count_state([vrt(j), 1], 2, V, 0, 15, grid, r)[1]
    assert win(0, 1) == [1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]           # corner: clipped to 2 x 2
    assert win(2, 1) == [0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0]           # top edge: 2 x 3
    assert win(7, 1) == [0, 1, 1, 1, 0] * 3                                    # centre: the full 3 x 3
    assert win(14, 1) == [0] * 8 + [1, 1, 0, 0, 0, 1, 1]                        # the far corner
    assert win(9, 0) == [0] * 9 + [1] + [0] * 5                                 # radius 0: the patch itself
    assert win(4, 7) == [1] * 15                                                # a radius larger than the grid: all of it, once
    assert win(7, 2) == [1] * 15
    # the row's own offset: patches lo .. hi - 1 of a shared table
    assert count_state([vrt(0, lo=4), 1], 2, V, 4, 10, (2, 3), 1)[1] == [1, 1, 0, 1, 1, 0]
    with pytest.raises(ValueError, match="grid"):
        count_state([1], 1, V, 0, 15, (3, 4), 1)


# ------------------------------------------------------------------------------------------------------------ options
def test_the_options_carry_only_whether_each_mechanism_is_on():
    base = GenOptions(eos_ids=(EOS,))
    assert not base.counts and base.step_mode() == StepMode() and StepMode().counts is False
    c = dataclasses.replace(base, count_penalties=True)
    s = dataclasses.replace(base, patch_suppression=True)
    both = dataclasses.replace(c, patch_suppression=True)
    assert c.counts and s.counts and both.counts
    assert c.step_mode() == s.step_mode() == both.step_mode() == StepMode(counts=True)
    assert len({base, c, s, both}) == 4 and c != base and c == dataclasses.replace(base, count_penalties=True)
    assert "count_penalties=True" in repr(c) and "patch_suppression=True" in repr(s)
    withbias = dataclasses.replace(c, logit_bias=((3, 1.0),))
    assert withbias.step_mode() == StepMode(counts=True, bias=True)


def test_generate_resolves_the_three_arguments():
    m = _resolving_model()
    plain, kw0 = _resolved(m)
    off, kw1 = _resolved(m, frequency_penalty=None, presence_penalty=0.0, patch_suppression=[None, None])
    assert plain == off == GenOptions(eos_ids=(EOS,)) and off.step_mode() == StepMode()          # off: the parent's options and step mode
    assert kw0["counts"] is None and kw1["counts"] is None and kw1["hooks"] is None
    on, kw = _resolved(m, frequency_penalty=2.0, presence_penalty=[1.0, 0.5])
    assert on.count_penalties and not on.patch_suppression and on.step_mode() == StepMode(counts=True)
    assert kw["counts"] == dict(frequency_penalty=[2.0, 2.0], presence_penalty=[1.0, 0.5], patch_suppression=None) and kw["hooks"] is None
    sup, kws = _resolved(m, patch_suppression=(1, INF))
    assert sup.patch_suppression and not sup.count_penalties and kws["counts"]["patch_suppression"] == [(1, INF), (1, INF)]
    assert kws["counts"]["frequency_penalty"] is None
    # the values are per-batch data: batches with different values share a decode group, a batch with and one without do not
    assert _resolved(m, frequency_penalty=0.5)[0] == _resolved(m, presence_penalty=[1.0, -1.0])[0] == on
    assert _resolved(m, patch_suppression=[None, (3, 0.5)])[0] == sup and sup != on and on != plain
    # the dict form of generation_config=, read the way top_logprobs is; an explicit argument wins
    cfg_on, kwc = _resolved(m, generation_config=dict(frequency_penalty=1.5, patch_suppression=[2, 4.0]))
    assert cfg_on.count_penalties and cfg_on.patch_suppression
    assert kwc["counts"] == dict(frequency_penalty=[1.5, 1.5], presence_penalty=[0.0, 0.0], patch_suppression=[(2, 4.0), (2, 4.0)])
    assert _resolved(m, generation_config=dict(frequency_penalty=1.5), frequency_penalty=0.25)[1]["counts"]["frequency_penalty"] == [0.25, 0.25]
    # the re-run: the options' keywords plus the batch's own values resolve back to the same call
    again, kwa = _resolved(m, **on.generate_kwargs(), **on.warper_kwargs(), **on.bias_kwargs(), **on.stop_kwargs(), **kw["counts"])
    assert again == on and kwa["counts"] == kw["counts"]
    mixed, _ = _resolved(m, frequency_penalty=1.0, logit_bias={5: 1.0}, stop_sequences=[[3]], no_repeat_ngram_size=2, forced_tokens=[[5], [6]])
    assert mixed.counts and mixed.score_bias and mixed.stop and mixed.rules is not None and mixed.forced
    for exc, name, kwargs in ((ValueError, "frequency_penalty", dict(frequency_penalty=2.5)),
                              (ValueError, "frequency_penalty", dict(frequency_penalty=NAN)),
                              (ValueError, "presence_penalty.*3 entries", dict(presence_penalty=[1.0, 1.0, 1.0])),
                              (ValueError, "presence_penalty", dict(generation_config=dict(presence_penalty=-3))),
                              (NotImplementedError, "patch_suppression.*at most 7", dict(patch_suppression=(8, 1.0))),
                              (ValueError, "patch_suppression.*radius", dict(patch_suppression=(-1, 1.0))),
                              (ValueError, "patch_suppression.*penalty", dict(patch_suppression=(1, 0.0))),
                              (ValueError, "patch_suppression.*penalty", dict(patch_suppression=[None, (1, NAN)])),
                              (NotImplementedError, "output_logits", dict(frequency_penalty=1.0, output_logits=True)),
                              (NotImplementedError, "sequence_bias", dict(sequence_bias={(1,): 1.0})),
                              (NotImplementedError, "min_new_tokens", dict(min_new_tokens=2))):
        with pytest.raises(exc, match=name):
            m.generate(input_ids=torch.zeros(2, 3, dtype=torch.long), attention_mask=None, pixel_values=None, image_grid_thw=None,
                       max_new_tokens=8, **kwargs)


def test_the_bf16_rerun_carries_the_batchs_values():
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    calls = []

    class Twin:
        def generate(self, **kw):
            calls.append(kw)
            return "out"

    me = object.__new__(M)
    me.operands, me.dtype, me.overflow_reruns, me.prefers_bf16, me._batches_seen, me._fallback = "auto", torch.float16, 0, False, 10, Twin()
    me.precision, me._sd_factory = "default", (lambda: None)
    base = GenOptions(eos_ids=(EOS,))
    on = dataclasses.replace(base, count_penalties=True, patch_suppression=True)
    vals = dict(frequency_penalty=[2.0, 0.0], presence_penalty=[1.0, 1.0], patch_suppression=[None, (1, INF)])
    for opts, counts in ((on, vals), (base, None)):
        group = dict(opts=opts, T_max=8, schedule=None, sync_every=4, use_graph=True, lane=0)
        sub = dict(inputs=(None, None, None, None), input_ids=None, forced=None, automaton=None, patch_bias=None, stop=None, counts=counts)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert me._non_finite_batch(group, sub, True, True, False, False) == "out"
    assert {k: calls[0][k] for k in vals} == vals
    assert not any(k in calls[1] for k in vals)                                # without them: the call the parent made


def test_the_keywords_reach_every_entry_point():
    from padt_amd import harness, pipeline
    for fn in (pipeline.rec_batch, pipeline.PipelinedRunner.submit, harness.infer_dataset):
        assert {"frequency_penalty", "presence_penalty", "patch_suppression"} <= set(inspect.signature(fn).parameters), fn
    m = _resolving_model()
    with pytest.raises(Exception) as e:                                        # score_completions hands **generate_kwargs to generate()
        m.score_completions(torch.zeros(2, 3, dtype=torch.long), None, None, None, [[5], [6]], frequency_penalty=1.0)
    assert e.value.args[0].count_penalties and e.value.args[0].forced


def test_the_entry_points_are_declared_with_the_documented_argument_lists():
    decl = {**_lib.parse_header(), **_lib.parse_header(_lib.HEADER_F16)}
    bias = decl["padt_vrt_head_bias"]
    for name in ("padt_vrt_head_counts", "padt_vrt_head_counts_f16"):
        _, argtypes, argnames = decl[name]
        assert argnames[: len(bias[2])] == bias[2] and argnames[len(bias[2]):] == ["cnt_text", "ld_cnt", "cnt_patch", "near", "cpen"]
    assert decl["padt_count_update"][2] == ["stream", "tokens", "ld_tokens", "step", "unfinished", "vrt_off", "grid", "radius", "cnt_text",
                                            "ld_cnt", "vocab", "cnt_patch", "near", "n_proto", "batch"]
    assert "padt_count_update_f16" not in decl                                # type-independent: compiled once
    assert ops.COUNT_MAX_RADIUS == COUNT_MAX_RADIUS == 7 and (2 * ops.COUNT_MAX_RADIUS + 1) ** 2 <= 256
    t = torch.tensor([0, 1, -1, -32768], dtype=ops.COUNT_DTYPE)
    assert ops.count_values(t).tolist() == [0, 1, ops.COUNT_SAT, 32768]
