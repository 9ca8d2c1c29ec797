"""generate(logit_bias=, patch_bias=, exponential_decay_length_penalty=), host side: the normal forms and refusals of the three arguments, the
decay table and the plain statement of the specification (generation.score_bias_row) against the installed HF processors bit for bit, the
options (GenOptions / StepMode, generation configs, the re-run keywords), the C-ABI declaration with its wrapper, and the entry points.
No GPU."""
import dataclasses
import inspect
import math
import warnings
from types import SimpleNamespace

import pytest
import torch

from padt_amd import _lib, ops
from padt_amd.generation import (DECAY_OFF, GenOptions, StepMode, check_decay_length_penalty, check_generate_kwargs, check_logit_bias,
                                 check_patch_bias, decay_table, resolve_options, score_bias_row)

INF = float("inf")
EOS, VOCAB = 7, 1000


def hf_defaults(**kw):
    return SimpleNamespace(repetition_penalty=1.0, eos_token_id=[EOS], pad_token_id=0, do_sample=False, temperature=1.0, top_k=50, top_p=1.0,
                           no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, **kw)


def same_bits(a, b):
    """equal fp32 values, -inf in the same places, no NaN (a zero's sign aside: HF adds a zero tensor to the columns it leaves alone)"""
    return a.dtype == b.dtype == torch.float32 and not bool(torch.isnan(a).any()) and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ logit_bias
def test_logit_bias_normal_form():
    key = check_logit_bias({5: 1.5, 3: -2, 9: -INF, 11: 0.0}, VOCAB)
    assert key == ((3, -2.0), (5, 1.5), (9, -INF)) and all(isinstance(v, float) for _, v in key)
    assert check_logit_bias([[9, -INF], (5, 1.5), [3, -2]], VOCAB) == key == check_logit_bias({"5": 1.5, "3": -2.0, "9": -INF}, VOCAB)
    assert check_logit_bias({3: torch.tensor(-2.0), torch.tensor(5): 1.5, 9: -INF}, VOCAB) == key
    assert hash(check_logit_bias([[3, -2], [5, 1.5], [9, -INF]], VOCAB)) == hash(key)
    assert check_logit_bias({4: 0.1}, VOCAB) == ((4, float(torch.tensor(0.1, dtype=torch.float32))),)      # what the device adds
    for off in (None, {}, [], {4: 0.0}):
        assert check_logit_bias(off, VOCAB) is None
    assert check_logit_bias({VOCAB - 1: 1.0, 0: 1.0}, VOCAB) == ((0, 1.0), (VOCAB - 1, 1.0))


@pytest.mark.parametrize("exc,given", [
    (ValueError, {3: float("nan")}), (ValueError, {3: INF}), (ValueError, {3: 1e39}), (ValueError, {3: "x"}), (ValueError, {3: True}),
    (ValueError, {-1: 1.0}), (ValueError, {2.5: 1.0}), (ValueError, {True: 1.0}), (ValueError, [[3, 1.0], [3, 2.0]]), (ValueError, [[3, 1.0, 2.0]]),
    (ValueError, 5), (ValueError, [3]), (NotImplementedError, {VOCAB: 1.0}), (NotImplementedError, [[VOCAB + 40, -INF]]),
])
def test_logit_bias_refusals_name_the_argument(exc, given):
    with pytest.raises(exc, match="logit_bias"):
        check_logit_bias(given, VOCAB)


def test_a_vrt_id_points_to_patch_bias():
    with pytest.raises(NotImplementedError, match="patch_bias"):
        check_logit_bias({VOCAB + 3: 1.0}, VOCAB)


# ------------------------------------------------------------------------------------------------------------ patch_bias
def test_patch_bias_normal_form():
    m = torch.arange(12.0).reshape(3, 4)
    out = check_patch_bias([None, m, [0.5, -INF, 2]], 3)
    assert out[0] is None and torch.equal(out[1], m) and out[1].dtype == torch.float32 and out[1].is_contiguous()      # a map keeps its shape until the grid is known
    assert torch.equal(out[2], torch.tensor([0.5, -INF, 2.0]))
    out = check_patch_bias([None, m.to(torch.float16), torch.tensor([1, 2, 3])], 3, patches=[5, 12, 3], grids=[(1, 5), (3, 4), (1, 3)])
    assert torch.equal(out[1], torch.arange(12.0)) and torch.equal(out[2], torch.tensor([1.0, 2.0, 3.0]))
    assert torch.equal(check_patch_bias([m.t()], 1, patches=[12], grids=[(4, 3)])[0], m.t().reshape(-1))     # row-major over the map: VRT-id order
    for off in (None, [None, None]):
        assert check_patch_bias(off, 2) is None
    again = check_patch_bias(check_patch_bias([None, m], 2), 2, patches=[7, 12], grids=[(1, 7), (3, 4)])      # the normal form is a legal argument
    assert again[0] is None and torch.equal(again[1], torch.arange(12.0))


@pytest.mark.parametrize("given,B,kw,what", [
    ([None], 2, {}, "1 entries for a batch of 2"),
    (torch.zeros(2, 5), 2, {}, "list"),
    (5, 1, {}, "list"),
    ([None, torch.zeros(5)], 2, dict(patches=[5, 12]), "row 1.*5 values for 12"),
    ([torch.zeros(4, 3), None], 2, dict(patches=[12, 5], grids=[(3, 4), (1, 5)]), "row 0.*map"),
    ([None, torch.tensor([1.0, float("nan")])], 2, {}, "row 1.*NaN"),
    ([torch.tensor([INF, 0.0]), None], 2, {}, r"row 0.*\+inf"),
    ([torch.tensor([1e39], dtype=torch.float64)], 1, {}, "row 0.*fp32"),
    ([torch.zeros(2, 2, 2)], 1, {}, "row 0"),
    ([torch.tensor([True, False])], 1, {}, "row 0"),
    (["ab"], 1, {}, "row 0"),
])
def test_patch_bias_refusals_name_the_argument_and_the_row(given, B, kw, what):
    with pytest.raises(ValueError, match="patch_bias.*" + what):
        check_patch_bias(given, B, **kw)


# ------------------------------------------------------------------------------------------------------------ the decay
def test_decay_normal_form_and_refusals():
    assert check_decay_length_penalty((3, 1.5), 16) == (3, 1.5) == check_decay_length_penalty([3, 1.5], 16)
    assert check_decay_length_penalty((0, 2), 16) == (0, 2.0) and isinstance(check_decay_length_penalty((0, 2), 16)[1], float)
    assert check_decay_length_penalty(None, 16) is None
    assert check_decay_length_penalty((5, 0.5), 4096) == (5, 0.5)                                 # a factor below 1 never overflows
    assert check_decay_length_penalty((0, 2.0), 127) == (0, 2.0)
    for bad in ((-1, 1.5), (1.5, 1.5), (True, 1.5), (3, 0.0), (3, -1.0), (3, INF), (3, float("nan")), (3, "x"), (3,), 3, (3, 1.5, 2), (3, True)):
        with pytest.raises(ValueError, match="exponential_decay_length_penalty"):
            check_decay_length_penalty(bad, 16)
    for start, factor, n in ((0, 2.0, 128), (100, 2.0, 128), (0, 1.1, 1024), (0, 1e30, 2)):     # factor ** max_new_tokens: the bound the issue sets
        with pytest.raises(ValueError, match="exponential_decay_length_penalty.*fp32"):
            check_decay_length_penalty((start, factor), n)


def test_decay_table_entries():
    a = decay_table((3, 1.5), 8)
    assert a.dtype == torch.float32 and a.shape == (8,) and torch.equal(a[:4], torch.zeros(4))
    assert a.tolist()[4:] == [float(torch.tensor(1.5 ** k - 1, dtype=torch.float64).to(torch.float32)) for k in (1, 2, 3, 4)]
    assert torch.equal(decay_table(None, 5), torch.zeros(5)) and torch.equal(decay_table(DECAY_OFF, 5), torch.zeros(5))
    assert decay_table((0, 0.9), 3).tolist() == [0.0] + [float(torch.tensor(0.9 ** k - 1).to(torch.float32)) for k in (1, 2)]
    assert bool(torch.isfinite(decay_table((0, 2.0), 128)).all())


def test_decay_table_longer_than_the_validated_call():
    """a session's table may be longer than the call that was validated: the powers past max_new_tokens need not fit a double"""
    assert check_decay_length_penalty((0, 4.0), 60) == (0, 4.0)
    a = decay_table((0, 4.0), 1024, 60)                                                   # what DecodeSession.begin builds
    assert a.shape == (1024,) and bool(torch.isfinite(a).all()) and torch.equal(a[60:], torch.zeros(964)) and float(a[0]) == 0.0
    assert a[1:60].tolist() == [float(torch.tensor(4.0 ** k - 1, dtype=torch.float64).to(torch.float32)) for k in range(1, 60)]
    assert torch.equal(decay_table((0, 4.0), 60), a[:60]) and torch.equal(decay_table((0, 4.0), 40, 60), a[:40])
    whole = decay_table((0, 4.0), 1024)                                                   # no bound given: +inf past the double range, no exception
    assert torch.equal(whole[:60], a[:60]) and bool((whole[600:] == INF).all()) and not bool(torch.isnan(whole).any())
    assert torch.equal(decay_table((3, 0.5), 2000, 5)[5:], torch.zeros(1995)) and torch.equal(decay_table((3, 1.5), 8, 0), torch.zeros(8))


@pytest.mark.parametrize("start", [0, 3])
@pytest.mark.parametrize("factor", [1.3, 0.8])
def test_decay_table_is_hfs_processor_bit_for_bit(start, factor):
    from transformers.generation.logits_process import ExponentialDecayLengthPenalty
    L, n, T, eos = 5, 40, 9, (7, 21)
    g = torch.Generator().manual_seed(start * 10 + int(factor * 10))
    hf = ExponentialDecayLengthPenalty((start, factor), list(eos), L)
    table = decay_table((start, factor), T)
    changed = 0
    for t in range(T):                                            # t tokens generated so far: both sides of `start`
        rows = torch.randn(4, n, generator=g) * 6
        want = hf(torch.zeros(4, L + t, dtype=torch.long), rows.clone())
        got = score_bias_row(rows, eos_ids=eos, a_t=table[t])
        assert same_bits(got, want), t
        if t <= start:
            assert torch.equal(got, rows), t
        changed += int(not torch.equal(got, rows))
    assert changed == T - 1 - start


def test_the_specification_is_hfs_chain_in_hfs_order_bit_for_bit():
    """SequenceBias (1-token sequences) → RepetitionPenalty → ExponentialDecayLengthPenalty on random fp32 rows with -inf entries"""
    from transformers.generation.logits_process import (ExponentialDecayLengthPenalty, RepetitionPenaltyLogitsProcessor,
                                                        SequenceBiasLogitsProcessor)
    L, n, rows, eos, pen = 6, 64, 5, (7, 21), 1.3
    g = torch.Generator().manual_seed(11)
    key = check_logit_bias({3: 2.5, 7: -1.25, 9: -INF, 30: 0.3, 40: -7.0, 63: 4.0}, n)
    bias = torch.zeros(n)
    for k, v in key:
        bias[k] = v
    for start, factor in ((0, 1.3), (3, 0.8)):
        table = decay_table((start, factor), 8)
        for t in range(8):
            logits = torch.randn(rows, n, generator=g) * 5
            masked = torch.rand(rows, n, generator=g) < 0.2                               # the logit mask: -inf before any processor
            masked[:, list(eos)] = False                                                   # HF turns a -inf EOS column into NaN: its own test below
            logits[masked] = -INF
            ids = torch.randint(0, n, (rows, L + t), generator=g)
            seen = torch.zeros(rows, n, dtype=torch.bool).scatter_(1, ids, True)
            want = logits.clone()
            for proc in (SequenceBiasLogitsProcessor({(k,): v for k, v in key}), RepetitionPenaltyLogitsProcessor(pen),
                         ExponentialDecayLengthPenalty((start, factor), list(eos), L)):
                want = proc(ids, want)
            got = score_bias_row(logits, bias=bias, penalty=pen, seen=seen, eos_ids=eos, a_t=table[t])
            assert same_bits(got, want), (start, t)
            assert bool((got[:, 9] == -INF).all()) and bool((got[masked] == -INF).all())
    # the order matters: the penalty of a biased seen column is taken on the biased value
    x = torch.tensor([[1.0, -1.0]])
    got = score_bias_row(x, bias=torch.tensor([-3.0, 3.0]), penalty=2.0, seen=torch.ones(1, 2, dtype=torch.bool))
    assert got.tolist() == [[-4.0, 1.0]]


def test_the_deviation_a_banned_eos_column_stays_minus_inf():
    from transformers.generation.logits_process import ExponentialDecayLengthPenalty
    rows = torch.tensor([[1.0, -INF, 2.0, -3.0]])
    hf = ExponentialDecayLengthPenalty((0, 1.5), [1, 3], 2)(torch.zeros(1, 4, dtype=torch.long), rows.clone())
    assert math.isnan(float(hf[0, 1]))                                                     # what HF does there
    got = score_bias_row(rows, eos_ids=(1, 3), a_t=decay_table((0, 1.5), 4)[2])
    assert got.tolist() == [[1.0, -INF, 2.0, -3.0 + 3.0 * 1.25]]
    banned = torch.tensor([[False, False, False, True]])
    assert score_bias_row(rows, banned=banned, eos_ids=(3,), a_t=1.0).tolist() == [[1.0, -INF, 2.0, -INF]]      # the bans come before the decay
    assert score_bias_row(rows, bias=torch.tensor([0.0, 5.0, -INF, 0.0])).tolist() == [[1.0, -INF, -INF, -3.0]]  # -inf + bias, bias -inf: bans


# ------------------------------------------------------------------------------------------------------------ options, step mode, configs
def test_the_options_are_part_of_equality_hash_and_repr_and_select_one_step_mode():
    base = resolve_options(hf_defaults(), EOS, VOCAB)
    assert base.logit_bias is None and base.decay is None and base.patch_bias is False and not base.score_bias
    assert base == GenOptions(eos_ids=(EOS,)) and StepMode().bias is False and base.step_mode() == StepMode()
    lb1, lb2 = check_logit_bias({3: 1.0}, VOCAB), check_logit_bias({3: 2.0}, VOCAB)
    a, a2, b = (dataclasses.replace(base, logit_bias=x) for x in (lb1, check_logit_bias([[3, 1.0]], VOCAB), lb2))
    assert a != base and a == a2 and hash(a) == hash(a2) and a != b and repr(a) != repr(base) and repr(a) != repr(b)
    p = dataclasses.replace(base, patch_bias=True)                                        # a patch_bias on one batch only
    assert p != base and p != a and hash(p) != hash(base) and dataclasses.replace(p, patch_bias=False) == base
    d1, d2 = dataclasses.replace(base, decay=(3, 1.5)), dataclasses.replace(base, decay=(3, 1.6))
    assert d1 != base and d1 != d2 and d1 == dataclasses.replace(base, decay=[3, 1.5]) and dataclasses.replace(d1, decay=None) == base
    assert dataclasses.replace(a, keep_scores=True).logit_bias == lb1 and dataclasses.replace(d1, forced=True).decay == (3, 1.5)
    assert dataclasses.replace(p, automaton=None).patch_bias and dataclasses.replace(dataclasses.replace(a, forced=True), decay=(1, 2.0)).forced
    names = {f.name for f in dataclasses.fields(GenOptions)}
    assert not names & {"logit_bias", "decay", "patch_bias"} and not set(a.generate_kwargs()) & {"logit_bias", "exponential_decay_length_penalty"}
    # values that share a graph: one step mode for every bias / decay / patch prior, another than without
    on = base.step_mode()._replace(bias=True)
    assert a.step_mode() == b.step_mode() == p.step_mode() == d1.step_mode() == d2.step_mode() == on != base.step_mode()
    assert dataclasses.replace(a, decay=(3, 1.5), patch_bias=True).step_mode() == on
    assert a.step_mode(processors=True).bias and a.step_mode(reference=True).bias
    big = dataclasses.replace(base, logit_bias=tuple((i, 1.0) for i in range(500)))
    assert len(repr(big)) < 1000


class _Launched(Exception):
    pass


def _resolving_model(**gc):
    from padt_amd.modeling import PaDTForConditionalGeneration as M

    class Probe(M):
        def _launch(self, opts, *a, **kw):
            raise _Launched(opts, kw)
    m = object.__new__(Probe)
    m.generation_config = hf_defaults(**gc)
    m.config = SimpleNamespace(eos_token_id=EOS, vocab_size=VOCAB)
    m.prefers_bf16, m.precision = False, "default"
    return m


def _resolved(m, **kw):
    with pytest.raises(_Launched) as e:
        m.generate(input_ids=torch.zeros(2, 3, dtype=torch.long), attention_mask=None, pixel_values=None, image_grid_thw=None,
                   **dict(dict(max_new_tokens=8), **kw))
    return e.value.args


def test_generate_resolves_the_three_arguments():
    m = _resolving_model()
    plain, kw0 = _resolved(m)
    off, kw1 = _resolved(m, logit_bias=None, patch_bias=None, exponential_decay_length_penalty=None)
    off2, kw2 = _resolved(m, logit_bias={}, patch_bias=[None, None], exponential_decay_length_penalty=DECAY_OFF)
    assert plain == off == off2 == GenOptions(eos_ids=(EOS,)) and plain.step_mode() == StepMode()      # off: the call without them
    assert kw0["patch_bias"] is None and kw1["patch_bias"] is None and kw2["patch_bias"] is None and kw2["hooks"] is None
    on, kw = _resolved(m, logit_bias={5: 1.0, 3: -INF}, patch_bias=[None, torch.ones(4)], exponential_decay_length_penalty=(2, 1.5))
    assert on.logit_bias == ((3, -INF), (5, 1.0)) and on.decay == (2, 1.5) and on.patch_bias and on.step_mode() == StepMode(bias=True)
    assert kw["patch_bias"][0] is None and torch.equal(kw["patch_bias"][1], torch.ones(4)) and kw["hooks"] is None
    assert _resolved(m, logit_bias=[[5, 1.0]])[0] != _resolved(m, logit_bias=[[5, 2.0]])[0]
    assert _resolved(m, patch_bias=[torch.ones(4), None])[0] == _resolved(m, patch_bias=[None, torch.zeros(9)])[0] != plain
    both, kwb = _resolved(m, logit_bias={5: 1.0}, forced_tokens=[[5], [6]], no_repeat_ngram_size=2, output_token_logprobs=True)
    assert both.logit_bias and both.forced and both.rules is not None and both.token_logprobs and kwb["forced"] is not None
    for exc, name, kwargs in ((NotImplementedError, "logit_bias.*patch_bias", dict(logit_bias={VOCAB: 1.0})),
                              (ValueError, "logit_bias", dict(logit_bias={3: float("nan")})),
                              (ValueError, "patch_bias.*3 entries", dict(patch_bias=[None] * 3)),
                              (ValueError, "exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(0, 1e30))),
                              (ValueError, "exponential_decay_length_penalty", dict(exponential_decay_length_penalty=(-1, 1.5))),
                              (NotImplementedError, "output_logits", dict(output_logits=True, logit_bias={3: 1.0})),
                              (NotImplementedError, "output_logits", dict(output_logits=True, patch_bias=[torch.ones(2), None])),
                              (NotImplementedError, "output_logits", dict(output_logits=True, exponential_decay_length_penalty=(0, 1.5)))):
        with pytest.raises(exc, match=name):
            _resolved(m, **kwargs)
    samp, _ = _resolved(m, output_logits=True, logit_bias={3: 1.0}, do_sample=True, seed=1)       # under sampling the raw rows keep their stash
    assert samp.keep_logits and samp.logit_bias


def test_the_decay_comes_from_generation_configs_and_explicit_arguments_win():
    from transformers import GenerationConfig
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    m = _resolving_model()
    assert _resolved(m, generation_config=GenerationConfig(exponential_decay_length_penalty=(2, 1.5)))[0].decay == (2, 1.5)
    assert _resolved(m, generation_config=dict(exponential_decay_length_penalty=[2, 1.5]))[0].decay == (2, 1.5)
    assert _resolved(m, generation_config=dict(exponential_decay_length_penalty=[2, 1.5]), exponential_decay_length_penalty=(1, 1.1))[0].decay == (1, 1.1)
    ck = _resolving_model()
    M.load_generation_config(ck, dict(exponential_decay_length_penalty=[4, 1.25]))          # the checkpoint's generation_config.json
    assert ck.generation_config.exponential_decay_length_penalty == (4, 1.25)
    assert _resolved(ck)[0].decay == (4, 1.25) and _resolved(ck)[0].step_mode().bias
    assert _resolved(ck, exponential_decay_length_penalty=(1, 1.1))[0].decay == (1, 1.1)
    assert _resolved(ck, generation_config=dict(exponential_decay_length_penalty=[2, 1.5]))[0].decay == (2, 1.5)
    assert _resolved(ck, exponential_decay_length_penalty=DECAY_OFF)[0] == GenOptions(eos_ids=(EOS,))       # spelled as off: no checkpoint switches it on
    with pytest.raises(ValueError, match="exponential_decay_length_penalty"):
        M.load_generation_config(_resolving_model(), dict(exponential_decay_length_penalty=[4, -1.0]))
    with pytest.raises(ValueError, match="exponential_decay_length_penalty.*fp32"):          # the range check needs the call's max_new_tokens
        _resolved(_resolving_model(exponential_decay_length_penalty=(0, 2.0)), max_new_tokens=200)
    with pytest.raises(ValueError, match="logit_bias"):                                      # never a generation-config field: the unused-keyword error
        _resolved(m, generation_config=dict(logit_bias={3: 1.0}))


def test_the_rerun_keywords_resolve_back_to_the_options_under_any_generation_config():
    lb = check_logit_bias({5: 1.0, 3: -INF}, VOCAB)
    for gc in (dict(), dict(exponential_decay_length_penalty=(4, 1.25))):
        for lbv, dv in ((None, None), (lb, None), (None, (2, 1.5)), (lb, (2, 1.5))):
            o = dataclasses.replace(resolve_options(hf_defaults(), EOS, VOCAB), logit_bias=lbv, decay=dv)
            kw = o.bias_kwargs()
            assert set(kw) == {"logit_bias", "exponential_decay_length_penalty"} and all(v is not None for v in kw.values())
            assert _resolved(_resolving_model(**gc), **kw)[0] == o, (gc, lbv, dv)


def test_the_bf16_rerun_passes_the_three_on():
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    calls = []

    class Twin:
        def generate(self, **kw):
            calls.append(kw)
            return "out"

    me = object.__new__(M)
    me.operands, me.dtype, me.overflow_reruns, me.prefers_bf16, me._batches_seen, me._fallback = "auto", torch.float16, 0, False, 10, Twin()
    me.precision, me._sd_factory = "default", (lambda: None)
    pb = [None, torch.ones(3)]
    on = dataclasses.replace(GenOptions(eos_ids=(EOS,)), logit_bias=((3, 1.0),), decay=(2, 1.5), patch_bias=True)
    for opts, patch in ((on, pb), (GenOptions(eos_ids=(EOS,)), None)):
        group = dict(opts=opts, T_max=4, schedule=None, sync_every=4, use_graph=True, lane=0)
        sub = dict(inputs=(None, None, None, None), input_ids=None, forced=None, automaton=None, patch_bias=patch)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert me._non_finite_batch(group, sub, True, True, False, False) == "out"
    assert calls[0]["logit_bias"] == {3: 1.0} and calls[0]["exponential_decay_length_penalty"] == (2, 1.5) and calls[0]["patch_bias"] is pb
    assert calls[1]["logit_bias"] == {} and calls[1]["exponential_decay_length_penalty"] == DECAY_OFF and "patch_bias" not in calls[1]


# ------------------------------------------------------------------------------------------------------------ entry points, names, ABI
NAMES = ("logit_bias", "patch_bias", "exponential_decay_length_penalty")


def test_every_entry_point_accepts_the_three():
    from padt_amd import harness, pipeline
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    p = inspect.signature(M.generate).parameters
    assert not set(NAMES) & set(p) and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD          # popped from **kwargs: the parameter list is frozen
    doc = inspect.getdoc(M.generate)
    assert all(n in doc for n in NAMES) and "sequence_bias" in doc and "NaN" in doc
    assert "dict(bias=" in inspect.getdoc(M.generate_launch)
    for fn in (pipeline.rec_batch, pipeline.PipelinedRunner.submit):
        for n in NAMES:
            assert inspect.signature(fn).parameters[n].default is None, (fn, n)
    for n in ("logit_bias", "exponential_decay_length_penalty"):                                 # a batch's patch prior comes from prepare()
        assert inspect.signature(harness.infer_dataset).parameters[n].default is None
    assert "patch_bias" in inspect.getsource(harness.infer_dataset) and "patch_bias" in harness.__doc__
    assert inspect.signature(M.score_completions).parameters["generate_kwargs"].kind is inspect.Parameter.VAR_KEYWORD


def test_score_completions_hands_the_three_to_generate():
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    m = _resolving_model()
    with pytest.raises(_Launched) as e:
        M.score_completions(m, torch.zeros(2, 3, dtype=torch.long), None, None, None, [[5, 6], [6]], logit_bias={5: 1.0},
                            patch_bias=[None, torch.ones(2)], exponential_decay_length_penalty=(0, 1.5))
    opts, kw = e.value.args
    assert opts.forced and opts.token_logprobs and opts.logit_bias == ((5, 1.0),) and opts.decay == (0, 1.5) and opts.patch_bias
    assert kw["patch_bias"][0] is None


def test_infer_dataset_and_rec_batch_hand_them_on(monkeypatch, tmp_path):
    from padt_amd import harness, pipeline
    seen = []

    class Runner:
        def __init__(self, *a, **kw):
            pass

        def submit(self, *a, **kw):
            seen.append(kw)
            return []

        def flush(self):
            return []
    monkeypatch.setattr(harness, "PipelinedRunner", Runner)
    pbs = [[torch.ones(2)], None]
    prepare = lambda s: dict(input_ids=None, attention_mask=None, pixel_values=None, image_grid_thw=None, ids=[s[0]], image_sizes=[(1, 1)],
                             patch_bias=pbs[s[0]])
    harness.infer_dataset(None, None, [0, 1], prepare, str(tmp_path), logit_bias={3: 1.0}, exponential_decay_length_penalty=(1, 1.5), merge=1)
    assert [kw["patch_bias"] for kw in seen] == pbs
    assert all(kw["logit_bias"] == {3: 1.0} and kw["exponential_decay_length_penalty"] == (1, 1.5) for kw in seen)

    class Stop(Exception):
        pass

    class Model:
        def generate(self, **kw):
            raise Stop(kw)
    proc = SimpleNamespace(assign_to_global_vrt_id=lambda ids, g: ids)
    with pytest.raises(Stop) as e:
        pipeline.rec_batch(Model(), proc, torch.zeros(1, 3, dtype=torch.long), None, None, None, logit_bias={3: 1.0}, patch_bias=pbs[0],
                           exponential_decay_length_penalty=(1, 1.5))
    kw = e.value.args[0]
    assert kw["logit_bias"] == {3: 1.0} and kw["patch_bias"] is pbs[0] and kw["exponential_decay_length_penalty"] == (1, 1.5)


def test_what_this_is_not_the_hf_names_stay_rejected():
    for name, v in (("sequence_bias", {(3,): 1.0}), ("forced_eos_token_id", 7), ("min_new_tokens", 2), ("min_length", 5)):
        with pytest.raises(NotImplementedError, match=name):
            check_generate_kwargs({name: v}, 4, None, 3)
    for name in NAMES:                                            # left in **kwargs they are stray keywords: generate() pops them first
        with pytest.raises(ValueError, match=name):
            check_generate_kwargs({name: 1}, 4, None, 3)
    m = _resolving_model()
    with pytest.raises(NotImplementedError, match="sequence_bias"):
        _resolved(m, sequence_bias={(3,): 1.0})
    with pytest.raises(NotImplementedError, match="min_new_tokens"):
        _resolved(m, min_new_tokens=2)
    with pytest.raises(ValueError, match="logit_biass"):
        _resolved(m, logit_biass={3: 1.0})


def test_the_entry_point_is_declared_with_the_documented_argument_list():
    decl = {**_lib.parse_header(), **_lib.parse_header(_lib.HEADER_F16)}
    probe = decl["padt_vrt_head_probe"][2]
    for name in ("padt_vrt_head_bias", "padt_vrt_head_bias_f16"):
        assert decl[name][2] == probe + ["bias", "decay", "t_decay"], name
    for name in ("padt_vrt_head", "padt_vrt_head_ban", "padt_vrt_head_lse", "padt_vrt_head_probe"):        # the others keep their signatures
        assert not {"bias", "decay"} & set(decl[name][2])
    p = inspect.signature(ops.vrt_head_bias).parameters
    assert list(p)[:7] == list(inspect.signature(ops.vrt_head).parameters)[:7]
    for k in ("bias", "decay", "step", "ban", "part_sum", "forced", "probe_val", "logits", "table_packed", "rows", "gen_cfg", "seen"):
        assert p[k].default is None, k
