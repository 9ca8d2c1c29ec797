"""generate(stop_sequences=, min_tokens=, max_tokens=) as host logic: the specification functions of padt_amd/generation.py (stop_ban_ids
against HF's MinNewTokensLengthLogitsProcessor bit for bit, stop_state on hand-written cases), the packed table and its caps, the argument
policy by name, GenOptions / StepMode, and the keywords' way through generate() to _launch.  No GPU."""
import dataclasses

import pytest
import torch

import stop_rules_util as S
from padt_amd import ops
from padt_amd.generation import (NO_BUDGET, STOP_MAX_LEN, STOP_MAX_SEQS, GenOptions, StepMode, check_generate_kwargs, check_max_tokens,
                                 check_min_tokens, check_stop_sequences, stop_ban_ids, stop_scan, stop_state, stop_table)
from test_score_bias_cpu import EOS, VOCAB, _resolved, _resolving_model

INF = float("inf")


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ the ban against HF
@pytest.mark.parametrize("eos", [(37,), (37, 41), (37, 41, 112, 5)], ids=["1 id", "2 ids", "4 ids"])
def test_ban_is_hfs_min_new_tokens_processor(eos):
    from transformers.generation.logits_process import MinNewTokensLengthLogitsProcessor
    g = torch.Generator().manual_seed(len(eos))
    L, W, n_min = 6, 113, 4
    proc = MinNewTokensLengthLogitsProcessor(L, n_min, list(eos))
    for step in range(0, n_min + 3):                                  # both sides of min_tokens
        rows = torch.randn(3, W, generator=g) * 4
        rows[1, eos[-1]] = -INF                                       # already -inf in an EOS column
        rows[2, 40] = -INF
        ids = torch.zeros(3, L + step, dtype=torch.long)
        want = proc(ids, rows.clone())
        banned = stop_ban_ids(step, n_min, eos)
        assert banned == (sorted(eos) if step < n_min else [])
        got = rows.clone()
        got[:, banned] = -INF
        assert torch.equal(bits(got), bits(want)), step
    assert stop_ban_ids(0, 2, (37, -1, 41, 37, -1)) == [37, 41] and stop_ban_ids(0, 0, eos) == []


# ------------------------------------------------------------------------------------------------------------ stop_state by hand
LIVE_ROWS = [r for r in S.ROWS if r.preset is None]                   # the row finished on entry is a kernel case: it is never looked at


@pytest.mark.parametrize("row", LIVE_ROWS, ids=[r.name for r in LIVE_ROWS])
def test_stop_state_on_the_hand_written_rows(row):
    step, reason, index = row.want
    for n in range(1, step + 1):                                      # not finished before ...
        assert stop_state(row.tokens, n, S.SEQS, row.min_tokens, row.max_tokens, S.EOS_IDS) == (False, None, -1), n
    assert stop_state(row.tokens, step + 1, S.SEQS, row.min_tokens, row.max_tokens, S.EOS_IDS) == (True, reason, index)
    assert stop_scan(row.tokens, S.SEQS, row.min_tokens, row.max_tokens, S.EOS_IDS) == row.want


def test_stop_state_corners():
    assert stop_state([5], 0, S.SEQS, 0, 1, S.EOS_IDS) == (False, None, -1)              # no token yet
    assert stop_state([7], 1, S.SEQS, 5, None, S.EOS_IDS) == (True, "eos", -1)           # a (forced) EOS below min_tokens still ends the row
    assert stop_state([3, 4], 2, S.SEQS, 3, None, S.EOS_IDS) == (False, None, -1)        # the gate
    assert stop_state([3, 4], 2, S.SEQS, 2, None, S.EOS_IDS) == (True, "stop", 0)
    assert stop_state([3, 4], 2, None, 0, 2, S.EOS_IDS) == (True, "length", -1)
    assert stop_state([3, 4], 2, None, 0, None, S.EOS_IDS) == (False, None, -1)
    assert stop_state([3, 4, 8, 8], 2, S.SEQS, 0, None, S.EOS_IDS) == (True, "stop", 0)  # only the first n tokens are read
    assert stop_scan([2, 2, 2], S.SEQS, 0, NO_BUDGET, S.EOS_IDS) == (-1, "length", -1)   # still running at the end
    # the simulation every kernel launch is compared with ends every hand-written row where its `want` says
    state = S.initial_state()
    for n in range(1, S.T_MAX + 2):
        S.simulate(n, state)
    unf, step, reason, index = state
    assert unf == [0] * len(S.ROWS)
    assert [(s, r, i) for s, r, i in zip(step, reason, index)] == [(w[0], S.REASON_CODE[w[1]], w[2]) for w in (r.want for r in S.ROWS)]


# ------------------------------------------------------------------------------------------------------------ the table and its caps
def test_table_layout_and_caps():
    key = check_stop_sequences(S.SEQS, 1000)
    assert key == tuple(tuple(q) for q in S.SEQS) and key[2] == key[3]                   # the caller's order; a duplicate keeps both places
    t = stop_table(key)
    assert t.dtype == torch.int32 and t.numel() == ops.STOP_RULES_INTS == 2 + 32 + 32 * 32
    assert int(t[0]) == ops.STOP_RULES_MAGIC and int(t[1]) == len(S.SEQS)
    assert t[2: 2 + len(S.SEQS)].tolist() == [len(q) for q in S.SEQS] and not bool(t[2 + len(S.SEQS): 34].any())
    for i, q in enumerate(S.SEQS):
        assert t[34 + 32 * i: 34 + 32 * i + len(q)].tolist() == q
    assert stop_table(None)[:2].tolist() == [ops.STOP_RULES_MAGIC, 0] and not bool(stop_table(())[2:].any())
    # at the caps, and one past them
    full = [[i] * STOP_MAX_LEN for i in range(STOP_MAX_SEQS)]
    assert stop_table(check_stop_sequences(full, 1000))[-1] == STOP_MAX_SEQS - 1
    with pytest.raises(NotImplementedError, match=r"stop_sequences.*at most 32"):
        check_stop_sequences(full + [[1]], 1000)
    with pytest.raises(NotImplementedError, match=r"stop_sequences.*33 ids; at most 32"):
        check_stop_sequences([[1] * (STOP_MAX_LEN + 1)], 1000)
    assert check_stop_sequences(None, 1000) is None
    assert check_stop_sequences([torch.tensor([3, 4]), (5,)], 1000) == ((3, 4), (5,))


def test_argument_policy_by_name():
    for bad in ([], [[]], [[1], []], 5, "ab", [[1.5]], [[True]], [[-1]]):
        with pytest.raises(ValueError, match="stop_sequences"):
            check_stop_sequences(bad, 1000)
    with pytest.raises(NotImplementedError, match="stop_sequences: id 1000 is not a text id"):      # the rule table's wording
        check_stop_sequences([[3, 1000]], 1000)
    with pytest.raises(NotImplementedError, match="is not a text id"):
        ops.gen_rules_key(suppress_tokens=[1000], vocab_size=1000)
    # max_tokens: 1 .. max_new_tokens, an int or one int per row
    assert check_max_tokens(None, 2, 8) is None and check_max_tokens(8, 2, 8) == [8, 8] and check_max_tokens([1, 8], 2, 8) == [1, 8]
    assert check_max_tokens(torch.tensor([3, 4]), 2, 8) == [3, 4]
    for bad in (0, 9, [1, 9], [0, 1], [1], [1, 2, 3], 1.5, [1, 2.0], True, "3"):
        with pytest.raises(ValueError, match="max_tokens"):
            check_max_tokens(bad, 2, 8)
    # min_tokens: 0 .. the row's budget; one value is an int (part of the options), per-row values a list (they travel with the batch)
    assert check_min_tokens(None, 2, 8) is None and check_min_tokens(0, 2, 8) == 0 and check_min_tokens(8, 2, 8) == 8
    assert check_min_tokens([0, 8], 2, 8) == [0, 8] and check_min_tokens(3, 2, 8, [3, 4]) == 3 and check_min_tokens([3, 4], 2, 8, [3, 4]) == [3, 4]
    for bad, budget in ((-1, None), (9, None), ([0, 9], None), ([0, -2], None), (4, [3, 8]), ([1, 5], [8, 4]), ([1], None), (2.0, None), (False, None)):
        with pytest.raises(ValueError, match="min_tokens"):
            check_min_tokens(bad, 2, 8, budget)
    # HF's names stay rejected exactly as they are
    for name, v in (("min_new_tokens", 2), ("min_length", 5), ("stop_strings", ["x"]), ("max_time", 1.0)):
        with pytest.raises(NotImplementedError, match=name):
            check_generate_kwargs({name: v}, 4, None, 3)
    for name in ("stop_sequences", "min_tokens", "max_tokens"):       # the new names are generate()'s own keywords, not stray model kwargs
        with pytest.raises(ValueError, match=name):
            check_generate_kwargs({name: 1}, 4, None, 3)


# ------------------------------------------------------------------------------------------------------------ options and step mode
def test_gen_options_equality_hash_and_step_mode():
    base = GenOptions(eos_ids=(EOS,))
    a = dataclasses.replace(base, stop_sequences=((3, 4), (5,)))
    a2 = dataclasses.replace(base, stop_sequences=[[3, 4], [5]])
    b = dataclasses.replace(base, stop_sequences=((5,), (3, 4)))      # another order is another stop_index: not the same options
    m1, m2, rl = dataclasses.replace(base, min_tokens=1), dataclasses.replace(base, min_tokens=2), dataclasses.replace(base, row_limits=True)
    assert a == a2 and hash(a) == hash(a2) and len({base, a, a2, b, m1, m2, rl}) == 6
    assert dataclasses.replace(base, min_tokens=0) != base            # given is given: the output then carries the finish fields
    assert not base.stop and all(o.stop for o in (a, b, m1, m2, rl))
    assert base.step_mode() == StepMode() and not StepMode().stop
    on = StepMode(stop=True)
    assert a.step_mode() == b.step_mode() == m1.step_mode() == rl.step_mode() == on        # one captured graph for every value
    assert dataclasses.replace(a, forced=True).stop_sequences == a.stop_sequences and dataclasses.replace(m1, keep_scores=True).min_tokens == 1
    names = {f.name for f in dataclasses.fields(GenOptions)}
    assert not names & {"stop_sequences", "min_tokens", "row_limits"} and not set(a.generate_kwargs()) & {"stop_sequences", "min_tokens", "max_tokens"}
    assert "stop_sequences=((3, 4), (5,))" in repr(a) and "min_tokens=2" in repr(m2)
    big = dataclasses.replace(base, stop_sequences=tuple((i,) * 32 for i in range(32)))
    assert len(repr(big)) < 1000
    # the re-run's spelling resolves back
    for o in (base, a, m1, dataclasses.replace(a, min_tokens=3)):
        kw = o.stop_kwargs()
        assert set(kw) == {"stop_sequences", "min_tokens"}
        again = dataclasses.replace(base, stop_sequences=check_stop_sequences(kw["stop_sequences"], VOCAB), min_tokens=kw["min_tokens"])
        assert again == o


def test_generate_resolves_the_three_arguments():
    m = _resolving_model()
    plain, kw0 = _resolved(m)
    off, kw1 = _resolved(m, stop_sequences=None, min_tokens=None, max_tokens=None)
    assert plain == off == GenOptions(eos_ids=(EOS,)) and plain.step_mode() == StepMode()      # without them: the parent's options and step mode
    assert kw0["stop"] is None and kw1["stop"] is None and kw1["hooks"] is None
    on, kw = _resolved(m, stop_sequences=[[3, 4], [5]], min_tokens=2, max_tokens=[4, 8])
    assert on.stop_sequences == ((3, 4), (5,)) and on.min_tokens == 2 and on.row_limits and on.step_mode() == StepMode(stop=True)
    assert kw["stop"] == dict(min_tokens=None, max_tokens=[4, 8]) and kw["hooks"] is None
    per, kwp = _resolved(m, min_tokens=[1, 2])
    assert per.min_tokens is None and per.row_limits and per.stop_sequences is None and kwp["stop"] == dict(min_tokens=[1, 2], max_tokens=None)
    one, kwo = _resolved(m, max_tokens=5)
    assert one.row_limits and kwo["stop"]["max_tokens"] == [5, 5]
    assert _resolved(m, min_tokens=1)[0] != _resolved(m, min_tokens=2)[0]                   # a one-value minimum decides the decode group ...
    assert _resolved(m, max_tokens=[1, 2])[0] == _resolved(m, max_tokens=[3, 4])[0] == _resolved(m, min_tokens=[0, 1])[0]      # ... per-row lists do not
    # the bf16 re-run: generate_kwargs() + stop_kwargs() + the batch's own lists resolve back to the same call
    again, kwa = _resolved(m, **on.generate_kwargs(), **on.warper_kwargs(), **on.bias_kwargs(), **on.stop_kwargs(),
                           **{k: v for k, v in kw["stop"].items() if v is not None})
    assert again == on and kwa["stop"] == kw["stop"]
    both, _ = _resolved(m, stop_sequences=[[3]], forced_tokens=[[5], [6]], no_repeat_ngram_size=2, logit_bias={5: 1.0})
    assert both.stop and both.forced and both.rules is not None and both.logit_bias
    for exc, name, kwargs in ((ValueError, "stop_sequences", dict(stop_sequences=[])),
                              (ValueError, "stop_sequences.*sequence 1 is empty", dict(stop_sequences=[[1], []])),
                              (NotImplementedError, "stop_sequences.*not a text id", dict(stop_sequences=[[VOCAB]])),
                              (NotImplementedError, "stop_sequences.*at most 32", dict(stop_sequences=[[1]] * 33)),
                              (NotImplementedError, "stop_sequences.*at most 32", dict(stop_sequences=[[1] * 33])),
                              (ValueError, "min_tokens.*negative", dict(min_tokens=-1)),
                              (ValueError, "min_tokens.*budget of 8", dict(min_tokens=9)),
                              (ValueError, "min_tokens.*budget of 3", dict(min_tokens=4, max_tokens=[8, 3])),
                              (ValueError, "max_tokens", dict(max_tokens=0)),
                              (ValueError, "max_tokens", dict(max_tokens=9)),
                              (ValueError, "max_tokens.*3 entries", dict(max_tokens=[1, 2, 3])),
                              (NotImplementedError, "min_new_tokens", dict(min_new_tokens=2)),
                              (NotImplementedError, "min_length", dict(min_length=5)),
                              (NotImplementedError, "stop_strings", dict(stop_strings=["x"])),
                              (NotImplementedError, "max_time", dict(max_time=1.0))):
        with pytest.raises(exc, match=name):
            m.generate(input_ids=torch.zeros(2, 3, dtype=torch.long), attention_mask=None, pixel_values=None, image_grid_thw=None,
                       max_new_tokens=8, **kwargs)


def test_the_bf16_rerun_passes_the_three_on():
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
    base = GenOptions(eos_ids=(EOS,))
    on = dataclasses.replace(base, stop_sequences=((3, 4), (5,)), min_tokens=2, row_limits=True)
    rows = dataclasses.replace(base, row_limits=True)
    for opts, stop in ((on, dict(min_tokens=None, max_tokens=[4, 8])), (rows, dict(min_tokens=[1, 2], max_tokens=None)), (base, None)):
        group = dict(opts=opts, T_max=8, schedule=None, sync_every=4, use_graph=True, lane=0)
        sub = dict(inputs=(None, None, None, None), input_ids=None, forced=None, automaton=None, patch_bias=None, stop=stop)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert me._non_finite_batch(group, sub, True, True, False, False) == "out"
    assert calls[0]["stop_sequences"] == [[3, 4], [5]] and calls[0]["min_tokens"] == 2 and calls[0]["max_tokens"] == [4, 8]
    assert calls[1]["stop_sequences"] is None and calls[1]["min_tokens"] == [1, 2] and "max_tokens" not in calls[1]
    assert calls[2]["stop_sequences"] is None and calls[2]["min_tokens"] is None and "max_tokens" not in calls[2]      # None: the call without them


def test_the_keywords_reach_every_entry_point():
    import inspect
    from padt_amd import harness, pipeline
    for fn in (pipeline.rec_batch, pipeline.PipelinedRunner.submit, harness.infer_dataset):
        assert {"stop_sequences", "min_tokens", "max_tokens"} <= set(inspect.signature(fn).parameters), fn
