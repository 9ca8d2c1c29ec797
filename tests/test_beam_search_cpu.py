"""generate(beam_width=, n_best=, beam_length_penalty=, beam_early_stopping=) as host logic: generation.beam_step against the installed
transformers' beam-search helpers on the same candidate streams, beam_backtrace, check_beam's normal forms and refusals, the length table,
GenOptions / StepMode, the keywords' way through generate() to _launch, the refusal list by name and the C ABI of the three kernels.  No GPU."""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

from padt_amd import _lib, ops
from padt_amd.generation import (BEAM_EARLY, BEAM_MAX_WIDTH, GenOptions, StepMode, beam_backtrace, beam_keep, beam_len_table, beam_new_state,
                                 beam_step, check_beam, check_beam_compatible, check_beam_session)
from test_score_bias_cpu import EOS, VOCAB, _resolved, _resolving_model

INF = float("inf")
PACKED = dict(head_dim=128, num_attention_heads=2, num_key_value_heads=1)      # a model with the packed KV caches


def _beam_model(**gc):
    """the resolving model of the other CPU tests, with what a beam call asks of the model config"""
    m = _resolving_model(**gc)
    m.config.__dict__.update(PACKED)
    return m
V, PROMPT, STEPS = 24, 2, 6          # the stream's vocabulary, HF's decoder_prompt_len, the call's max_new_tokens
EOS_SETS = {1: (3,), 2: (3, 7)}


def ulps(a, b):
    """|a - b| in units of the fp32 spacing at the larger magnitude"""
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    return abs(a - b) / float(np.spacing(np.float32(max(abs(a), abs(b)))))


def stream(seed, K, eos):
    """log-prob rows [STEPS][K][V]: what the beam in slot p sees at step t — a log-softmax of random logits whose EOS columns are lifted at
    some steps so that hypotheses finish inside and outside the first K candidates"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(STEPS, K, V, generator=g) * 2.0
    lift = torch.rand(STEPS, K, generator=g)
    for e in eos:
        rows[:, :, e] += torch.where(lift > 0.45, 3.0, -1.0)
    return torch.log_softmax(rows, dim=-1)


def hf_mixin():
    from transformers.generation.utils import GenerationMixin

    class Bare(GenerationMixin):
        pass
    return object.__new__(Bare)


def run_hf(lp, K, eos, penalty, early):
    """HF 5.x's _beam_search loop body on the stream, with its own helpers → per step dict(tok, parent, live, finishing, order), the final
    store and the done step"""
    m = hf_mixin()
    keep = max(2, 1 + len(eos)) * K
    max_length = PROMPT + STEPS
    cur_len = PROMPT
    running_sequences = torch.zeros((1, K, max_length), dtype=torch.int64)
    sequences = running_sequences.clone()
    running_beam_scores = torch.zeros((1, K), dtype=torch.float)
    running_beam_scores[:, 1:] = -1e9
    beam_scores = torch.full((1, K), -1e9, dtype=torch.float)
    is_sent_finished = torch.zeros((1, K), dtype=torch.bool)
    unsat = torch.ones((1, 1), dtype=torch.bool)
    running_beam_indices = torch.full((1, K, max_length - cur_len), -1, dtype=torch.int32)
    beam_indices = running_beam_indices.clone()
    top_num_beam_mask = torch.cat((torch.ones(K, dtype=torch.bool), torch.zeros(keep - K, dtype=torch.bool)))
    eos_t = torch.tensor(eos)
    steps, done_at = [], None
    for t in range(STEPS):
        log_probs = lp[t][None] + running_beam_scores[:, :, None]
        flat = log_probs.reshape(1, K * V)
        topk_log_probs, topk_seq, topk_idx = m._get_top_k_continuations(
            accumulated_log_probs=flat, running_sequences=running_sequences, running_beam_indices=running_beam_indices, cur_len=cur_len,
            decoder_prompt_len=PROMPT, do_sample=False, beams_to_keep=keep, num_beams=K, vocab_size=V, batch_size=1)
        hits = (torch.isin(topk_seq[:, :, cur_len], eos_t) | (cur_len + 1 >= max_length))
        running_sequences, running_beam_scores, running_beam_indices = m._get_running_beams_for_next_iteration(
            topk_log_probs=topk_log_probs, topk_running_sequences=topk_seq, topk_running_beam_indices=topk_idx,
            next_token_hits_stopping_criteria=hits, num_beams=K)
        sequences, beam_scores, beam_indices, is_sent_finished = m._update_finished_beams(
            sequences=sequences, topk_running_sequences=topk_seq, beam_scores=beam_scores, topk_log_probs=topk_log_probs,
            beam_indices=beam_indices, topk_running_beam_indices=topk_idx, is_early_stop_heuristic_unsatisfied=unsat,
            is_sent_finished=is_sent_finished, next_token_hits_stopping_criteria=hits, top_num_beam_mask=top_num_beam_mask, num_beams=K,
            cur_len=cur_len, decoder_prompt_len=PROMPT, length_penalty=penalty, early_stopping=early)
        steps.append(dict(tok=running_sequences[0, :, cur_len].tolist(), parent=running_beam_indices[0, :, t].tolist(),
                          live=running_beam_scores[0].tolist(), finishing=hits[0].tolist(), values=topk_log_probs[0].tolist(),
                          order=[(int(b), int(c)) for b, c in zip(topk_idx[0, :, t].tolist(), topk_seq[0, :, cur_len].tolist())],
                          sent=is_sent_finished[0].tolist(), scores=beam_scores[0].tolist()))
        cur_len += 1
        unsat = m._check_early_stop_heuristic(
            is_early_stop_heuristic_unsatisfied=unsat, running_beam_scores=running_beam_scores, beam_scores=beam_scores,
            is_sent_finished=is_sent_finished, cur_len=cur_len, max_length=max_length, decoder_prompt_len=PROMPT, early_stopping=early,
            length_penalty=penalty)
        if not bool(m._beam_search_has_unfinished_sequences(unsat, is_sent_finished, hits, early)):
            done_at = t
            break
    store = [dict(score=float(beam_scores[0, k]), sent=bool(is_sent_finished[0, k]),
                  tokens=[int(x) for x, i in zip(sequences[0, k, PROMPT:].tolist(), beam_indices[0, k].tolist()) if i >= 0],
                  parents=[int(i) for i in beam_indices[0, k].tolist() if i >= 0]) for k in range(K)]
    return steps, store, done_at


GRID = list(itertools.product((1, 2, 3, 4), (1, 2), (0.0, 1.0, 2.0), (False, True, "never")))
SEEN = dict(max_ulps=0.0, early_done=0, merged=0, outside=0)


@pytest.mark.parametrize("K,n_eos,penalty,early", GRID, ids=[f"K{k}-eos{n}-lp{p:g}-{e}" for k, n, p, e in GRID])
def test_beam_step_is_hfs_beam_search(K, n_eos, penalty, early):
    eos = EOS_SETS[n_eos]
    keep = beam_keep(K, n_eos)
    assert keep == max(2, 1 + n_eos) * K
    lp = stream(1000 + 17 * K + 5 * n_eos, K, eos)
    assert int(torch.isfinite(lp[0, 0]).sum()) >= keep                # beam 0 has `keep` finite columns at step 0: -inf and HF's -1e9 agree
    hf_steps, hf_store, hf_done = run_hf(lp, K, eos, penalty, early)
    table = beam_len_table(penalty, STEPS)
    st = beam_new_state(K)
    toks, parents, lps = [], [], []
    done_at = None
    for t in range(STEPS):
        val, idx = torch.sort(lp[t], dim=-1, descending=True, stable=True)
        tok, par, slp, info = beam_step(st, val[:, :keep].tolist(), idx[:, :keep].tolist(), t, keep, eos, table, STEPS - 1, early,
                                        pad=0, length_penalty=penalty)
        toks.append(tok), parents.append(par), lps.append(slp)
        h = hf_steps[t]
        # the seeds keep adjacent accumulated values apart: the order is then decided by values alone, on both sides
        vals = h["values"]
        assert all(a - b > 1e-4 for a, b in zip(vals, vals[1:])), (t, vals)
        assert [(p, int(idx[p, r])) for p, r in info["order"]] == h["order"], t          # the same candidates in the same order
        assert info["finishing"] == h["finishing"], t
        for c in range(K):
            if st["live"][c] == -INF:                              # a dead slot: HF continues a finished candidate at -1e9
                assert h["live"][c] < -1e8, (t, c)
                continue
            assert (tok[c], par[c]) == (h["tok"][c], h["parent"][c]), (t, c)
            assert st["live"][c] == h["live"][c], (t, c)             # the same fp32 sum
        assert st["sent"] == h["sent"], t
        for e, s, hs in zip(st["store"], st["sent"], h["scores"]):
            if s:
                SEEN["max_ulps"] = max(SEEN["max_ulps"], ulps(e[0], hs))
                assert ulps(e[0], hs) <= 4, (t, e[0], hs)
        SEEN["merged"] += len(info["merged"])
        SEEN["outside"] += sum(1 for i, f in enumerate(info["finishing"]) if f and i >= K)
        if st["done"]:
            done_at = t
            break
    assert done_at == hf_done and done_at is not None
    SEEN["early_done"] += done_at < STEPS - 1
    # store membership and order: tokens and parents walked back, against HF's stored sequences
    hyps = beam_backtrace(st["store"], toks, parents, lps, K)
    for k in range(K):
        assert st["sent"][k] == hf_store[k]["sent"], k
        if not st["sent"][k]:
            continue
        assert hyps[k]["tokens"] == hf_store[k]["tokens"], k
        assert [r[1] for r in hyps[k]["rows"]] == hf_store[k]["parents"], k
        assert hyps[k]["length"] == len(hf_store[k]["tokens"]) == st["store"][k][1] + 1
        assert ulps(hyps[k]["score"], hf_store[k]["score"]) <= 4
        # the score is the fp32 sum of the hypothesis' step log-probs in step order, divided by the table's entry
        acc = np.float32(0.0)
        for x in hyps[k]["logprobs"]:
            acc = np.float32(acc + np.float32(x))
        assert float(np.float32(acc / np.float32(float(table[hyps[k]["length"] - 1])))) == hyps[k]["score"]
    print(f"largest store-score difference so far: {SEEN['max_ulps']:.2f} ulps")


def test_the_grid_reached_every_branch():
    """over the whole grid (it has run before this test in file order): hypotheses merged, EOS candidates outside the first K, samples done before the last step"""
    if SEEN["merged"] == 0:                                           # selected alone: run the grid here
        for case in GRID:
            test_beam_step_is_hfs_beam_search(*case)
    assert SEEN["merged"] > 100 and SEEN["outside"] > 10 and SEEN["early_done"] > 5, SEEN
    assert SEEN["max_ulps"] <= 4


# ------------------------------------------------------------------------------------------------------------ beam_step's edge cases by hand
def test_minus_inf_candidates_dead_beams_and_a_done_sample():
    table = beam_len_table(1.0, 4)
    st = beam_new_state(3)
    assert st["live"] == [0.0, -INF, -INF] and not any(st["sent"]) and st["open"] and not st["done"]
    # beam 0 has two finite columns only: one live beam, one finished hypothesis, the third slot is dead
    val = [[-0.5, -1.0] + [-INF] * 4, [-0.1] * 6, [-0.1] * 6]
    idx = [[5, 3, -1, -1, -1, -1], [1] * 6, [2] * 6]
    tok, par, lp, info = beam_step(st, val, idx, 0, 6, (3,), table, 3, pad=99)
    assert tok == [5, 99, 99] and par == [0, 1, 2] and lp == [-0.5, 0.0, 0.0]
    assert st["live"] == [-0.5, -INF, -INF] and st["store"][0][:4] == (-1.0, 0, 0, 3) and st["sent"] == [True, False, False]
    assert info["order"] == [(0, 0), (0, 1)] and info["finishing"] == [False, True] and not st["done"]
    # ties: equal values across beams go to the lower beam, within a beam to the lower rank
    st = beam_new_state(2)
    st["live"] = [-1.0, -1.0]
    tok, par, lp, info = beam_step(st, [[-1.0, -1.0, -2.0, -3.0], [-1.0, -1.5, -2.0, -3.0]], [[8, 9, 10, 11], [4, 5, 6, 7]], 1, 4, (3,), table, 3)
    assert info["order"] == [(0, 0), (0, 1), (1, 0), (1, 1)] and tok == [8, 9] and par == [0, 0]
    # the last step finishes everything: the first K candidates enter the store, every slot is dead, the sample is done
    tok, par, lp, info = beam_step(st, [[-1.0, -2.0, -3.0, -4.0]] * 2, [[8, 9, 10, 11]] * 2, 3, 4, (3,), table, 3, pad=99)
    assert all(info["finishing"]) and tok == [99, 99] and st["live"] == [-INF, -INF] and st["done"] and st["sent"] == [True, True]
    assert [e[1:4] for e in st["store"]] == [(3, 0, 8), (3, 1, 8)]
    before = (list(st["live"]), list(st["store"]), list(st["sent"]), st["open"])
    assert beam_step(st, [[-1.0] * 4] * 2, [[1] * 4] * 2, 4, 4, (3,), table, 3, pad=99)[:3] == ([99, 99], [0, 1], [0.0, 0.0])
    assert before == (st["live"], st["store"], st["sent"], st["open"])                # a done sample changes nothing
    # nothing at all to continue: every one of no candidates is finishing
    st = beam_new_state(2)
    beam_step(st, [[-INF] * 4] * 2, [[-1] * 4] * 2, 0, 4, (3,), table, 3)
    assert st["done"] and st["live"] == [-INF, -INF]


def test_early_stopping_true_closes_a_full_store_and_never_reads_the_last_entry():
    table = beam_len_table(1.0, 8)
    st = beam_new_state(1)
    tok, *_ = beam_step(st, [[-0.1, -0.2]], [[3, 5]], 0, 2, (3,), table, 7, early=True)
    assert st["sent"] == [True] and st["done"] and tok == [5]                             # K = 1: the first EOS among the best fills the store
    st = beam_new_state(1)
    beam_step(st, [[-0.1, -0.2]], [[3, 5]], 0, 2, (3,), table, 7, early=False)
    # -0.2 / 1 > -0.1 fails: no running beam can beat the finished one
    assert not st["open"] and st["done"]
    st = beam_new_state(1)
    beam_step(st, [[-0.1, -0.2]], [[3, 5]], 0, 2, (3,), table, 7, early="never")
    assert st["open"] and not st["done"]                                                # -0.2 / 8 > -0.1: "never" with a positive penalty divides by the last entry


def test_backtrace_of_an_empty_store_entry():
    assert beam_backtrace(beam_new_state(2)["store"], [], [], [], 2) == [dict(score=-INF, length=0, tokens=[], logprobs=[], rows=[])] * 2


# ------------------------------------------------------------------------------------------------------------ check_beam, the table
def test_check_beam_normal_forms():
    assert check_beam() is None and check_beam(None, None, None, None, 3) is None
    assert check_beam(3) == (3, 1, 1.0, False)
    assert check_beam(4, 2, 0, "never", 2) == (4, 2, 0.0, "never") and isinstance(check_beam(4, 2, 0, "never")[2], float)
    assert check_beam(torch.tensor(2).item(), 2, 2.5, True) == (2, 2, 2.5, True)
    assert check_beam(BEAM_MAX_WIDTH, BEAM_MAX_WIDTH, n_eos=3) == (8, 8, 1.0, False)      # keep = 4 * 8 = 32: the cap itself
    assert beam_keep(1, 1) == 2 and beam_keep(4, 1) == 8 and beam_keep(4, 2) == 12 and beam_keep(8, 3) == ops.TOPK_ROWS_MAX_K


@pytest.mark.parametrize("exc,match,kw", [
    (ValueError, "beam_width", dict(beam_width=0)),
    (ValueError, "beam_width", dict(beam_width=-2)),
    (ValueError, "beam_width", dict(beam_width=2.0)),
    (ValueError, "beam_width", dict(beam_width=True)),
    (NotImplementedError, "beam_width=9.*beam_width=8", dict(beam_width=9)),
    (NotImplementedError, "beam_width=8.*32", dict(beam_width=8, n_eos=4)),
    (NotImplementedError, "beam_width=7.*32", dict(beam_width=7, n_eos=4)),
    (ValueError, "n_best", dict(beam_width=3, n_best=0)),
    (ValueError, "n_best", dict(beam_width=3, n_best=4)),
    (ValueError, "n_best", dict(beam_width=3, n_best=1.5)),
    (ValueError, "beam_length_penalty", dict(beam_width=3, beam_length_penalty=INF)),
    (ValueError, "beam_length_penalty", dict(beam_width=3, beam_length_penalty=float("nan"))),
    (ValueError, "beam_length_penalty", dict(beam_width=3, beam_length_penalty="1")),
    (ValueError, "beam_early_stopping", dict(beam_width=3, beam_early_stopping="always")),
    (ValueError, "beam_early_stopping", dict(beam_width=3, beam_early_stopping=1)),
    (ValueError, "n_best.*beam_width", dict(n_best=2)),
    (ValueError, "beam_length_penalty.*beam_width", dict(beam_length_penalty=1.0)),
    (ValueError, "beam_early_stopping.*beam_width", dict(beam_early_stopping=False)),
])
def test_check_beam_refusals(exc, match, kw):
    with pytest.raises(exc, match=match):
        check_beam(**kw)


def test_the_length_table_is_computed_in_double_and_rounded_once():
    for p in (0.0, 1.0, 2.0, 0.6, -1.5):
        t = beam_len_table(p, 9)
        assert t.dtype == torch.float32 and t.shape == (9,)
        assert t.tolist() == [float(np.float32(float(i + 1) ** p)) for i in range(9)]
    assert beam_len_table(0.0, 3).tolist() == [1.0, 1.0, 1.0]
    assert beam_len_table(400.0, 3).tolist() == [1.0, INF, INF]                          # beyond fp32: inf, never an exception
    assert beam_len_table(1.0, 0).numel() == 0
    cfg = ops.beam_cfg_tensor(3, 6, BEAM_EARLY["never"], 7, True)
    assert cfg.dtype == torch.int32 and cfg.tolist() == [ops.BEAM_CFG_MAGIC, 3, 6, 2, 7, 1, 0, 0] and cfg.numel() == ops.BEAM_CFG_INTS
    assert BEAM_EARLY == {False: 0, True: 1, "never": 2}


# ------------------------------------------------------------------------------------------------------------ options, step mode, round trip
def test_gen_options_carry_the_beam():
    base = GenOptions(eos_ids=(EOS,))
    b = dataclasses.replace(base, beam=(3, 2, 1.0, False))
    assert base.beam is None and base.beam_keep == 0 and base.step_mode() == StepMode() and StepMode().beam == 0
    assert b != base and hash(b) != hash(base) and "beam=(3, 2, 1.0, False)" in repr(b) and "beam=None" in repr(base)
    assert b == dataclasses.replace(base, beam=[3, 2, 1, False]) and dataclasses.replace(b, forced=True).beam == b.beam
    for other in ((4, 2, 1.0, False), (3, 3, 1.0, False), (3, 2, 2.0, False), (3, 2, 1.0, True), (3, 2, 1.0, "never")):
        assert dataclasses.replace(base, beam=other) != b, other
    assert {f.name for f in dataclasses.fields(GenOptions)} == {"repetition_penalty", "eos_ids", "sampling", "rules", "keep_scores", "keep_logits",
                                                                "token_logprobs", "top_logprobs", "patch_logprobs"}      # not a field
    # the step mode: the width and the candidate count select the graph; penalty, early stopping and n_best are device data or host work
    assert b.beam_keep == 6 and b.step_mode() == StepMode(top_k=6, beam=3)
    assert dataclasses.replace(base, eos_ids=(EOS, 9), beam=(3, 2, 1.0, False)).step_mode() == StepMode(top_k=9, beam=3)
    for same in ((3, 1, 1.0, False), (3, 2, 0.0, True), (3, 3, 2.0, "never")):
        assert dataclasses.replace(base, beam=same).step_mode() == b.step_mode()
    assert dataclasses.replace(base, beam=(2, 2, 1.0, False)).step_mode() != b.step_mode()
    assert dataclasses.replace(b, token_logprobs=True).step_mode() == StepMode(top_k=6, beam=3, token_logprobs=True)      # the LSE head + padt_beam_cand_lp
    # the re-run's spelling
    assert b.beam_kwargs() == dict(beam_width=3, n_best=2, beam_length_penalty=1.0, beam_early_stopping=False)
    assert base.beam_kwargs() == dict(beam_width=None, n_best=None, beam_length_penalty=None, beam_early_stopping=None)
    assert check_beam(**b.beam_kwargs()) == b.beam and check_beam(**base.beam_kwargs()) is None


def test_generate_resolves_the_four_keywords():
    m = _beam_model()
    plain, kw0 = _resolved(m)
    off, kw1 = _resolved(m, beam_width=None, n_best=None, beam_length_penalty=None, beam_early_stopping=None)
    assert plain == off == GenOptions(eos_ids=(EOS,)) and kw0["beam_orig"] is None and kw1["beam_orig"] is None and kw1["hooks"] is None
    on, kw = _resolved(m, beam_width=3, n_best=2, beam_length_penalty=0.5, beam_early_stopping="never", output_token_logprobs=True)
    assert on.beam == (3, 2, 0.5, "never") and on.token_logprobs and on.step_mode() == StepMode(top_k=6, beam=3, token_logprobs=True)
    assert kw["hooks"] is None and kw["n_slots"] == 1 and kw["group"] is None
    assert kw["beam_orig"]["input_ids"].shape == (2, 3) and kw["beam_orig"]["image_index"] is None
    dflt, _ = _resolved(m, beam_width=2)
    assert dflt.beam == (2, 1, 1.0, False)
    two, _ = _resolved(m, beam_width=2, eos_token_id=[EOS, 9])
    assert two.beam_keep == 6 and two.step_mode().top_k == 6
    # allowed together: the score edits (the head applies them), a schedule, token log-probs
    ok, kwb = _resolved(m, beam_width=2, logit_bias={5: 1.0}, patch_bias=[torch.ones(4), None], exponential_decay_length_penalty=(1, 1.5),
                        schedule=["t", "v", None])
    assert ok.beam and ok.score_bias and len(kwb["patch_bias"]) == 4 and kwb["patch_bias"][1] is kwb["patch_bias"][0] and kwb["patch_bias"][2] is None
    assert kwb["beam_orig"]["patch_bias"][1] is None and len(kwb["beam_orig"]["patch_bias"]) == 2


class _Expanded(Exception):
    pass


def test_the_call_is_expanded_to_b_times_k_rows_on_the_host():
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    from types import SimpleNamespace

    class Probe(M):
        def _launch(self, opts, input_ids, attention_mask, pixel_values, image_grid_thw, image_index, **kw):
            raise _Expanded(input_ids, attention_mask, image_index, kw)
    m = object.__new__(Probe)
    m.generation_config = _resolving_model().generation_config
    m.config = SimpleNamespace(eos_token_id=EOS, vocab_size=VOCAB, **PACKED)
    m.prefers_bf16, m.precision = False, "default"
    ids = torch.arange(6).view(2, 3)
    am = torch.tensor([[0, 1, 1], [1, 1, 1]])
    with pytest.raises(_Expanded) as e:
        m.generate(input_ids=ids, attention_mask=am, pixel_values=None, image_grid_thw=None, max_new_tokens=4, beam_width=3)
    got_ids, got_am, got_idx, kw = e.value.args
    assert torch.equal(got_ids, ids[[0, 0, 0, 1, 1, 1]]) and torch.equal(got_am, am[[0, 0, 0, 1, 1, 1]]) and got_idx == [0, 0, 0, 1, 1, 1]
    with pytest.raises(_Expanded) as e:                               # an image_index is composed with the repeat
        m.generate(input_ids=ids, attention_mask=None, pixel_values=None, image_grid_thw=None, max_new_tokens=4, beam_width=2, image_index=[1, 1])
    assert e.value.args[1] is None and e.value.args[2] == [1, 1, 1, 1] and e.value.args[3]["beam_orig"]["image_index"] == [1, 1]
    # a beam batch is its own decode group: with a group to join the launch declines
    assert m.generate_launch(ids, None, None, None, 4, hooks=dict(beam=dict(beam_width=2)), group=dict(owner=m)) is None


REFUSED = [
    ("do_sample", dict(do_sample=True, seed=1)),
    ("repetition_penalty", dict(repetition_penalty=1.2)),
    ("no_repeat_ngram_size", dict(no_repeat_ngram_size=2)),
    ("bad_words_ids", dict(bad_words_ids=[[4, 5]])),
    ("suppress_tokens", dict(suppress_tokens=[4])),
    ("begin_suppress_tokens", dict(begin_suppress_tokens=[4])),
    ("forced_tokens", dict(forced_tokens=[[5], [6]])),
    ("stop_sequences", dict(stop_sequences=[[4, 5]])),
    ("min_tokens", dict(min_tokens=2)),
    ("max_tokens", dict(max_tokens=3)),
    ("frequency_penalty", dict(frequency_penalty=0.5)),
    ("presence_penalty", dict(presence_penalty=0.5)),
    ("patch_suppression", dict(patch_suppression=(1, 2.0))),
    ("top_logprobs", dict(top_logprobs=3)),
    ("output_patch_logprobs", dict(output_patch_logprobs=True)),
    ("output_scores", dict(output_scores=True)),
    ("output_logits", dict(output_logits=True)),
    ("logits_processor", dict(logits_processor=[lambda i, s: s])),
    ("stopping_criteria", dict(stopping_criteria=[lambda i, s: False])),
]


@pytest.mark.parametrize("name,kw", REFUSED, ids=[n for n, _ in REFUSED])
def test_what_beam_search_refuses_by_name(name, kw):
    m = _beam_model()
    with pytest.raises(NotImplementedError, match=r"beam_width[\s\S]*" + name):
        _resolved(m, beam_width=2, **kw)
    _resolved(m, **kw)                                                # ... and only together with beam_width


def test_the_other_refusals():
    from padt_amd.generation import TokenAutomaton
    m = _beam_model()
    with pytest.raises(NotImplementedError, match=r"beam_width[\s\S]*token_automaton"):
        _resolved(m, beam_width=2, token_automaton=TokenAutomaton([[(TokenAutomaton.TEXT, 0), (TokenAutomaton.EOS, 1)], []]))
    m.precision = "reference"
    with pytest.raises(NotImplementedError, match=r"beam_width[\s\S]*precision"):
        _resolved(m, beam_width=2)
    m.precision = "default"
    for kw in (dict(n_best=2), dict(beam_length_penalty=2.0), dict(beam_early_stopping=True)):        # without beam_width: ValueError
        with pytest.raises(ValueError, match="beam_width"):
            _resolved(m, **kw)
    with pytest.raises(NotImplementedError, match="beam_width=9"):
        _resolved(m, beam_width=9)
    with pytest.raises(NotImplementedError, match="beam_width=7"):
        _resolved(m, beam_width=7, eos_token_id=[EOS, 1, 2, 3])      # keep = 5 * 7 > 32
    # HF's names keep today's behaviour exactly
    for name, v in (("num_beams", 4), ("num_beam_groups", 2), ("num_return_sequences", 2), ("length_penalty", 2.0), ("early_stopping", True)):
        with pytest.raises(NotImplementedError, match=name):
            _resolved(m, **{name: v})
        with pytest.raises(NotImplementedError, match=name):
            _resolved(m, beam_width=2, **{name: v})
    _resolved(m, num_beams=1, num_return_sequences=1, length_penalty=1.0, early_stopping=False)
    check_beam_compatible(GenOptions(eos_ids=(EOS,), token_logprobs=True, logit_bias=((3, 1.0),), decay=(1, 1.5), patch_bias=True))


def test_a_model_without_packed_caches_and_too_many_rows_are_refused_before_anything_is_launched():
    from types import SimpleNamespace
    ok = SimpleNamespace(**PACKED)
    check_beam_session(ok, 16, 8)                                     # 128 rows: the cap itself
    check_beam_session(SimpleNamespace(head_dim=128, num_attention_heads=32, num_key_value_heads=2), 1, 1)
    with pytest.raises(NotImplementedError, match=r"beam_width=8.*17 queries.*136 rows.*128"):
        check_beam_session(ok, 17, 8)
    for cfg in (SimpleNamespace(head_dim=80, num_attention_heads=2, num_key_value_heads=1),
                SimpleNamespace(head_dim=128, num_attention_heads=34, num_key_value_heads=2)):
        with pytest.raises(NotImplementedError, match=r"beam_width.*packed KV caches"):
            check_beam_session(cfg, 2, 2)
    assert ops.DECODE_ROWS_MAX == 128
    # ... through generate(): raised where the options resolve, the launch is never reached
    m = _beam_model()
    ids = torch.zeros(33, 3, dtype=torch.long)
    with pytest.raises(NotImplementedError, match=r"beam_width=4.*33 queries.*132 rows"):
        m.generate(input_ids=ids, attention_mask=None, pixel_values=None, image_grid_thw=None, max_new_tokens=4, beam_width=4)
    m.config.head_dim = 80
    with pytest.raises(NotImplementedError, match=r"beam_width.*packed KV caches"):
        _resolved(m, beam_width=2)
    _resolved(m)                                                      # ... and only with beam_width


# ------------------------------------------------------------------------------------------------------------ the option's way through the callers
class _FakeModel:
    """generate() / vl_decode() of a model, recorded: what rec_batch hands over and what it does with B * n_best returned rows"""

    def __init__(self, rows, L, T):
        self.rows, self.L, self.T, self.calls = rows, L, T, {}

    def generate(self, **kw):
        from padt_amd.modeling import CustomGenerateDecoderOnlyOutput as Out
        self.calls["generate"] = kw
        seq = torch.cat([kw["input_ids"].repeat_interleave(self.rows // kw["input_ids"].shape[0], 0),
                         torch.full((self.rows, self.T), 5, dtype=torch.long)], 1)
        return Out(sequences=seq, hidden_states=[], token_logprobs=None, top_token_ids=None, top_logprobs=None, patch_logprobs=None,
                   past_image_embeds="proto", past_high_res_image_embeds="high", past_visual_pe="pe",
                   sequences_scores=torch.arange(self.rows).float(), sequence_lengths=torch.full((self.rows,), self.T))

    def vl_decode(self, feats, proto, high, grid, pe):
        self.calls["vl_decode"] = dict(feats=feats, grid=grid)
        return dict(pred_boxes=torch.zeros(0, 4))


def test_rec_batch_hands_the_option_over_and_reads_b_times_n_best_rows():
    import padt_amd
    import parity_util as U
    from padt_amd import pipeline
    cfg = padt_amd.small_test_config()
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 64), 2)
    proc.model_embed_token_size = cfg.vocab_size
    grid = torch.tensor([[1, 4, 4], [1, 2, 4]])
    ids = torch.randint(0, 100, (2, 6))
    model = _FakeModel(rows=4, L=6, T=3)
    decoded, completions, labels, vrts = pipeline.rec_batch(model, proc, ids, None, None, grid, max_new_tokens=3, beam_width=3, n_best=2,
                                                            beam_length_penalty=0.5, beam_early_stopping="never",
                                                            need_thinking_mask=torch.tensor([True, False]))
    kw = model.calls["generate"]
    assert (kw["beam_width"], kw["n_best"], kw["beam_length_penalty"], kw["beam_early_stopping"]) == (3, 2, 0.5, "never")
    assert kw["input_ids"].shape == (2, 6) and kw["image_grid_thw"] is grid          # the caller's rows: generate() expands them itself
    assert len(completions) == len(labels) == len(vrts) == 4                          # row b * n_best + r: sample b's r-th best
    assert model.calls["vl_decode"]["grid"].tolist() == grid[[0, 0, 1, 1]].tolist() and len(model.calls["vl_decode"]["feats"]) == 4
    assert decoded["sequences_scores"].tolist() == [0.0, 1.0, 2.0, 3.0] and decoded["sequence_lengths"].tolist() == [3] * 4
    g, m, n = pipeline.beam_rows(2, grid, torch.tensor([True, False]), 2)
    assert g.tolist() == grid[[0, 0, 1, 1]].tolist() and m.tolist() == [True, True, False, False] and n == 4
    assert pipeline.beam_rows(1, grid, None, 2)[1] is None
    # without the option: the call it was
    plain = _FakeModel(rows=2, L=6, T=3)
    pipeline.rec_batch(plain, proc, ids, None, None, grid, max_new_tokens=3)
    assert plain.calls["generate"]["beam_width"] is None and plain.calls["vl_decode"]["grid"] is grid


def test_a_flagged_beam_batch_is_rerun_from_the_callers_rows():
    """operands="auto": the bf16 twin gets the rows the caller gave (not their expansion to B * K) and the beam keywords"""
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    seen = {}

    class Twin:
        def generate(self, **kw):
            seen.update(kw)
            return "rerun"
    m = object.__new__(M)
    m.operands, m.dtype, m.overflow_reruns, m.prefers_bf16, m._batches_seen = "auto", torch.float16, 0, False, 10
    m.fallback_model = lambda: Twin()
    ids, am = torch.arange(6).view(2, 3), torch.ones(2, 3, dtype=torch.long)
    pb = [torch.ones(4), None]
    opts = GenOptions(eos_ids=(EOS,), token_logprobs=True, beam=(3, 2, 0.5, True), patch_bias=True)
    group = dict(opts=opts, T_max=4, schedule=None, sync_every=16, use_graph=True, lane=0)
    sub = dict(input_ids=ids.repeat_interleave(3, 0), inputs=(am.repeat_interleave(3, 0), "pix", "grid", [0, 0, 0, 1, 1, 1]),
               patch_bias=[pb[0]] * 3 + [None] * 3,
               beam_orig=dict(input_ids=ids, attention_mask=am, image_index=None, patch_bias=pb))
    with pytest.warns(RuntimeWarning, match="fp16 range exceeded"):
        assert m._non_finite_batch(group, sub, True, True, False, False) == "rerun"
    assert seen["input_ids"] is ids and seen["attention_mask"] is am and seen["image_index"] is None and seen["patch_bias"] is pb
    assert (seen["beam_width"], seen["n_best"], seen["beam_length_penalty"], seen["beam_early_stopping"]) == (3, 2, 0.5, True)
    assert seen["output_token_logprobs"] is True and seen["pixel_values"] == "pix" and seen["max_new_tokens"] == 4


# ------------------------------------------------------------------------------------------------------------ header / binding agreement
def test_reported_log_probs_are_recorded_and_never_added():
    """cand_rep: what the step returns and the store keeps as log-probs; values, order and scores are cand_val's"""
    table = beam_len_table(1.0, 4)
    val, idx = [[-0.5, -1.0, -2.0, -3.0], [0.0] * 4], [[5, 3, 6, 7], [-1] * 4]
    reported = [[-0.5000001, -1.0000001, -2.0000002, -3.0000002], [9.0] * 4]
    a, b = beam_new_state(2), beam_new_state(2)
    ta = beam_step(a, val, idx, 0, 4, (3,), table, 3)
    tb = beam_step(b, val, idx, 0, 4, (3,), table, 3, cand_rep=reported)
    assert ta[:2] == tb[:2] and ta[2] == [-0.5, -2.0] and tb[2] == [-0.5000001, -2.0000002]
    assert a["live"] == b["live"] == [-0.5, -2.0] and a["store"][0][:4] == b["store"][0][:4] == (-1.0, 0, 0, 3)
    assert a["store"][0][4] == -1.0 and b["store"][0][4] == -1.0000001


def test_the_entry_points_are_declared_as_the_bindings_call_them():
    import inspect
    import re
    decls = _lib.parse_header()
    src = inspect.getsource(ops)
    for name, n_args in (("padt_beam_step", 40), ("padt_beam_cand_lp", 14), ("padt_beam_reorder_kv", 12), ("padt_beam_finalize", 24)):
        assert name in decls and len(decls[name][1]) == n_args, name
        call = src[src.index(f"_lib.load().{name}("):]
        depth, n = 0, 1
        for ch in call[call.index("(", call.index(name)) + 1:]:
            if ch in "([":
                depth += 1
            elif ch in ")]":
                if depth == 0:
                    break
                depth -= 1
            elif ch == "," and depth == 0:
                n += 1
        assert n == n_args, (name, n, n_args)
    # the kernel file defines exactly these four, and the build compiles it once (no fp16 twin: it moves raw bits)
    from padt_amd import build
    csrc = open(build.CSRC + "/beam_search.hip").read()
    assert set(re.findall(r'extern "C"\s+int\s+(padt_\w+)\s*\(', csrc)) == {"padt_beam_step", "padt_beam_cand_lp", "padt_beam_reorder_kv", "padt_beam_finalize"}
    assert "beam_search.hip" in build.SOURCES and "beam_search.hip" not in build.TWIN_SOURCES
    assert ops.BEAM_MAX_WIDTH == BEAM_MAX_WIDTH == 8 and "BEAM_MAX_K = 8" in csrc and f"0x{ops.BEAM_CFG_MAGIC:08x}" in csrc
