"""DecodeSession is the only writer of its per-generate state: what begin() leaves for a new decode group, what add_batch() writes for one
batch's rows, what a second begin() resets and keeps.  A session on the CPU over the small test configuration: no kernel runs (the
repetition penalty's bitmap, written by ops.seen_init, is the GPU suite's).  No GPU."""
import dataclasses

import pytest
import torch

from padt_amd import config, ops
from padt_amd.generation import NO_BUDGET, GenOptions, Sampling, StepMode
from padt_amd.llm import DecodeSession
from padt_amd.weights import PreparedWeights, _pad_to

B, S_MAX, NP_MAX, T_MAX = 4, 128, 16, 6                          # 2 slots of 2 rows; 8 patch rows per batch
FEATURE = ("scores", "raw_scores", "part_sum", "logprobs", "top_idx", "top_val", "top_flat", "patch_lp", "topk_ws", "forced", "probe_val", "atab",
           "astate", "aban", "bias", "decay", "stab", "min_tok", "max_tok", "finish_step", "finish_reason", "stop_index", "sban", "summary_stop",
           "summary_stop_host", "cnt_text", "cnt_patch", "near", "cpen", "cgrid", "cradius", "logits", "hid32")


@pytest.fixture()
def sess():
    cfg = config.small_test_config()
    W = PreparedWeights()
    W.llm_weights, W.op16, W.fp8_prefill, W.llm_ipad = "bf16", torch.float16, False, _pad_to(cfg.intermediate_size, 64)
    return DecodeSession(cfg, W, B, S_MAX, NP_MAX, T_MAX, "cpu")


def all_on(cfg, **kw):
    """Every option of GenOptions that owns session state (the repetition penalty apart: its bitmap is written by a kernel)"""
    o = dict(sampling=Sampling(1.0, 5, 1.0, 3), rules=ops.gen_rules_key(3, vocab_size=cfg.vocab_size), keep_scores=True, token_logprobs=True,
             top_logprobs=3, patch_logprobs=True, forced=True, logit_bias=((1, 0.5), (7, -1.0)), decay=(2, 1.1), patch_bias=True,
             stop_sequences=((1, 2), (3,)), min_tokens=1, row_limits=True, count_penalties=True, patch_suppression=True)
    o.update(kw)
    return GenOptions(**o)


def dirty(s):
    for v in vars(s).values():
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(t, torch.Tensor):
                t.fill_(7)


def ints(t):
    return t.tolist()


def test_begin_makes_a_dirtied_session_neutral(sess):
    dirty(sess)
    sess.begin(GenOptions(), schedule=["t", "v", None, "e"])
    pad = sess.cfg.pad_token_id
    assert ints(sess.mode_table[:7]) == [1, 2, 0, 3, 0, 0, 0]
    assert ints(sess.step) == [0] and ints(sess.err) == [0]
    assert ints(sess.unfinished) == [0] * B and ints(sess.slot) == [0] * B
    assert ints(sess.lens) == [1] * B and ints(sess.pos3) == [[0] * B] * 3 and ints(sess.cur_tok) == [pad] * B
    assert ints(sess.vrt_off) == [0] * (B + 1)
    assert sess.mode == StepMode() and sess.step_fn is None and sess.hooks is None
    for name in FEATURE:                                          # nothing is allocated for an option that is off
        assert getattr(sess, name) is None, name
    # what a plain generate never reads keeps what it held: the sampling key, the prompt history
    assert ints(sess.batch_row0) == [7] * B and ints(sess.hist_len) == [7] * B


def test_begin_fills_the_mode_table_up_to_the_calls_steps(sess):
    dirty(sess)
    sess.begin(GenOptions(), n_steps=3, schedule=["e", "e", "e", "e", "e"])       # the schedule is cut at the call's max_new_tokens
    assert ints(sess.mode_table) == [3, 3, 3, 0, 7, 7, 7]


def test_add_batch_writes_its_own_rows(sess):
    o = GenOptions()
    sess.begin(o)
    sess.add_batch(o, 0, 0, [0, 4, 8], [5, 9], [11, 13])
    assert ints(sess.vrt_off) == [0, 4, 8, 8, 8]                  # rows not yet in use: an empty VRT range behind the batch's
    assert ints(sess.unfinished) == [1, 1, 0, 0]
    assert ints(sess.slot) == [5, 9, 0, 0] and ints(sess.lens) == [6, 10, 1, 1]
    assert ints(sess.pos3) == [[11, 13, 0, 0]] * 3
    sess.add_batch(o, 2, 8, [0, 4, 8], [3, 7], [4, 21])
    assert ints(sess.vrt_off) == [0, 4, 8, 12, 16]
    assert ints(sess.unfinished) == [1, 1, 1, 1]
    assert ints(sess.slot) == [5, 9, 3, 7] and ints(sess.lens) == [6, 10, 4, 8]
    assert ints(sess.pos3) == [[11, 13, 4, 21]] * 3
    assert ints(sess.step) == [0] and ints(sess.cur_tok) == [sess.cfg.pad_token_id] * B


def test_add_batch_with_the_options_on(sess):
    cfg = sess.cfg
    V = cfg.vocab_size
    o = all_on(cfg, min_tokens=None)                              # per-row minima: the options carry no single value
    sess.begin(o, p_max=4)
    assert ints(sess.batch_row0) == [0] * B
    first = dict(stop=dict(min_tokens=[2, 0], max_tokens=[3, 6]), counts=dict(frequency_penalty=[0.5, 0.0], presence_penalty=[0.25, 0.0], patch_suppression=None),
                 count_grids=[(2, 2), (2, 2)], patch_bias=[None, None])
    sess.add_batch(o, 0, 0, [0, 4, 8], [5, 9], [11, 13], prompt_ids=torch.tensor([[1, V + 3, 2], [0, 0, V]]),
                   forced=torch.tensor([[V + 1]], dtype=torch.int32).expand(2, 1), **first)
    assert ints(sess.max_tok) == [3, 6, T_MAX, T_MAX] and ints(sess.min_tok) == [2, 0, 0, 0]       # unfilled rows: the budget of begin()
    assert ints(sess.hist[:2, :3]) == [[1, V + 3, 2], [0, 0, V]] and ints(sess.forced[:2, :2]) == [[V + 1, -1]] * 2       # proto_row0 0: no shift
    assert ints(sess.cradius) == [-1] * B and ints(sess.batch_row0) == [0] * B
    assert not bool(sess.bias[V:].any())                          # a row without an entry adds 0
    # the second batch: its VRT ids (>= vocab) move by its first prototype row, text ids stay
    pb = [torch.tensor([[1.0, 2.0], [3.0, 4.0]]), None]
    sess.add_batch(o, 2, 8, [0, 4, 8], [3, 7], [4, 21], prompt_ids=torch.tensor([[1, 2, V + 1, 3], [V + 7, 0, 0, V - 1]]),
                   forced=torch.tensor([[V + 2, 5, -1], [-1, V, 3]], dtype=torch.int32), stop=dict(min_tokens=[1, 2], max_tokens=None),
                   counts=dict(frequency_penalty=[0.5, 0.25], presence_penalty=None, patch_suppression=[(1, 2.0), None]),
                   count_grids=[(2, 2), (0, 0)], patch_bias=pb)
    assert ints(sess.hist[2:, :4]) == [[1, 2, V + 9, 3], [V + 15, 0, 0, V - 1]]
    assert ints(sess.hist_len) == [3, 3, 4, 4]                    # each batch's padded prompt length
    assert ints(sess.forced[2:]) == [[V + 10, 5, -1, -1, -1, -1], [-1, V + 8, 3, -1, -1, -1]]     # steps past the table's width stay free
    assert ints(sess.min_tok) == [2, 0, 1, 2] and ints(sess.max_tok) == [3, 6, NO_BUDGET, NO_BUDGET]
    assert ints(sess.cpen) == [[0.5, 0.0, 0.5, 0.25], [0.25, 0.0, 0.0, 0.0], [0.0, 0.0, 2.0, 0.0]]
    assert ints(sess.cgrid) == [[2, 2], [2, 2], [2, 2], [0, 0]] and ints(sess.cradius) == [-1, -1, 1, -1]
    assert ints(sess.batch_row0) == [0, 0, 2, 2]
    assert ints(sess.bias[V + 8: V + 16]) == [1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0]      # its segment at vocab + 8, zeros for the row without an entry
    assert not bool(sess.bias[V: V + 8].any())
    assert ints(sess.bias[[1, 7]]) == [0.5, -1.0] and float(sess.bias[:V].abs().sum()) == 1.5      # the call's logit_bias, from begin()
    # the first batch's rows are as it left them
    assert ints(sess.hist[:2, :3]) == [[1, V + 3, 2], [0, 0, V]] and ints(sess.forced[:2]) == [[V + 1, -1, -1, -1, -1, -1]] * 2


def test_a_second_begin_resets_what_the_first_generate_left_and_keeps_every_address(sess):
    cfg = sess.cfg
    o = all_on(cfg)
    wider = dataclasses.replace(o, top_logprobs=5)
    sess.begin(o, p_max=4)
    owned = [n for n in FEATURE if isinstance(getattr(sess, n), torch.Tensor) and n not in ("top_idx", "top_val", "summary_stop_host")]
    assert {"part_sum", "logprobs", "patch_lp", "topk_ws", "forced", "probe_val", "bias", "decay", "stab", "min_tok", "max_tok", "finish_step",
            "finish_reason", "stop_index", "sban", "summary_stop", "cnt_text", "cnt_patch", "near", "cpen", "cgrid", "cradius"} <= set(owned)
    ptr = {n: getattr(sess, n).data_ptr() for n in owned}
    flat = [f.data_ptr() for f in sess.top_flat]
    assert tuple(sess.top_idx.shape) == (B, T_MAX, 3) and sess.top_idx.data_ptr() == flat[0] and sess.top_val.data_ptr() == flat[1]
    assert sess.top_flat[0].numel() == B * T_MAX * ops.TOPK_ROWS_MAX_K
    dirty(sess)                                                   # what a generate leaves behind
    sentinels = {StepMode(): "plain", StepMode(patches=True): "patches", StepMode(patches=True, top_k=True): "both", StepMode(top_k=True): "top"}
    sess.graphs = dict(sentinels)
    sess.begin(wider, p_max=4)
    assert sess.graphs == sentinels                               # the patch buffer is wide enough: every captured graph stays
    assert {n: getattr(sess, n).data_ptr() for n in owned} == ptr and [f.data_ptr() for f in sess.top_flat] == flat
    assert tuple(sess.top_idx.shape) == (B, T_MAX, 5) and sess.top_idx.data_ptr() == flat[0] and sess.top_val.data_ptr() == flat[1]
    assert bool((sess.top_idx == -1).all()) and bool((sess.top_val == float("-inf")).all()) and bool((sess.patch_lp == float("-inf")).all())
    assert bool((sess.forced == -1).all()) and not bool(sess.logprobs.any()) and not bool(sess.part_sum.any())
    for n in ("cnt_text", "cnt_patch", "near"):
        assert int(ops.count_values(getattr(sess, n)).sum()) == 0, n
    assert not bool(sess.cpen.any()) and not bool(sess.cgrid.any()) and ints(sess.cradius) == [-1] * B
    assert ints(sess.finish_step) == [-1] * B and ints(sess.finish_reason) == [0] * B and ints(sess.stop_index) == [-1] * B
    assert ints(sess.min_tok) == [1] * B and ints(sess.max_tok) == [T_MAX] * B and ints(sess.hist_len) == [0] * B
    assert ints(sess.bias[[1, 7]]) == [0.5, -1.0] and float(sess.bias.abs().sum()) == 1.5
    # a wider sample: the patch buffer is reallocated, and exactly the graphs captured over the smaller one go
    sess.begin(wider, p_max=9)
    assert sess.graphs == {m: v for m, v in sentinels.items() if not m.patches} and len(sess.graphs) == 2
    assert tuple(sess.patch_lp.shape) == (B, T_MAX, 9) and sess.p_cap == 9 and bool((sess.patch_lp == float("-inf")).all())
    assert {n: getattr(sess, n).data_ptr() for n in owned if n != "patch_lp"} == {n: p for n, p in ptr.items() if n != "patch_lp"}


def test_begin_with_an_automaton_resets_its_row_states(sess):
    from padt_amd.generation import TokenAutomaton
    trie = TokenAutomaton.from_sequences([[1, 2, TokenAutomaton.VRT], [1, 3]], repeat=True)
    o = GenOptions(automaton=trie.key)
    sess.begin(o, automaton=trie)
    assert ints(sess.astate) == [[-1, -1]] * B and sess.atab.numel() == ops.TOKEN_AUTOMATON_INTS and sess.aban.shape == sess.ban.shape
    tab = ops.token_automaton_tensor(trie)
    assert torch.equal(sess.atab[: tab.numel()], tab)
    ptr = (sess.atab.data_ptr(), sess.astate.data_ptr(), sess.aban.data_ptr())
    sess.astate.fill_(3)
    sess.begin(o, automaton=trie)
    assert ints(sess.astate) == [[-1, -1]] * B and (sess.atab.data_ptr(), sess.astate.data_ptr(), sess.aban.data_ptr()) == ptr
    sess.begin(GenOptions())                                      # off again: the buffers stay where they are, the step no longer reads them
    assert not sess.mode.automaton and sess.atab.data_ptr() == ptr[0]
