"""generate(stop_sequences=, min_tokens=, max_tokens=) on the device.

Kernel level: padt_stop_ban against generation.stop_ban_ids bit for bit (then both operand twins of the ban head on its bitmap), and
padt_stop_match against generation.stop_state on the hand-written rows of stop_rules_util, launch after launch, all outputs between guard words.

End to end, on the small synthetic model and the two ragged samples of the other generate suites: the three arguments inside the captured
step (and kernel by kernel) against the HOOKED loop running HF's MinNewTokensLengthLogitsProcessor and a stopping criterion written from
stop_state — sequences, score rows, hidden rows bit for bit, token log-probs within test_token_logprobs_gpu.within of fp64 log_softmax of the
reference's rows, the finish fields equal to stop_scan over the reference's tokens.  Stop sequences are taken from a free run's own output, so
the stop point is known by construction.  Without the feature this module does not import (the specification functions are missing), and
generate() refuses the three keywords as unknown arguments."""
import types

import pytest
import torch

import stop_rules_util as S
import test_score_bias_gpu as SB
import test_token_logprobs_gpu as TL
from padt_amd.generation import NO_BUDGET, StepMode, stop_ban_ids, stop_scan, stop_table

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD, GUARD_WORD = 4, 0x5A5A5A5A
T_NEW = 12
i32 = TL.i32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def guarded_i32(n, fill):
    """n int32 words set to `fill` between two runs of guard words → (flat, view)"""
    flat = torch.full((2 * GUARD + n,), GUARD_WORD, dtype=torch.int32, device="cuda")
    view = flat[GUARD: GUARD + n]
    view.fill_(fill)
    return flat, view


def guards_ok(flat):
    return bool((flat[:GUARD] == GUARD_WORD).all()) and bool((flat[-GUARD:] == GUARD_WORD).all())


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ the ban kernel
BAN_V, BAN_COUNTS = 96, (6, 4, 7)
BAN_COLS = BAN_V + sum(BAN_COUNTS)           # 113: four bitmap words, the last one partly used
BAN_WORDS = (BAN_COLS + 31) // 32
BAN_EOS, BAN_LIST = 37, (41, 112, 200, -1)   # 112: the last column; 200: outside the table, sets nothing
BAN_MIN = [0, 2, 5]


def want_ban_words(step, incoming):
    want = incoming.clone().to(torch.int64) & 0xFFFFFFFF if incoming is not None else torch.zeros(3, BAN_WORDS, dtype=torch.int64)
    for b, n in enumerate(BAN_MIN):
        for e in stop_ban_ids(step, n, (BAN_EOS,) + BAN_LIST):
            if e < BAN_COLS:
                want[b, e >> 5] |= 1 << (e & 31)
    return want


@pytest.mark.parametrize("incoming", [False, True], ids=["zeros", "incoming bitmap"])
def test_ban_kernel_is_stop_ban_ids(ops, incoming):
    assert BAN_COLS == 113 and BAN_WORDS == 4
    g = torch.Generator().manual_seed(5)
    cfg = ops.gen_cfg_tensor(1.0, BAN_LIST[:3], "cuda")
    mins = i32(BAN_MIN)
    seen_on = seen_off = 0
    for step in (0, 1, 2, 4, 5):
        inc = None
        if incoming:
            inc = torch.randint(-2 ** 31, 2 ** 31 - 1, (3, BAN_WORDS), generator=g, dtype=torch.int64).to(torch.int32)
            inc[:, -1] &= (1 << (BAN_COLS & 31)) - 1                    # as padt_gen_rules leaves it: no bit past the table
            inc[:, BAN_EOS >> 5] &= ~(1 << (BAN_EOS & 31))               # ... and the config EOS not banned by the rules themselves
        flat, out = guarded_i32(3 * BAN_WORDS, -1)                      # every bit set: the kernel writes the rows from scratch
        out = out.view(3, BAN_WORDS)
        got = ops.stop_ban(cfg, BAN_EOS, i32([step]), mins, out, BAN_COLS, ban_in=None if inc is None else inc.cuda())
        assert got is out and guards_ok(flat)
        want = want_ban_words(step, inc)
        assert torch.equal(out.cpu().to(torch.int64) & 0xFFFFFFFF, want), step
        for b, n in enumerate(BAN_MIN):
            on = bool((want[b, BAN_EOS >> 5] >> (BAN_EOS & 31)) & 1)
            assert on == (step < n)
            seen_on, seen_off = seen_on + on, seen_off + (not on)
    assert seen_on and seen_off


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_head_writes_minus_inf_exactly_where_the_ban_kernel_says(ops, dt):
    from test_gen_rules_gpu import _head
    g = torch.Generator().manual_seed(11)
    D = 256
    E = torch.randn(BAN_V, D, generator=g).to(dt).cuda()
    P = torch.randn(sum(BAN_COUNTS), D, generator=g).to(dt).cuda()
    h = torch.randn(3, D, generator=g).to(dt).cuda()
    off = i32([0, 6, 10, 17])
    cfg = ops.gen_cfg_tensor(1.0, BAN_LIST[:3], "cuda")
    _, _, plain = _head(ops, h, E, P, off, packed=False)
    for step in (1, 5):
        ban = ops.stop_ban(cfg, BAN_EOS, i32([step]), i32(BAN_MIN), torch.full((3, BAN_WORDS), -1, dtype=torch.int32, device="cuda"), BAN_COLS)
        banned = torch.zeros(3, BAN_COLS, dtype=torch.bool)
        for b, n in enumerate(BAN_MIN):
            banned[b, [e for e in stop_ban_ids(step, n, (BAN_EOS,) + BAN_LIST) if e < BAN_COLS]] = True
        assert bool(banned.any()) == (step < max(BAN_MIN))
        want = torch.where(banned.cuda(), torch.full_like(plain, -INF), plain)
        for packed in (False, True):
            pv, pi, lg = _head(ops, h, E, P, off, packed=packed, ban=ban)
            assert torch.equal(bits(lg), bits(want)), (step, packed)


# ------------------------------------------------------------------------------------------------------------ the matcher
class Matcher:
    def __init__(self, ops):
        self.ops = ops
        B = len(S.ROWS)
        self.table = stop_table(S.SEQS).cuda()
        self.cfg = ops.gen_cfg_tensor(1.0, S.EOS_LIST, "cuda")
        self.tokens = torch.tensor([r.tokens for r in S.ROWS], dtype=torch.int64).cuda()
        self.tokens0 = self.tokens.clone()
        self.mins, self.maxs = i32([r.min_tokens for r in S.ROWS]), i32([r.max_tokens for r in S.ROWS])
        self.state = S.initial_state()
        self.flats, self.dev = [], []
        for vals in self.state:                                       # unfinished, finish_step, finish_reason, stop_index
            flat, view = guarded_i32(B, 0)
            view.copy_(torch.tensor(vals, dtype=torch.int32))
            self.flats.append(flat), self.dev.append(view)
        self.step = i32([0])

    def launch(self, n):
        self.step.fill_(n)
        unf, fstep, reason, index = self.dev
        self.ops.stop_match(self.table, self.cfg, S.CFG_EOS, self.tokens, self.step, self.mins, self.maxs, unf, fstep, reason, index)

    def check(self, n):
        for name, dev, want, flat in zip(("unfinished", "finish_step", "finish_reason", "stop_index"), self.dev, self.state, self.flats):
            assert dev.tolist() == want, f"*step = {n}: {name} {dev.tolist()} != {want}"
            assert guards_ok(flat), f"*step = {n}: a guard word of {name} was written"
        assert torch.equal(self.tokens, self.tokens0), "the token buffer was written"


def test_matcher_is_stop_state_launch_after_launch(ops):
    m = Matcher(ops)
    assert m.tokens.shape == (8, S.T_MAX) and len(S.SEQS[-1]) == 32
    m.launch(0)                                                       # no token yet: nothing happens
    m.check(0)
    for n in range(1, S.T_MAX + 1):
        m.launch(n)
        S.simulate(n, m.state)
        m.check(n)
        m.launch(n)                                                   # a repeated launch finds every finish recorded
        m.check(n)
    unf, step, reason, index = m.state
    assert [(s, r, i) for s, r, i in zip(step, reason, index)] == [(r.want[0], S.REASON_CODE[r.want[1]], r.want[2]) for r in S.ROWS]
    # past the token buffer: nothing happens, even for rows made live again
    for view, v in zip(m.dev, (1, -1, 0, -1)):
        view.fill_(v)
    m.launch(S.T_MAX + 1)
    assert [d.tolist() for d in m.dev] == [[1] * 8, [-1] * 8, [0] * 8, [-1] * 8] and all(guards_ok(f) for f in m.flats)
    # a table that is not the packer's writes nothing
    bad = m.table.clone()
    bad[0] = 0
    m.table = bad
    m.launch(3)
    assert [d.tolist() for d in m.dev] == [[1] * 8, [-1] * 8, [0] * 8, [-1] * 8]


def test_collect_summary_stop_is_collect_summary_and_the_finish_arrays(ops):
    n_rows, n_batch, t_max, done, eos = 5, 2, 9, 6, 7
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, 12, (n_rows, t_max), generator=g).cuda()
    err, unf, nf_rows, nf_batch = i32([0]), i32([0, 1, 0, 0, 1]), i32([0, 0, 3, 0, 0]), i32([0, 1, 9])
    cfg = ops.gen_cfg_tensor(1.0, (9, 3), "cuda")
    fs, fr, si = i32([2, -1, 0, 5, -1]), i32([1, 0, 2, 3, 0]), i32([-1, -1, 4, -1, -1])
    base = torch.full((2 + 2 * n_rows + n_batch,), -7, dtype=torch.int32, device="cuda")
    ops.collect_summary(err, unf, nf_rows, nf_batch, n_batch, tok, done, eos, cfg, base)
    flat, out = guarded_i32(2 + 5 * n_rows + n_batch, -7)
    ops.collect_summary_stop(err, unf, nf_rows, nf_batch, n_batch, tok, done, eos, cfg, fs, fr, si, out)
    assert guards_ok(flat)
    assert out[: base.numel()].tolist() == base.tolist()
    assert out[base.numel():].tolist() == fs.tolist() + fr.tolist() + si.tolist()


# ------------------------------------------------------------------------------------------------------------ end to end
# What every call below shares, the free run included.  The synthetic model left alone repeats one patch token per row (its patch logits
# are near 200, its text logits below 4), so a run with distinct TEXT tokens — something a stop sequence can be cut from — needs the text-only
# schedule of the other suites and a repetition penalty; both are on both sides of every comparison.
BASE = dict(schedule=["t"] * T_NEW, repetition_penalty=2.0)


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model()
    kw = TL.two_ragged(cfg, U)
    L = kw["input_ids"].shape[1]
    free = model.generate(max_new_tokens=T_NEW, output_scores=True, **BASE, **kw)
    e = types.SimpleNamespace(cfg=cfg, U=U, model=model, kw=kw, L=L, sess=free.past_key_values, free=free,
                              tok=free.sequences[:, L:].cpu().tolist(), eos=[int(cfg.eos_token_id)])
    print(f"\n[stop rules] free run {e.tok}")
    assert all(len(set(r)) == T_NEW and max(r) < cfg.vocab_size and not {int(cfg.eos_token_id), int(cfg.pad_token_id)} & set(r) for r in e.tok), \
        "precondition: the free run ends no row before max_new_tokens and its rows are distinct text tokens"
    return e


def per_row(v, B, default):
    return [default] * B if v is None else ([v] * B if isinstance(v, int) else list(v))


def device(e, **gen):
    out = e.model.generate(**dict(dict(BASE, max_new_tokens=T_NEW), **gen), **e.kw)
    out["step_mode"] = out.past_key_values.mode
    return out


def hooked(e, stop_sequences=None, min_tokens=None, max_tokens=None, logits_processor=(), **gen):
    """the twin on the hooked loop: HF's MinNewTokensLengthLogitsProcessor and a criterion written from stop_state instead of the three arguments"""
    B = e.kw["input_ids"].shape[0]
    eos = tuple(dict.fromkeys([int(e.cfg.eos_token_id)] + [int(x) for x in gen.get("eos_token_id", e.eos)]))
    mins, maxs = per_row(min_tokens, B, 0), per_row(max_tokens, B, None)
    procs = [S.min_new_tokens_processor(e.L, mins, eos)] + list(logits_processor)
    crit = S.criteria_from_stop_state(e.L, stop_sequences, mins, maxs, eos)
    out = e.model.generate(**dict(dict(BASE, max_new_tokens=T_NEW, output_scores=True), **gen), logits_processor=procs, stopping_criteria=[crit],
                           **e.kw)
    assert out.past_key_values.mode.processors and not out.past_key_values.mode.stop and "finish_reason" not in out
    return out


def compare(e, dev, ref, stop_sequences=None, min_tokens=None, max_tokens=None, scores=True, eos=None, tag=""):
    """→ the finish fields.  Sequences, hidden rows and live score rows bit for bit; token log-probs of both against fp64 log_softmax of the
    reference's rows; the finish fields against stop_scan over the reference's own tokens."""
    L, B = e.L, e.kw["input_ids"].shape[0]
    eos = tuple(dict.fromkeys([int(e.cfg.eos_token_id)] + [int(x) for x in (eos or e.eos)]))
    tok, rtok = dev.sequences[:, L:].cpu(), ref.sequences[:, L:].cpu()
    print(f"\n[{tag}] device {tok.tolist()}\n[{tag}] hooked {rtok.tolist()}")
    assert dev["step_mode"].stop
    assert torch.equal(dev.sequences, ref.sequences), "sequences differ"
    assert torch.equal(SB.hidden_bits(dev), SB.hidden_bits(ref)), "hidden rows differ"
    T = tok.shape[1]
    mins, maxs = per_row(min_tokens, B, 0), per_row(max_tokens, B, NO_BUDGET)
    want = [stop_scan(rtok[b].tolist(), stop_sequences, mins[b], maxs[b], eos) for b in range(B)]
    got = list(zip(dev.finish_step, dev.finish_reason, dev.stop_index))
    print(f"[{tag}] finish {got}")
    assert got == want, (got, want)
    assert T == (max(w[0] for w in want) + 1 if all(w[0] >= 0 for w in want) else T_NEW)
    live = torch.tensor([[w[0] < 0 or t <= w[0] for t in range(T)] for w in want])
    rv = torch.stack([x.cpu() for x in ref.scores], 1)
    assert not bool(torch.isnan(rv[live]).any())
    for b in range(B):                                                # the ban itself: every EOS column of a live row below its minimum
        for t in range(min(mins[b], T)):
            if live[b, t]:
                assert bool((rv[b, t, list(eos)] == -INF).all()), (b, t)
    if scores:
        dv = torch.stack([x.cpu() for x in dev.scores], 1)
        assert torch.equal(bits(dv[live]), bits(rv[live])), "live score rows differ from the hooked twin"
    if dev.token_logprobs is not None:
        ref_lp = TL.ref_logprob(rv[live], tok[live])
        for name, out in (("device", dev), ("hooked", ref)):
            lp = out.token_logprobs.cpu()
            assert tuple(lp.shape) == (B, T) and bool((lp[~live] == 0.0).all()), f"{name}: steps after a row's finish must hold 0.0"
            print(f"[{tag}] {name}: largest |token_logprobs - fp64| {TL.within(lp[live], ref_lp):.3e}")
    return want


def text_window(e, b, j, m):
    w = e.tok[b][j: j + m]
    ok = len(w) == m and all(0 <= x < e.cfg.vocab_size and x not in (e.cfg.eos_token_id, e.cfg.pad_token_id) for x in w)
    return w if ok else None


def pick_window(e, b, m):
    """tokens j .. j + m of row b of the free run that do not occur earlier in that row: the largest such j <= 4"""
    row = e.tok[b]
    for j in range(4, -1, -1):
        w = text_window(e, b, j, m)
        if w is not None and all(row[i: i + m] != w for i in range(j)):
            return j, w
    raise AssertionError(f"precondition: row {b} of the free run has no window of {m} text tokens that is new where it stands: {row}")


def test_plain_call_launches_what_it_launched(monkeypatch):
    """Without the three arguments: the parent's step mode, none of the new kernels, none of the new fields, no new buffer."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops
    cfg, U, model = TL.small_model()
    kw = TL.two_ragged(cfg, U)
    calls = []
    for name in ("stop_ban", "stop_match", "collect_summary_stop"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=getattr(ops, name), **k: (calls.append(_n), _f(*a, **k))[1])
    plain = model.generate(max_new_tokens=6, use_graph=False, **kw)
    sess = plain.past_key_values
    assert calls == [] and sess.mode == StepMode() and sess.stab is None and sess.sban is None
    assert not {"finish_reason", "stop_index", "finish_step"} & set(plain)
    on = model.generate(max_new_tokens=6, use_graph=False, max_tokens=6, **kw)      # a budget nobody reaches early: the same run, recorded
    assert on.past_key_values.mode == StepMode(stop=True) and torch.equal(on.sequences, plain.sequences)
    assert calls.count("stop_ban") == calls.count("stop_match") == 6 and calls.count("collect_summary_stop") >= 1
    assert on.finish_reason == ["length", "length"] and on.finish_step == [5, 5] and on.stop_index == [-1, -1]
    again = model.generate(max_new_tokens=6, use_graph=False, **kw)
    assert again.past_key_values.mode == StepMode() and "finish_reason" not in again and torch.equal(again.sequences, plain.sequences)


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_stop_sequences_from_the_free_runs_own_output(E, m, use_graph):
    e = E
    picks = [pick_window(e, b, m) for b in range(2)]
    seqs = [w for _, w in picks]
    want = [stop_scan(e.tok[b], seqs, 0, NO_BUDGET, e.eos) for b in range(2)]      # the other row's sequence may end a row earlier
    for b, (j, w) in enumerate(picks):
        assert want[b][1] == "stop" and want[b][0] <= j + m - 1
    assert any(want[b][0] == picks[b][0] + m - 1 and want[b][2] == b for b in range(2))
    dev = device(e, stop_sequences=seqs, output_scores=True, use_graph=use_graph)
    ref = hooked(e, stop_sequences=seqs)
    got = compare(e, dev, ref, stop_sequences=seqs, tag=f"stop m={m}")
    assert got == want
    L = e.L
    for b in range(2):                                                # the sequence's tokens stay in the output; the prompt is never matched
        n = want[b][0] + 1
        assert dev.sequences[b, L: L + n].tolist() == e.tok[b][:n]
        assert bool((dev.sequences[b, L + n:] == e.cfg.pad_token_id).all())


def test_a_sequence_that_ends_the_prompt_is_not_matched(E):
    """[the prompt's last token, the row's first generated token] would complete at the first step if the prompt were matched"""
    e = E
    last = [int(x) for x in e.kw["input_ids"][:, -1].tolist()]
    assert all(0 <= x < e.cfg.vocab_size for x in last) and all(text_window(e, b, 0, 1) for b in range(2))
    seqs = [[last[b], e.tok[b][0]] for b in range(2)]
    want = [stop_scan(e.tok[b], seqs, 0, 5, e.eos) for b in range(2)]
    assert all(w[0] >= 1 for w in want)                               # two ids need two generated tokens
    dev = device(e, stop_sequences=seqs, max_tokens=5)
    assert list(zip(dev.finish_step, dev.finish_reason, dev.stop_index)) == want


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "eager"])
def test_min_tokens_puts_the_first_eos_at_its_index(E, use_graph):
    e = E
    eos = int(e.cfg.eos_token_id)
    lb = {eos: 60.0}
    now = device(e, logit_bias=lb)
    assert now.sequences[:, e.L].tolist() == [eos, eos] and now.sequences.shape[1] == e.L + 1, "precondition: the bias makes EOS the arg-max from step 0"
    dev = device(e, logit_bias=lb, min_tokens=3, output_scores=True, output_token_logprobs=True, use_graph=use_graph)
    ref = hooked(e, min_tokens=3, logit_bias=lb, output_token_logprobs=True)
    got = compare(e, dev, ref, min_tokens=3, tag="min_tokens")
    assert got == [(3, "eos", -1)] * 2
    assert dev.sequences[:, e.L: e.L + 3].tolist() == [r[:3] for r in e.tok] and dev.sequences[:, e.L + 3].tolist() == [eos, eos]
    per = device(e, logit_bias=lb, min_tokens=[1, 4], use_graph=use_graph)
    assert per.finish_step == [1, 4] and per.finish_reason == ["eos", "eos"] and per.sequences.shape[1] == e.L + 5


def common(e):
    """EOS is the arg-max wherever it is allowed; row 0 may end from its fourth token on, row 1 from its second — where a stop sequence
    taken from the free run waits"""
    a = text_window(e, 1, 1, 1)
    assert a is not None, "precondition: row 1's second free token is a text id"
    return dict(logit_bias={int(e.cfg.eos_token_id): 60.0}, min_tokens=[3, 2], stop_sequences=[a], max_tokens=[T_NEW, 9])


def mode_cases(e):
    import token_automaton_util as TA
    from test_token_automaton_gpu import LABELS
    eos = int(e.cfg.eos_token_id)
    first = int(e.tok[0][0])

    def push_down(input_ids, scores):                                 # a caller's processor that changes the run: row 0's first free token pushed down
        out = scores.clone()
        out[:, first] -= 20.0
        return out
    return {
        "greedy": (dict(), dict()),
        "token_logprobs": (dict(output_token_logprobs=True), dict(scores=False)),
        "sampling": (dict(do_sample=True, temperature=0.8, top_k=30, top_p=0.95, seed=13, output_token_logprobs=True), dict()),
        "logits_processor": (dict(logits_processor=[push_down]), dict()),
        "forced_eos_below_min_tokens": (dict(forced_tokens=[[-1, eos], [-1, -1, -1]], output_token_logprobs=True, min_tokens=4, max_tokens=[6, 6]), dict()),
        "no_repeat_ngram": (dict(no_repeat_ngram_size=1), dict()),
        # without the text-only schedule: the labels are followed by the rows' own patches
        "token_automaton": (dict(token_automaton=TA.label_automaton(LABELS, repeat=True), min_tokens=[4, 2], schedule=None), dict()),
    }


MODES = ("greedy", "token_logprobs", "sampling", "logits_processor", "forced_eos_below_min_tokens", "no_repeat_ngram", "token_automaton")


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("mode", MODES)
def test_modes_equal_the_hooked_loop(E, mode, use_graph):
    e = E
    extra, how = mode_cases(e)[mode]
    args = dict(common(e), **extra)
    three = {k: args[k] for k in ("stop_sequences", "min_tokens", "max_tokens")}
    scores = how.get("scores", True)
    dev = device(e, output_scores=scores, use_graph=use_graph, **args)
    ref = hooked(e, **args)
    got = compare(e, dev, ref, scores=scores, tag=mode, **three)
    assert dev["step_mode"].processors == (mode == "logits_processor")
    if not scores:
        assert dev.scores is None
    if mode == "greedy":                                              # by construction: row 0 its EOS at index 3 at the latest, row 1 the sequence at index 1
        assert got[1] == (1, "stop", 0) and got[0][0] <= 3 and got[0][1] in ("eos", "stop")
    if mode == "forced_eos_below_min_tokens":
        assert got[0] == (1, "eos", -1) and float(dev.token_logprobs[0, 1]) == -INF, "a forced EOS wins, with log-prob -inf"
        assert got[1][0] <= 5
    if mode == "no_repeat_ngram":                                     # the union: a generated token's column and the EOS column are both -inf
        row = dev.scores[1][0].cpu()
        assert row[int(dev.sequences[0, e.L])] == -INF and row[int(e.cfg.eos_token_id)] == -INF


def test_criteria_on_the_hooked_loop_are_recorded_as_criteria(E):
    e = E

    def after_three(input_ids, scores):
        return torch.tensor([input_ids.shape[1] - e.L >= 3, False], device=input_ids.device)
    out = device(e, stopping_criteria=[after_three], max_tokens=[T_NEW, 5])
    assert out.finish_reason == ["criteria", "length"] and out.finish_step == [2, 4] and out.stop_index == [-1, -1]
    assert out.sequences.shape[1] == e.L + 5 and out.sequences[0, e.L: e.L + 3].tolist() == e.tok[0][:3]


def test_exact_trimming_with_a_late_sync(E):
    """sync_every=8: nine tokens are generated before the host first looks; every row ended at token 3, so four columns come back."""
    e = E
    by_budget = device(e, max_tokens=4, sync_every=8)
    assert by_budget.finish_step == [3, 3] and by_budget.finish_reason == ["length"] * 2 and by_budget.sequences.shape[1] == e.L + 4
    assert int(by_budget.past_key_values.step.item()) == 9, "precondition: the loop ran past the rows' end before the host looked"
    assert by_budget.sequences[:, e.L:].tolist() == [r[:4] for r in e.tok]
    seqs = [e.tok[b][2:4] for b in range(2)]
    assert all(text_window(e, b, 2, 2) for b in range(2))
    want = [stop_scan(e.tok[b], seqs, 0, 4, e.eos) for b in range(2)]
    assert max(w[0] for w in want) == 3 and any(w[1] == "stop" for w in want), f"precondition: {want}"
    by_seq = device(e, stop_sequences=seqs, max_tokens=4, sync_every=8)
    assert list(zip(by_seq.finish_step, by_seq.finish_reason, by_seq.stop_index)) == want and by_seq.sequences.shape[1] == e.L + 4
    free = device(e, sync_every=8)
    assert free.sequences.shape[1] == e.L + T_NEW and "finish_step" not in free


def test_score_completions_with_ragged_budgets(E):
    e = E
    comp = [e.tok[0][:3], e.tok[1][:1]]
    plain = e.model.score_completions(e.kw["input_ids"], e.kw["attention_mask"], e.kw["pixel_values"], e.kw["image_grid_thw"], comp)
    assert "finish_reason" not in plain and plain.sequences.shape[1] == e.L + 3          # what it returns today: the short row runs free
    out = e.model.score_completions(e.kw["input_ids"], e.kw["attention_mask"], e.kw["pixel_values"], e.kw["image_grid_thw"], comp, max_tokens=[3, 1])
    assert out.finish_step == [2, 0] and out.finish_reason == ["length", "length"]
    assert bool((out.sequences[1, e.L + 1:] == e.cfg.pad_token_id).all()) and bool((out.token_logprobs[1, 1:] == 0.0).all())
    assert torch.equal(bits(out.completion_logprobs), bits(plain.completion_logprobs))


def test_bf16_rerun_keeps_the_three_arguments():
    """operands="auto": a batch whose SwiGLU hidden exceeds fp16's range is re-run on the bf16 twin WITH the sequences, the minimum and the
    per-row budgets — the result is the bf16 model's own run under them (the weight edit is test_range_guard_gpu.py's `llm_swiglu` case)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    w = U.bf16_weights(cfg, seed=21, std=0.05)
    for name, idx, val in (("model.layers.0.self_attn.o_proj.weight", (7, slice(None)), 8192.0), ("model.layers.1.mlp.gate_proj.weight", (3, 7), 32.0),
                           ("model.layers.1.mlp.up_proj.weight", (3, 7), 32.0)):
        w[name] = w[name].clone()
        w[name][idx] = val
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8], [1, 10, 12]], n_pre=5, n_post=8, ragged=True, seed=41)
    kw = dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    L, gen = ids.shape[1], dict(BASE, max_new_tokens=T_NEW)
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16")
    tok = ref.generate(**gen, **kw).sequences[:, L:].cpu().tolist()
    assert all(max(r[:4]) < cfg.vocab_size for r in tok)
    three = dict(stop_sequences=[tok[0][2:4]], min_tokens=2, max_tokens=[9, 6])
    want = ref.generate(**three, **gen, **kw)
    assert want.finish_reason[0] == "stop" and want.finish_step[0] <= 3 and want.finish_step[1] <= 5
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(**three, **gen, **kw)
    assert auto.overflow_reruns == 1 and torch.equal(got.sequences, want.sequences)
    for name in ("finish_reason", "stop_index", "finish_step"):
        assert got[name] == want[name], name


def test_merged_group_with_per_row_budgets_equals_each_batch_alone():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import pipeline
    from test_generate_combinations_gpu import make_merged
    cfg, U, model, proc, batches = make_merged()
    budgets = ([3, 7], [5, 2], [6, 6])
    mins = ([0, 2], [1, 0], [0, 0])
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], max_new_tokens=8, max_tokens=mx, min_tokens=mn)
             for b, mx, mn in zip(batches, budgets, mins)]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b, mx, mn in zip(batches, budgets, mins):
        got += runner.submit(b[0].clone(), *b[1:], max_new_tokens=8, max_tokens=mx, min_tokens=mn)
    got += runner.flush()
    assert runner.n_groups == 2 and len(got) == 3, "per-row lists do not split a decode group"
    for i, ((d0, c0, l0, v0), (d1, c1, l1, v1)) in enumerate(zip(alone, got)):
        assert c0 == c1 and l0 == l1 and v0 == v1, f"batch {i}"
        for name in ("finish_reason", "stop_index", "finish_step"):
            assert d0[name] == d1[name], (i, name, d0[name], d1[name])
        assert all(0 <= s < mx for s, mx in zip(d0["finish_step"], budgets[i])), (i, d0["finish_step"])
        for name in ("pred_boxes", "pred_mask", "pred_score"):
            assert torch.equal(d0[name], d1[name]), f"batch {i}: {name}"
    print(f"\n[merged] finish {[(d['finish_step'], d['finish_reason']) for d, _, _, _ in got]}")
