"""generate(token_automaton=A) on the device.

Kernel level: padt_token_automaton's bitmap against `TokenAutomaton.allowed()` bit for bit (a 1003-column text table, patch ranges [0, 5),
[5, 5), [5, 42), EOS lists of 1 and 4 ids, random automata of ~40 states, histories of 0, 1, 2 and 70 tokens), idempotence, rebuild after an
invalidated state, the union with padt_gen_rules' bitmap, finished rows, malformed tables in a poisoned oversized buffer.
Convention for the bits past n_cols in the last word: zero.

End to end (the small synthetic model, three ragged samples): `generate(token_automaton=A)` — the new kernel inside the captured step —
against the SAME model with `allowed()` wrapped into HF's PrefixConstrainedLogitsProcessor as `logits_processor=[...]` on the hooked loop,
which does not run the new kernel: sequences and every live `.scores` row equal, in every mode the automaton is wired into."""
import types

import pytest
import torch

import token_automaton_util as T
from padt_amd.generation import TokenAutomaton as TA

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD, GUARD_WORD = 4, 0x5A5A5A5A
RANGES = list(zip(T.VRT_OFF[:-1], T.VRT_OFF[1:]))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------ the kernel
class Rows:
    """Device state of one padt_token_automaton problem over the three rows of token_automaton_util: the packed table followed by garbage
    slack, generation config, patch offsets, token buffer, step counter, stop state, state pairs, and a ban bitmap pre-filled with set bits
    between two runs of sentinel words."""

    def __init__(self, ops, A, eos, tokens, t, t_max=None, unfinished=(1, 1, 1), table=None):
        self.ops, B = ops, 3
        tab = ops.token_automaton_tensor(A) if table is None else table
        self.table = torch.cat([tab, torch.full((37,), 0x7F7F7F7F, dtype=torch.int32)]).cuda()
        self.gen_cfg = ops.gen_cfg_tensor(1.0, eos, "cuda")
        self.vrt_off = i32(T.VRT_OFF)
        t_max = t_max or max(max(len(tk) for tk in tokens), 1) + 2
        tok = torch.full((B, t_max), 3, dtype=torch.int64)                   # past the step counter: a text id (an over-read would walk on)
        for b, tk in enumerate(tokens):
            tok[b, : len(tk)] = torch.tensor(tk, dtype=torch.int64)
        self.tokens, self.step, self.unfinished = tok.cuda(), i32([t]), i32(list(unfinished))
        self.state = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
        self.flat = torch.full((2 * GUARD + B * T.WORDS,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.ban = self.flat[GUARD: GUARD + B * T.WORDS].view(B, T.WORDS)
        self.ban.fill_(-1)                                                   # every bit set: the kernel rebuilds the row from nothing

    def run(self, rules_ban=None):
        self.ops.token_automaton(self.table, self.gen_cfg, self.vrt_off, self.tokens, self.step, self.unfinished, self.state, self.ban, T.N_COLS,
                                 T.V, rules_ban=rules_ban)

    def guards_ok(self):
        return bool((self.flat[:GUARD] == GUARD_WORD).all()) and bool((self.flat[-GUARD:] == GUARD_WORD).all())

    def bitmap(self):
        got, tail_clear = T.bitmap_to_bool(self.ban, T.N_COLS)
        assert tail_clear, "bits past n_cols are set"
        assert self.guards_ok(), "sentinel words around ban overwritten"
        return got


def test_bitmap_equals_allowed_bit_for_bit(ops):
    """6 random automata x EOS lists of 1 / 4 ids x histories of 0, 1, 2, 70 tokens x the three rows: bitmap == allowed(), state == walk()"""
    n_off = n_big = n_vrt_only = 0
    for seed in range(6):
        eos = T.EOS_LISTS[seed % 2]
        A = T.random_automaton(seed, eos)
        for length in T.HISTORY_LENGTHS:
            hist = [T.random_history(100 * seed + b, A, length, RANGES[b], eos) for b in range(3)]
            r = Rows(ops, A, eos, hist, length)
            r.run()
            got, st = r.bitmap(), r.state.cpu().tolist()
            for b in range(3):
                want = T.ban_row(A, hist[b], RANGES[b], eos)
                diff = (got[b] != want).nonzero().flatten().tolist()
                assert not diff, (seed, length, b, diff[:10], hist[b][-3:])
                s = A.walk(hist[b], T.V, RANGES[b], eos)
                assert st[b] == [s, length]
                n_off += s == TA.OFF
                n_big += s == T.BIG_STATE
                n_vrt_only += s == T.VRT_ONLY_STATE
    assert n_off >= 3, "precondition: some histories leave the automaton"
    # the two special states directly: a history that ends in them, for every row (row 1 has no patches: VRT-only → EOS)
    for seed in range(2):
        eos = T.EOS_LISTS[seed]
        A = T.random_automaton(seed, eos)
        for target in (T.BIG_STATE, T.VRT_ONLY_STATE):
            B = TA(A.edges, start=target)
            r = Rows(ops, B, eos, [[], [], []], 0)
            r.run()
            got = r.bitmap()
            for b in range(3):
                assert torch.equal(got[b], T.ban_row(B, [], RANGES[b], eos)), (seed, target, b)
            if target == T.VRT_ONLY_STATE:
                assert (~got[1]).nonzero().flatten().tolist() == sorted(eos) and int((~got[2]).sum()) == 37 and int((~got[0]).sum()) == 5
            else:
                assert int((~got[0]).sum()) > 300


def test_second_launch_changes_nothing_and_a_rebuilt_state_is_the_advanced_one(ops):
    eos = T.EOS_LISTS[1]
    A = T.random_automaton(3, eos)
    n = 12
    hist = [T.random_history(40 + b, A, n, RANGES[b], eos) for b in range(3)]
    r = Rows(ops, A, eos, hist, 0, t_max=n + 2)
    for t in range(n + 1):                                                   # the decode loop: one launch per step, the state advanced by one token
        r.step.fill_(t)
        r.run()
        got, st = r.bitmap().clone(), r.state.clone()
        for b in range(3):
            assert torch.equal(got[b], T.ban_row(A, hist[b][:t], RANGES[b], eos)), (t, b)
            assert st[b].tolist() == [A.walk(hist[b][:t], T.V, RANGES[b], eos), t]
        r.ban.fill_(-1)
        r.run()                                                              # the same step again: idempotent
        assert torch.equal(r.bitmap(), got) and torch.equal(r.state, st)
        if t in (1, 5, n):                                                   # invalidated (reset, stale, from the future): rebuilt from the tokens
            for bad in ([-1, -1], [T.BIG_STATE, t - 3], [T.VRT_ONLY_STATE, t + 1]):
                r.state.copy_(i32([bad] * 3))
                r.ban.fill_(-1)
                r.run()
                assert torch.equal(r.bitmap(), got) and torch.equal(r.state, st), (t, bad)


def test_union_with_the_rules_bitmap_and_finished_rows(ops):
    eos = T.EOS_LISTS[0]
    # a wide state (any text, the own patches, five ids) and a narrow one: both bitmaps must have bits the other lacks
    A = TA([[(TA.TEXT, 0), (TA.VRT, 0), (TA.EOS, 2), (9, 1)], [(TA.VRT, 0)] + [(k, 0) for k in (0, 31, 32, 640, T.V - 1)], []])
    hist = [[5, 9], [9, 640], [5, 5]]
    g = torch.Generator().manual_seed(1)
    rules = torch.randint(-2 ** 31, 2 ** 31 - 1, (3, T.WORDS), generator=g, dtype=torch.int64).to(torch.int32)
    rules &= torch.randint(-2 ** 31, 2 ** 31 - 1, (3, T.WORDS), generator=g, dtype=torch.int64).to(torch.int32)     # about a quarter of the bits
    rules[:, -1] &= (1 << (T.N_COLS % 32)) - 1                               # what padt_gen_rules writes: nothing past n_cols
    rules_dev = rules.cuda()
    r = Rows(ops, A, eos, hist, 2, unfinished=(1, 1, 0))
    r.run(rules_ban=rules_dev)
    got = r.bitmap()
    rb, _ = T.bitmap_to_bool(rules, T.N_COLS)
    for b in range(2):
        own = T.ban_row(A, hist[b], RANGES[b], eos)
        assert torch.equal(got[b], own | rb[b]) and bool((own & ~rb[b]).any()), b
        assert b == 0 or bool((rb[b] & ~own).any())                          # (row 0's state allows ten columns only)
    assert torch.equal(got[2], rb[2])                                        # a finished row adds nothing of its own
    assert torch.equal(rules_dev.cpu(), rules)                               # the rules' buffer is read only
    # without rules a finished row bans nothing and keeps its state pair
    r = Rows(ops, A, eos, hist, 2, unfinished=(0, 1, 0))
    r.state.copy_(i32([[1, 1], [1, 1], [-1, -1]]))
    r.run()
    got = r.bitmap()
    assert not got[0].any() and not got[2].any() and got[1].any()
    assert r.state.cpu().tolist() == [[1, 1], [0, 2], [-1, -1]]                # row 1 advanced from state 1 by its last token, 640
    with pytest.raises(AssertionError):
        r.run(rules_ban=r.ban)                                               # two buffers are required
    with pytest.raises(AssertionError):
        ops.token_automaton(r.table, r.gen_cfg, r.vrt_off, r.tokens, r.step, r.unfinished, r.state, r.ban, T.WORDS * 32 + 1, T.V)


def test_malformed_table_writes_nothing_outside_the_row(ops):
    eos = T.EOS_LISTS[1]
    A = T.random_automaton(5, eos)
    good = ops.token_automaton_tensor(A)
    S, E = int(good[1]), int(good[2])
    hist = [T.random_history(60 + b, A, 2, RANGES[b], eos) for b in range(3)]
    # a header that is not the packer's: the kernel returns before its first write
    for idx, val in ((0, 0), (1, 0), (1, -5), (1, ops.TOKEN_AUTOMATON_MAX_STATES + 1), (2, -1), (2, ops.TOKEN_AUTOMATON_MAX_EDGES + 1),
                     (2, E + 64), (3, -1), (3, S), (1, S + 100)):
        bad = good.clone()
        bad[idx] = val
        r = Rows(ops, A, eos, hist, 2, table=bad)
        r.run()
        torch.cuda.synchronize()
        assert bool((r.ban == -1).all()) and r.guards_ok() and bool((r.state == -1).all()), (idx, val)
    # offsets or successors that leave the table: the row counts as off the automaton (EOS only); nothing outside the row is touched
    want_off = torch.ones(T.N_COLS, dtype=torch.bool)
    want_off[torch.tensor(sorted(eos))] = False
    s0 = A.start
    for what, idx, val in (("negative offset", 4 + s0, -7), ("offset past the edges", 4 + s0 + 1, E + 9), ("offsets reversed", 4 + s0, E),
                           ("huge offset", 4 + s0 + 1, 2 ** 31 - 1)):
        bad = good.clone()
        bad[idx] = val
        r = Rows(ops, A, eos, [[], [], []], 0, table=bad)
        r.run()
        got = r.bitmap()
        for b in range(3):
            assert torch.equal(got[b], want_off), (what, b)
    bad = good.clone()
    bad[5 + S + 1:: 2] = S + 3                                               # every successor outside the table
    r = Rows(ops, A, eos, hist, 2, table=bad)
    r.run()
    got = r.bitmap()
    for b in range(3):
        assert torch.equal(got[b], want_off) and r.state.cpu().tolist()[b] == [TA.OFF, 2]


# ------------------------------------------------------------------------------------------------------------ end to end
T_NEW = 16
LABELS = [[21, 22], [21, 23, 24], [31, 32]]
GRIDS = [[1, 10, 12], [1, 8, 8], [1, 6, 10]]


def batch3(cfg, U, seed=91, grids=GRIDS):
    grid, pix, ids, am = U.synthetic_batch(cfg, grids, n_pre=6, n_post=9, ragged=True, seed=seed)
    return dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)


def patch_ranges(grid, image_index=None):
    n = [int(g[1] * g[2]) // 4 for g in torch.as_tensor(grid).tolist()]
    if image_index is not None:
        n = [n[i] for i in image_index]
    off = [0]
    for x in n:
        off.append(off[-1] + x)
    return list(zip(off[:-1], off[1:]))


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_token_logprobs_gpu as TL
    cfg, U, model = TL.small_model()
    return cfg, U, model, batch3(cfg, U)


def hooked_twin(model, cfg, A, kw, **gen):
    """(device path, hooked twin): the automaton as an argument, and `allowed()` inside HF's PrefixConstrainedLogitsProcessor on the hooked loop"""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    L = kw["input_ids"].shape[1]
    eos = list(model.generation_config.eos_token_id)
    rng = patch_ranges(kw["image_grid_thw"], kw.get("image_index"))
    dev = model.generate(output_scores=True, token_automaton=A, max_new_tokens=T_NEW, **gen, **kw)
    dev["step_mode"] = dev.past_key_values.mode                     # the session is shared with the next call: its mode as of this one
    proc = PrefixConstrainedLogitsProcessor(T.prefix_fn(A, L, cfg.vocab_size, rng, eos), 1)
    hooked = model.generate(output_scores=True, logits_processor=[proc], max_new_tokens=T_NEW, **{k: v for k, v in gen.items() if k != "use_graph"}, **kw)
    hooked["step_mode"] = hooked.past_key_values.mode
    return dev, hooked, rng, eos


def assert_same(cfg, a, b, L, eos):
    """equal sequences; every score row up to and including the row's EOS step equal under ==, -inf at the same columns"""
    assert torch.equal(a.sequences, b.sequences), (a.sequences[:, L:].tolist(), b.sequences[:, L:].tolist())
    assert len(a.scores) == len(b.scores) == a.sequences.shape[1] - L
    tok = a.sequences[:, L:].cpu()
    n_rows = 0
    for r in range(tok.shape[0]):
        for t in range(tok.shape[1]):
            x, y = a.scores[t][r], b.scores[t][r]
            assert torch.equal(x == -INF, y == -INF), (r, t)
            assert bool((x == y).all()), (r, t)
            n_rows += 1
            if int(tok[r, t]) in eos:
                break
    return n_rows


def assert_accepted(A, cfg, out, L, rng, eos):
    tok = out.sequences[:, L:].cpu().tolist()
    for b, row in enumerate(tok):
        assert A.accepts(row, cfg.vocab_size, rng[b], eos), (b, row)
    return tok


def test_greedy_equals_the_hooked_prefix_constrained_run_and_decodes(setup):
    import test_forced_tokens_gpu as FT
    cfg, U, model, kw = setup
    A = T.label_automaton(LABELS)
    L = kw["input_ids"].shape[1]
    dev, hooked, rng, eos = hooked_twin(model, cfg, A, kw)
    assert dev["step_mode"].automaton and not hooked["step_mode"].automaton and hooked["step_mode"].processors      # the twin does not run the new kernel
    assert_same(cfg, dev, hooked, L, eos)
    tok = assert_accepted(A, cfg, dev, L, rng, eos)
    # only meaningful if the model does not satisfy the automaton unaided
    free = model.generate(max_new_tokens=T_NEW, **kw)
    assert not any(A.accepts(row, cfg.vocab_size, rng[b], eos) for b, row in enumerate(free.sequences[:, L:].cpu().tolist()))
    # every row starts with a label and its three own patches; -inf exactly outside allowed() at the first steps
    V = cfg.vocab_size
    for b, row in enumerate(tok):
        n = 2 if row[:2] in LABELS else 3
        assert row[:n] in LABELS and all(V + rng[b][0] <= x < V + rng[b][1] for x in row[n: n + 3]), (b, row)
        for t in range(n + 3):
            ok = torch.tensor(A.allowed(row[:t], V, rng[b], eos))
            fin = torch.isfinite(dev.scores[t][b]).nonzero().flatten().cpu()
            assert set(fin.tolist()) <= set(ok.tolist()) and fin.numel() > 0
    # hidden states that parseVRTintoCompletion + vl_decode accept: every row that reached its EOS decodes one object per VRT run (the
    # parser drops a completion that max_new_tokens cut inside a run) ...
    print(f"\n[automaton] constrained {tok}\n[automaton] free {free.sequences[:, L:].cpu().tolist()}")
    feats, dec = FT.decode_objects(model, cfg, U, dev, kw["image_grid_thw"], L)
    hid = dev.hidden_states.last_layer_rows()
    for b, row in enumerate(tok):
        if eos[0] in row:
            runs = [t for t in range(len(row)) if row[t] >= V and (t == 0 or row[t - 1] < V)]
            assert len(feats[b]) == len(runs) >= 1
            for f, t0 in zip(feats[b], runs):
                assert torch.equal(f, hid[t0: t0 + 3, b])
    assert dec["pred_boxes"].shape[0] == sum(len(f) for f in feats)
    # ... and without `repeat` every row is one label, three patches, EOS: three objects
    once = model.generate(token_automaton=T.label_automaton(LABELS, repeat=False), max_new_tokens=T_NEW, **kw)
    assert once.sequences.shape[1] - L <= 7 and bool((once.sequences[:, L:] == eos[0]).any(1).all())
    feats1, dec1 = FT.decode_objects(model, cfg, U, once, kw["image_grid_thw"], L)
    assert [len(f) for f in feats1] == [1, 1, 1] and all(f[0].shape[0] == 3 for f in feats1) and dec1["pred_boxes"].shape[0] == 3
    # the captured graph against eager steps, and a second prompt set through the same graph
    eager = model.generate(output_scores=True, token_automaton=A, max_new_tokens=T_NEW, use_graph=False, **kw)
    assert_same(cfg, dev, eager, L, eos)
    kw2 = batch3(cfg, U, seed=17)
    dev2, hooked2, rng2, _ = hooked_twin(model, cfg, A, kw2)
    assert_same(cfg, dev2, hooked2, kw2["input_ids"].shape[1], eos)
    assert not torch.equal(dev2.sequences[:, kw2["input_ids"].shape[1]:], dev.sequences[:, L:]), "precondition: the second prompts decode differently"
    # ... and another automaton: same step mode, same graph
    sess = dev2.past_key_values
    n_graphs = len(sess.graphs)
    assert dev2["step_mode"] in sess.graphs
    A2 = T.label_automaton([[41, 42, 43], [44, 45]], repeat=False)
    dev3, hooked3, *_ = hooked_twin(model, cfg, A2, kw)
    assert_same(cfg, dev3, hooked3, L, eos)
    assert len(dev3.past_key_values.graphs) == n_graphs and dev3.past_key_values is sess


MODES = {
    "sampling_min_p": dict(do_sample=True, seed=11, temperature=0.9, top_k=50, min_p=0.05),
    "ngram_union": dict(no_repeat_ngram_size=2),
    "penalty": dict(repetition_penalty=1.2),
    "penalty_ngram_logprobs": dict(repetition_penalty=1.2, no_repeat_ngram_size=2, output_token_logprobs=True, top_logprobs=3),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_modes_equal_the_hooked_run(setup, mode):
    cfg, U, model, kw = setup
    A = T.label_automaton(LABELS)
    L = kw["input_ids"].shape[1]
    dev, hooked, rng, eos = hooked_twin(model, cfg, A, kw, **MODES[mode])
    assert_same(cfg, dev, hooked, L, eos)
    tok = assert_accepted(A, cfg, dev, L, rng, eos)
    if "ngram" in mode:                                            # the union bites: a second object cannot repeat a (label, label) bigram
        plain = model.generate(token_automaton=A, max_new_tokens=T_NEW, **kw)
        print(f"\n[automaton + n-gram] {tok}\n[automaton alone]    {plain.sequences[:, L:].cpu().tolist()}")
        assert dev["step_mode"].rules and dev["step_mode"].automaton
        assert not torch.equal(plain.sequences, dev.sequences), "precondition: the n-gram ban changes the run"
        for row in tok:
            live = row[: row.index(eos[0]) + 1] if eos[0] in row else row
            grams = list(zip(live, live[1:]))
            assert len(grams) == len(set(grams))
    if "logprobs" in mode:
        import test_token_logprobs_gpu as TL
        t_all = dev.sequences[:, L:].cpu()
        ref = torch.stack([TL.ref_logprob(dev.scores[t], t_all[:, t]) for t in range(t_all.shape[1])], 1)
        live = torch.ones_like(ref, dtype=torch.bool)
        for b, row in enumerate(tok):
            if eos[0] in row:
                live[b, row.index(eos[0]) + 1:] = False
        TL.within(dev.token_logprobs.cpu()[live], ref[live])


def test_token_logprobs_are_the_log_softmax_over_the_allowed_columns(setup):
    import test_token_logprobs_gpu as TL
    cfg, U, model, kw = setup
    A = T.label_automaton(LABELS)
    L = kw["input_ids"].shape[1]
    eos = list(model.generation_config.eos_token_id)
    flagged = model.generate(token_automaton=A, max_new_tokens=T_NEW, output_token_logprobs=True, **kw)       # the fused path: no row written
    scored = model.generate(token_automaton=A, max_new_tokens=T_NEW, output_token_logprobs=True, output_scores=True, **kw)
    assert flagged.scores is None and torch.equal(flagged.sequences, scored.sequences)
    tok = flagged.sequences[:, L:].cpu()
    ref = torch.stack([TL.ref_logprob(scored.scores[t], tok[:, t]) for t in range(tok.shape[1])], 1)
    live = torch.ones_like(ref, dtype=torch.bool)
    for b, row in enumerate(tok.tolist()):
        if eos[0] in row:
            live[b, row.index(eos[0]) + 1:] = False
    d = TL.within(flagged.token_logprobs.cpu()[live], ref[live])
    TL.within(scored.token_logprobs.cpu()[live], ref[live])
    # a step with ONE allowed column is certain: the second token after label prefix (31,) is 32
    lp = flagged.token_logprobs.cpu()
    for b, row in enumerate(tok.tolist()):
        if row[0] == 31:
            assert row[1] == 32 and lp[b, 1] == 0.0
    assert bool((lp[live] <= 0).all()) and bool((lp[live] < 0).any())
    print(f"\n[automaton] largest |token_logprobs - log_softmax(scores)| {d:.3e}")


def test_forced_tokens_leave_the_automaton_or_are_scored_in_the_closed_set(setup):
    import test_token_logprobs_gpu as TL
    cfg, U, model, kw = setup
    A = T.label_automaton(LABELS)
    L = kw["input_ids"].shape[1]
    eos = list(model.generation_config.eos_token_id)
    base = model.generate(token_automaton=A, max_new_tokens=T_NEW, **kw)
    # a forced token without an edge: the row is off the automaton and ends on EOS at the next free step; the other rows do not notice
    out = model.generate(token_automaton=A, max_new_tokens=T_NEW, forced_tokens=[[21, 999], [], []], output_token_logprobs=True, **kw)
    tok, lp = out.sequences[:, L:].cpu(), out.token_logprobs.cpu()
    assert tok[0, :3].tolist() == [21, 999, eos[0]] and lp[0, 1] == -INF and lp[0, 2] == 0.0 and torch.isfinite(lp[0, 0])
    n = min(tok.shape[1], base.sequences.shape[1] - L)
    assert torch.equal(tok[1:, :n], base.sequences[1:, L: L + n].cpu())
    # a forced path inside the automaton: closed-set log-probs.  The start state branches into the first label tokens 21 and 31, state (21,)
    # into 22 and 23: forcing each branch in turn, the probabilities of a branching step sum to 1.  Bound: every log-prob is within
    # d_i = 5e-6 + 2^-22 |lp_i| of the exact one (test_token_logprobs_gpu.within), so |log Σ p_i| <= Σ p_i d_i <= 5e-6 + 2^-22 Σ p_i |lp_i|
    # <= 5e-6 + 2^-22 (Σ_i p_i |log p_i| <= log 2 < 1 over two branches)
    bound = 5e-6 + 2.0 ** -22
    first = [model.score_completions(completions=[[x]] * 3, token_automaton=A, **kw) for x in (21, 31)]
    p0 = sum(o.token_logprobs[:, 0].double().exp() for o in first).cpu()
    assert bool((p0.log().abs() <= bound).all()), p0.tolist()
    assert all(bool((o.token_logprobs[:, 0] < 0).all()) for o in first), "precondition: the branch is not certain"
    second = [model.score_completions(completions=[[21, x]] * 3, token_automaton=A, **kw) for x in (22, 23)]
    p1 = sum(o.token_logprobs[:, 1].double().exp() for o in second).cpu()
    assert bool((p1.log().abs() <= bound).all()), p1.tolist()
    for o, s in zip(second, first[:1] * 2):                        # the shared first step is the same number in every call
        assert torch.equal(o.token_logprobs[:, 0].view(torch.int32), s.token_logprobs[:, 0].view(torch.int32))
    assert torch.equal(second[0].completion_logprobs.view(torch.int32), second[0].token_logprobs[:, :2].sum(1).view(torch.int32))
    # a completion that leaves the automaton scores -inf there
    bad = model.score_completions(completions=[[21, 31]] * 3, token_automaton=A, **kw)
    assert bool((bad.completion_logprobs == -INF).all())
    # without an automaton the same branch is scored against the whole table: strictly less
    open_set = model.score_completions(completions=[[21]] * 3, **kw)
    assert bool((open_set.token_logprobs[:, 0] < first[0].token_logprobs[:, 0]).all())


def test_schedule_and_caller_processors_compose(setup):
    """the automaton is applied by the head, before a caller's processor sees the row; a schedule step that contradicts it leaves pad / EOS"""
    cfg, U, model, kw = setup
    A = T.label_automaton(LABELS)
    L = kw["input_ids"].shape[1]
    eos = list(model.generation_config.eos_token_id)
    seen = []

    def spy(input_ids, scores):
        seen.append(torch.isfinite(scores).sum(1).cpu().tolist())
        return scores
    out = model.generate(token_automaton=A, max_new_tokens=4, logits_processor=[spy], **kw)
    assert seen[0] == [2, 2, 2] and out.past_key_values.mode.automaton and out.past_key_values.mode.processors       # 21 / 31 at the start
    assert seen[1] == [2 if r[0] == 21 else 1 for r in out.sequences[:, L:].cpu().tolist()]                          # 22 / 23 after 21, 32 after 31
    rng = patch_ranges(kw["image_grid_thw"])
    assert_accepted(A, cfg, out, L, rng, eos)
    # schedule 'e' at step 1 forces EOS where the automaton wants a label token: the intersection is empty, the row emits pad, is off the
    # automaton and ends on EOS
    out = model.generate(token_automaton=A, max_new_tokens=4, schedule=["t", "e", None, None], **kw)
    tok = out.sequences[:, L:].cpu()
    assert bool((tok[:, 1] == cfg.pad_token_id).all()) and bool((tok[:, 2] == eos[0]).all())


def test_image_index(setup):
    cfg, U, model, _ = setup
    A = T.label_automaton(LABELS)
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8]], n_pre=6, n_post=9, seed=93)
    ids = ids.repeat(3, 1)
    ids[1, -4:] = torch.tensor([5, 6, 7, 8])
    ids[2, -4:] = torch.tensor([9, 10, 11, 12])
    kw = dict(input_ids=ids.cuda(), attention_mask=am.repeat(3, 1).cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, image_index=[0, 0, 0])
    dev, hooked, rng, eos = hooked_twin(model, cfg, A, kw)
    assert rng == [(0, 16), (16, 32), (32, 48)]
    assert_same(cfg, dev, hooked, ids.shape[1], eos)
    assert_accepted(A, cfg, dev, ids.shape[1], rng, eos)


@pytest.mark.parametrize("llm_weights", ["fp8", "fp4"])
def test_quantised_weight_images(llm_weights):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import padt_amd
    import parity_util as U
    from padt_amd.modeling import PaDTForConditionalGeneration
    cfg = padt_amd.small_test_config()
    model = PaDTForConditionalGeneration(cfg, U.bf16_weights(cfg, seed=5, std=0.05), device="cuda", llm_weights=llm_weights)
    kw = batch3(cfg, U)
    A = T.label_automaton(LABELS)
    dev, hooked, rng, eos = hooked_twin(model, cfg, A, kw)
    assert_same(cfg, dev, hooked, kw["input_ids"].shape[1], eos)
    assert_accepted(A, cfg, dev, kw["input_ids"].shape[1], rng, eos)


def test_reference_precision():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_token_logprobs_gpu as TL
    cfg, U, model = TL.small_model(precision="reference")
    kw = batch3(cfg, U)
    A = T.label_automaton(LABELS)
    dev, hooked, rng, eos = hooked_twin(model, cfg, A, kw)
    assert dev["step_mode"].reference and dev["step_mode"].automaton
    assert_same(cfg, dev, hooked, kw["input_ids"].shape[1], eos)
    assert_accepted(A, cfg, dev, kw["input_ids"].shape[1], rng, eos)


def test_merged_decode_groups_share_only_equal_automata(setup):
    cfg, U, model, _ = setup
    import padt_amd
    from padt_amd import pipeline
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 64), 2)
    proc.model_embed_token_size = cfg.vocab_size
    batches = []
    for s, g in enumerate([GRIDS, [[1, 6, 10], [1, 8, 8], [1, 8, 10]]]):
        grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5 + 3 * s, n_post=7, seed=100 + s, ragged=True)
        batches.append((ids.cuda(), am.cuda(), pix.cuda(), grid))
    A = T.label_automaton(LABELS)
    same = T.label_automaton(list(reversed(LABELS)))                # an equal automaton built separately
    other = T.label_automaton(LABELS, repeat=False)
    gen = dict(max_new_tokens=T_NEW, output_token_logprobs=True)
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], token_automaton=A, **gen) for b in batches]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b, a in zip(batches, (A, same)):
        got += runner.submit(b[0].clone(), *b[1:], token_automaton=a, **gen)
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2
    for (d0, c0, l0, v0), (d1, c1, l1, v1) in zip(alone, got):
        assert c0 == c1 and v0 == v1, "tokens of the merged group differ from the batch alone"
        assert torch.equal(d0["token_logprobs"].view(torch.int32), d1["token_logprobs"].view(torch.int32))
        assert torch.equal(d0["pred_boxes"], d1["pred_boxes"]) and d0["pred_boxes"].shape[0] >= 1
    # different automata, and an automaton next to none, never share a group
    for second in (other, None):
        runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
        got = runner.submit(batches[0][0].clone(), *batches[0][1:], token_automaton=A, **gen)
        got += runner.submit(batches[1][0].clone(), *batches[1][1:], token_automaton=second, **gen)
        got += runner.flush()
        assert runner.n_groups == 2 and len(got) == 2
        assert got[0][1] == alone[0][1] and torch.equal(got[0][0]["token_logprobs"].view(torch.int32), alone[0][0]["token_logprobs"].view(torch.int32))
        if second is None:
            assert got[1][1] != alone[1][1], "precondition: the unconstrained batch makes its own choice"


def test_range_guard_rerun_passes_the_automaton_on():
    """operands="auto": the batch whose SwiGLU hidden exceeds fp16's range (test_range_guard_gpu's `llm_swiglu` weights) is answered by the bf16
    twin under the caller's automaton — what the bf16 model gives directly"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_range_guard_gpu as RG
    from padt_amd.modeling import PaDTForConditionalGeneration
    cfg, w, U = RG._weights("llm_swiglu")
    grid, pix, ids, am = U.synthetic_batch(cfg, GRIDS, n_pre=5, n_post=8, ragged=True, seed=41)
    kw = dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    A = T.label_automaton(LABELS)
    gen = dict(max_new_tokens=T_NEW, output_token_logprobs=True, token_automaton=A)
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16").generate(**gen, **kw)
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(**gen, **kw)
    assert auto.overflow_reruns == 1
    assert torch.equal(got.sequences, ref.sequences) and torch.equal(got.token_logprobs.view(torch.int32), ref.token_logprobs.view(torch.int32))
    assert_accepted(A, cfg, got, ids.shape[1], patch_ranges(grid), [cfg.eos_token_id])


# ------------------------------------------------------------------------------------------------------------ what is launched
NEW_WRAPPERS = ("token_automaton", "token_automaton_tensor")


def _recorded(monkeypatch, ops, model, kw, **gen):
    """the ops wrappers a generate goes through, in order"""
    calls = []
    with monkeypatch.context() as mp:
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_"):
                def stub(*a, _fn=fn, _name=name, **k):
                    calls.append(_name + ("+ban" if _name == "vrt_head" and k.get("ban") is not None else ""))
                    return _fn(*a, **k)
                mp.setattr(ops, name, stub)
        out = model.generate(use_graph=False, max_new_tokens=T_NEW, **gen, **kw)
    return calls, out


@pytest.mark.parametrize("rules", [dict(), dict(no_repeat_ngram_size=2)], ids=["plain", "ngram"])
def test_an_unconstrained_call_launches_what_it_launched_before(setup, ops, monkeypatch, rules):
    cfg, U, model, kw = setup
    A = T.label_automaton(LABELS)
    plain, a = _recorded(monkeypatch, ops, model, kw, **rules)
    none, b = _recorded(monkeypatch, ops, model, kw, token_automaton=None, **rules)
    assert none == plain and torch.equal(a.sequences, b.sequences) and not a.past_key_values.mode.automaton
    assert not any(c in NEW_WRAPPERS for c in plain)
    assert ("vrt_head+ban" in plain) == bool(rules) and ("vrt_head" in plain) != bool(rules)
    # with the automaton: the same launches plus ONE kernel in front of every head call (and one table upload); the head reads a bitmap
    flagged, c = _recorded(monkeypatch, ops, model, kw, token_automaton=A, **rules)
    n_steps = c.sequences.shape[1] - kw["input_ids"].shape[1]
    heads = [i for i, x in enumerate(flagged) if x.startswith("vrt_head") and "nblk" not in x]
    assert all(flagged[i] == "vrt_head+ban" and flagged[i - 1] in ("token_automaton", "pack_rows") for i in heads)
    assert flagged.count("token_automaton") == len(heads) >= n_steps and flagged.count("token_automaton_tensor") == 1
    if not rules:                                                  # a constrained run may end at another step; step by step the lists agree
        per_step = lambda xs: [x.replace("+ban", "") for x in xs if x not in NEW_WRAPPERS]
        k = min(len(per_step(flagged)), len(per_step(plain)))
        assert per_step(flagged)[: k // 2] == per_step(plain)[: k // 2]
