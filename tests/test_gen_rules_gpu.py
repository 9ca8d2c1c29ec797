"""Device-side bans of generate(): no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens.

Kernel level: padt_gen_rules' bitmap against the installed HF logits-processor classes applied to a zero row (the ban set is where they return
-inf; exact equality of bits), padt_vrt_head_ban against the ban-less head (bit for bit outside the banned columns).  End to end (the small
synthetic model of test_e2e_gpu.py, two ragged samples): the device path — captured steps — against the SAME model with the HF classes passed
as `logits_processor=[...]` on the hooked loop (which the existing suite shows to reproduce the captured run bit for bit): sequences, every
`.scores[t]` and the per-step hidden rows equal, in every mode the bans are wired into."""
import pytest
import torch

import gen_rules_util as G

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
INF = float("inf")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------ the rules kernel
GUARD, GUARD_WORD = 4, 0x5A5A5A5A


class Rows:
    """Device state of one padt_gen_rules problem: rule table, padded prompt rows, token buffer, step counter and a ban bitmap pre-filled with
    garbage between two runs of sentinel words."""

    def __init__(self, ops, rules, eos, vocab, width, prompts, tokens, t, t_max=None):
        self.ops, self.width, B = ops, width, len(prompts)
        self.rules = ops.gen_rules_tensor(eos_ids=eos, vocab_size=vocab, **rules).cuda()
        ld = max(len(p) for p in prompts) + 3
        hist = torch.full((B, ld), G.TEXT[0], dtype=torch.int32)                  # past hist_len: an id of the alphabet (an over-read would match)
        for b, p in enumerate(prompts):
            hist[b, : len(p)] = torch.tensor(p, dtype=torch.int32)
        self.hist, self.hist_len = hist.cuda(), i32([len(p) for p in prompts])
        t_max = t_max or max(max(len(tk) for tk in tokens), 1) + 2
        tok = torch.full((B, t_max), G.TEXT[1], dtype=torch.int64)               # past the step counter: likewise
        for b, tk in enumerate(tokens):
            tok[b, : len(tk)] = torch.tensor(tk, dtype=torch.int64)
        self.tokens, self.step = tok.cuda(), i32([t])
        self.words = (width + 31) // 32
        self.flat = torch.full((2 * GUARD + B * self.words,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.ban = self.flat[GUARD: GUARD + B * self.words].view(B, self.words)
        self.ban.fill_(-1)                                                       # every bit set: the kernel rebuilds the row from nothing

    def run(self):
        self.ops.gen_rules(self.rules, self.hist, self.hist_len, self.tokens, self.step, self.ban, self.width)

    def bitmap(self):
        got, tail_clear = G.bitmap_to_bool(self.ban, self.width)
        assert tail_clear, "bits past the table width are set"
        assert bool((self.flat[:GUARD] == GUARD_WORD).all()) and bool((self.flat[-GUARD:] == GUARD_WORD).all()), "sentinel words around ban overwritten"
        return got


def test_rules_kernel_random_rule_sets_equal_the_hf_classes(ops):
    """60 seeded rule sets x 5 rows (hist_len in {1, 7, 40}, step in {0, 1, 2, 9}, ids from 5 text + 2 VRT ids, a 113-column table): bit for bit
    HF's ban set; bits past the width zero, sentinels intact.  test_gen_rules_cpu.py asserts the conditions these seeds are chosen for (at least
    90 % of the rows have a non-empty ban set, every rule kind bites in at least 10 cases)."""
    for seed in range(G.N_CASES):
        rules, lens, t, tokens, prompts = G.random_case(seed)
        r = Rows(ops, rules, G.EOS, G.V, G.WIDTH, prompts, tokens, t)
        r.run()
        got = r.bitmap()
        for b, (L, p, tk) in enumerate(zip(lens, prompts, tokens)):
            want = G.hf_ban(rules, G.EOS, p + tk, L, G.WIDTH)
            assert torch.equal(got[b], want), (seed, b, rules, p, tk, got[b].nonzero().flatten().tolist(), want.nonzero().flatten().tolist())


def test_rules_kernel_long_history_and_the_prompt_token_boundary(ops):
    g = torch.Generator().manual_seed(5)
    # L = 890, t = 119 (the OVD geometry's last step), n = 3 over a 3-id alphabet: every thread of the block walks the stride loop four times
    L, t = 890, 119
    h = [[(3, 64, G.VRT[0])[i] for i in torch.randint(0, 3, (L + t,), generator=g).tolist()] for _ in range(2)]
    r = Rows(ops, dict(no_repeat_ngram_size=3), (), G.V, G.WIDTH, [x[:L] for x in h], [x[L:] for x in h], t)
    r.run()
    got = r.bitmap()
    for b in range(2):
        want = G.hf_ban(dict(no_repeat_ngram_size=3), (), h[b], L, G.WIDTH)
        assert want.any() and torch.equal(got[b], want)
    # the ONLY n-gram match straddles the boundary: (1, 2 | 3) with 1, 2 the prompt's last ids and 3 the first generated one
    rules = dict(no_repeat_ngram_size=3)
    prompt, toks = [10, 11, 12, 13, 14, 1, 2], [3, 20, 21, 1, 2]
    r = Rows(ops, rules, (), G.V, G.WIDTH, [prompt], [toks], len(toks))
    r.run()
    want = G.hf_ban(rules, (), prompt + toks, len(prompt), G.WIDTH)
    assert want.nonzero().flatten().tolist() == [3] and torch.equal(r.bitmap()[0], want)
    # a bad word whose prefix straddles the boundary: (2 | 3) → 50; one id earlier or later it does not match
    rules = dict(bad_words_ids=[[2, 3, 50]])
    for toks, hit in (([3], True), ([], False), ([3, 3], False)):
        r = Rows(ops, rules, (), G.V, G.WIDTH, [prompt], [toks], len(toks))
        r.run()
        want = G.hf_ban(rules, (), prompt + toks, len(prompt), G.WIDTH)
        assert bool(want[50]) == hit and int(want.sum()) == int(hit) and torch.equal(r.bitmap()[0], want)
    # HF's length condition: a word as long as the history PLUS one is skipped (cur >= m, not m - 1)
    rules = dict(bad_words_ids=[[7, 8, 9]])
    for prompt2, hit in (([7, 8], False), ([5, 7, 8], True)):
        r = Rows(ops, rules, (), G.V, G.WIDTH, [prompt2], [[]], 0)
        r.run()
        want = G.hf_ban(rules, (), prompt2, len(prompt2), G.WIDTH)
        assert bool(want[9]) == hit and torch.equal(r.bitmap()[0], want)
    # a rule id that is a VRT id is refused by the packer (VRT numbering differs per batch of a merged group) ...
    with pytest.raises(NotImplementedError, match="bad_words_ids"):
        ops.gen_rules_tensor(bad_words_ids=[[3, G.VRT[0]]], vocab_size=G.V)
    # ... while the banned FOLLOWER of an n-gram and the matched history may be VRT ids
    v0, v1 = G.VRT
    rules = dict(no_repeat_ngram_size=2)
    r = Rows(ops, rules, (), G.V, G.WIDTH, [[v0, v1, 3]], [[v0]], 1)
    r.run()
    assert r.bitmap()[0].nonzero().flatten().tolist() == [v1] == G.hf_ban(rules, (), [v0, v1, 3, v0], 3, G.WIDTH).nonzero().flatten().tolist()


def test_rules_kernel_leaves_no_stale_bits_and_replays_in_a_graph(ops):
    rules = dict(begin_suppress_tokens=[40], bad_words_ids=[[3, 17, 64]], no_repeat_ngram_size=2, suppress_tokens=[95])
    prompt = [31, 3]
    script = [17, 5, 3, 17, 31, 3]                                               # the tokens the scripted "decode" appends, one per step
    r = Rows(ops, rules, (), G.V, G.WIDTH, [prompt, prompt[::-1]], [script, script[::-1]], 0, t_max=8)
    hists = [prompt + script, prompt[::-1] + script[::-1]]

    def want(t):
        return torch.stack([G.hf_ban(rules, (), h[: 2 + t], 2, G.WIDTH) for h in hists])
    # eager, the same bitmap rebuilt step after step
    seen = []
    for t in range(4):
        r.step.fill_(t)
        r.run()
        seen.append(r.bitmap())
        assert torch.equal(seen[-1], want(t)), t
    assert bool(seen[0][0, 40]) and not bool(seen[1][0, 40])                     # the begin-suppress bit of step 0 is gone at step 1
    assert bool(seen[1][0, 64]) and not bool(seen[2][0, 64])                     # (3, 17) → 64 at step 1; the prefix no longer matches at step 2
    # captured: rules kernel + the step increment in one graph, replayed six times over the scripted token buffer
    r.step.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.run()
        r.step.add_(1)
    r.step.zero_()
    r.ban.fill_(-1)
    for t in range(6):
        g.replay()
        assert torch.equal(r.bitmap(), want(t)), t
    assert int(r.step.item()) == 6


# ------------------------------------------------------------------------------------------------------------ the head
def _head(ops, h, E, P, off, packed, ban="none"):
    """→ (part_val, part_idx, logits): ban "none" = padt_vrt_head, "null" = padt_vrt_head_ban with a null bitmap, else the bitmap."""
    B, D = h.shape
    V, NP = E.shape[0], P.shape[0]
    nblk = ops.vrt_head_nblk(V, NP)
    pv = torch.full((nblk * B,), float("nan"), device="cuda")
    pi = torch.full((nblk * B,), -5, dtype=torch.int32, device="cuda")
    lg = torch.full((B, V + NP), float("nan"), device="cuda")
    hid, Ep = h, None
    if packed:
        hid = torch.zeros((B + 15) // 16 * 16, D, device="cuda", dtype=h.dtype)
        ops.pack_rows(h, hid, B, to_packed=True)
        Ep = ops.pack_weight(E)
    if isinstance(ban, str) and ban == "null":
        from padt_amd import _lib
        p = ops._p
        _lib.check(ops._fn("padt_vrt_head_ban", h.dtype)(ops._stream(), p(hid), hid.stride(0), p(E), V, p(P), NP, p(off), 0, 0, p(lg), lg.stride(0),
                                                         p(pv), p(pi), B, D, -3, p(Ep), 0, 0, 0, 0, 0), "padt_vrt_head_ban")
    else:
        ops.vrt_head(hid, E, P, off, pv, pi, -3, logits=lg, table_packed=Ep, rows=B, ban=None if isinstance(ban, str) else ban)
    return pv, pi, lg


def _select(ops, pv, pi, nblk, B, pad):
    D = 8
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    tok = torch.full((B, 1), -9, dtype=torch.int64, device="cuda")
    cur = torch.full((B,), -9, dtype=torch.int64, device="cuda")
    ops.greedy_step(pv, pi, nblk, torch.zeros(B, D, device="cuda", dtype=BF), torch.zeros(1, B, D, device="cuda", dtype=BF),
                    torch.ones(B, dtype=torch.int32, device="cuda"), tok, cur, z(1), z(B), z(B), z(3, B), -1, pad)
    return cur.cpu()


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("layout", ["rowmajor", "packed"])
@pytest.mark.parametrize("B", [5, 33, 128])
def test_head_with_a_ban_bitmap(ops, dt, layout, B):
    """padt_vrt_head_ban: logits equal the ban-less run bit for bit except -inf at the banned bits; the fused token is the first arg-max of the
    written row — every row's ban-less arg-max is planted in the bitmap, so the selection must move; a null / all-zero bitmap is padt_vrt_head;
    a fully banned row emits pad and leaves the other rows alone."""
    g = torch.Generator().manual_seed(700 + B)
    V, D, pad = 1040, 256, 11
    counts = [0] + [1 + (5 * b + b // 3) % 11 for b in range(1, B)]             # ragged: the width V + NP is no multiple of 32 for any B here
    NP = sum(counts)
    assert (V + NP) % 32
    E = torch.randn(V, D, generator=g).to(dt).cuda()
    P = torch.randn(NP, D, generator=g).to(dt).cuda()
    h = torch.randn(B, D, generator=g).to(dt).cuda()
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    off = i32(offs)
    packed = layout == "packed"
    nblk = ops.vrt_head_nblk(V, NP)
    pv0, pi0, lg0 = _head(ops, h, E, P, off, packed)
    words = (V + NP + 31) // 32
    for variant in ("null", torch.zeros((B, words), dtype=torch.int32, device="cuda")):
        pv, pi, lg = _head(ops, h, E, P, off, packed, ban=variant)
        assert torch.equal(lg.view(torch.int32), lg0.view(torch.int32)) and torch.equal(pv.view(torch.int32), pv0.view(torch.int32)) and torch.equal(pi, pi0)
    base = lg0.cpu()
    top = base.argmax(-1)
    banned = torch.rand((B, V + NP), generator=g) < 0.05
    banned[torch.arange(B), top] = True                                         # plant every row's current arg-max
    for b in range(1, B):
        banned[b, V + offs[b]] = True                                            # ... and the first VRT column of the row's own range
    full = 2                                                                     # one row with every column banned
    banned[full] = True
    bits = torch.zeros((B, words * 32), dtype=torch.bool)
    bits[:, : V + NP] = banned
    ban = (bits.view(B, words, 32).long() << torch.arange(32)).sum(-1)
    ban = torch.where(ban >= 2 ** 31, ban - 2 ** 32, ban).to(torch.int32).cuda()
    pv1, pi1, lg1 = _head(ops, h, E, P, off, packed, ban=ban)
    out = lg1.cpu()
    want = torch.where(banned, torch.full_like(base, -INF), base)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "logits differ from the ban-less run outside the banned columns"
    tok = _select(ops, pv1, pi1, nblk, B, pad)
    live = torch.arange(B) != full
    assert torch.isfinite(out[live]).any(-1).all()
    assert torch.equal(tok[live], out.argmax(-1)[live]), "fused token != first arg-max of the written row"
    assert bool((tok[live] != top[live]).all()), "the planted arg-max was selected"
    assert int(tok[full]) == pad and not torch.isfinite(out[full]).any(), "a fully banned row must emit pad"


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module", params=["fp16", "bf16"])
def setup(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    w = U.bf16_weights(cfg, seed=5, std=0.05)
    model = PaDTForConditionalGeneration(cfg, w, device="cuda", operands=request.param)
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 10, 12], [1, 8, 8]], n_pre=6, n_post=9, ragged=True, seed=91)
    kw = dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    return cfg, w, model, U, kw


T_REC = 12
SCHED = ["t"] * 5 + ["v"] * 3 + ["t"] * 3 + ["e"]                                # steps 0-4 text (the rules below are text ids), a VRT run, EOS forced last


def _twin(model, cfg, kw, rules, **gen):
    """(device path, hooked twin): the same generate with the bans as arguments, and with HF's classes as logits_processor on the hooked loop."""
    L = kw["input_ids"].shape[1]
    dev = model.generate(output_scores=True, **rules, **gen, **kw)
    procs = G.hf_processors(rules, model.generation_config.eos_token_id, L, device="cuda")
    hooked = model.generate(output_scores=True, logits_processor=procs, **gen, **kw)
    return dev, hooked


def _assert_same(a, b):
    assert torch.equal(a.sequences, b.sequences)
    assert len(a.scores) == len(b.scores) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    assert torch.equal(a.hidden_states.buf, b.hidden_states.buf)


def _rules_from(base_tok):
    """Rules that bite by construction, from an unconstrained run's tokens (B, T)."""
    return dict(bad_words_ids=[[int(base_tok[0, 1]), int(base_tok[0, 2])], [int(base_tok[1, 0])]],
                suppress_tokens=[int(base_tok[0, 3])], begin_suppress_tokens=[int(base_tok[0, 0])])


@pytest.mark.parametrize("which", ["bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "no_repeat_ngram_size", "all"])
def test_generate_bans_equal_the_hf_classes_on_the_hooked_loop(setup, which):
    cfg, w, model, U, kw = setup
    L = kw["input_ids"].shape[1]
    if which == "no_repeat_ngram_size":
        gen = dict(max_new_tokens=24)                                           # a free schedule
    else:
        gen = dict(max_new_tokens=T_REC, schedule=SCHED)
        if which == "all":
            gen["repetition_penalty"] = 1.3                                     # the unconstrained run carries the penalty too
    base = model.generate(output_scores=True, **gen, **kw)
    btok = base.sequences[:, L:].cpu()
    if which == "no_repeat_ngram_size":
        # the smallest n for which the unconstrained run repeats an n-gram on a live row: a token HF's processor bans given the run's own history
        def repeats(n):
            for b in range(btok.shape[0]):
                for t in range(btok.shape[1]):
                    if G.hf_ban(dict(no_repeat_ngram_size=n), (), base.sequences[b, : L + t].tolist(), L, cfg.vocab_size + 200)[int(btok[b, t])]:
                        return True
                    if int(btok[b, t]) == cfg.eos_token_id:
                        break
            return False
        ns = [n for n in (1, 2, 3) if repeats(n)]
        assert ns, "precondition: the unconstrained run repeats no 1-, 2- or 3-gram"
        rules = dict(no_repeat_ngram_size=ns[0])
    else:
        assert int(btok[:, :5].max()) < cfg.vocab_size, "precondition: the rules are taken from text steps"
        rules = _rules_from(btok)
        if which != "all":
            rules = {which: rules[which]}
        else:
            rules["no_repeat_ngram_size"] = 2
    dev, hooked = _twin(model, cfg, kw, rules, **gen)
    _assert_same(dev, hooked)
    assert not torch.equal(dev.sequences[:, L:].cpu()[:, : btok.shape[1]], btok[:, : dev.sequences.shape[1] - L]), "the rules did not bite"
    # what the arguments say, read off the result itself
    tok = dev.sequences[:, L:].cpu()
    if "suppress_tokens" in rules:
        assert not torch.isin(tok, torch.tensor(rules["suppress_tokens"])).any()
        assert all(bool((s[:, rules["suppress_tokens"]] == -INF).all()) for s in dev.scores)
    if "begin_suppress_tokens" in rules:
        assert not torch.isin(tok[:, 0], torch.tensor(rules["begin_suppress_tokens"])).any()
        assert bool((dev.scores[0][:, rules["begin_suppress_tokens"]] == -INF).all())
    if "bad_words_ids" in rules:
        assert not (tok == rules["bad_words_ids"][1][0]).any()
    # the eager loop and the defaults of a loaded generation_config.json give the same run
    assert torch.equal(model.generate(use_graph=False, **rules, **gen, **kw).sequences, dev.sequences)
    saved = {k: getattr(model.generation_config, k) for k in rules}
    try:
        model.load_generation_config(rules)
        assert torch.equal(model.generate(**gen, **kw).sequences, dev.sequences)
        off = dict(no_repeat_ngram_size=0, bad_words_ids=[], suppress_tokens=[], begin_suppress_tokens=[])
        assert torch.equal(model.generate(**off, **gen, **kw).sequences, base.sequences)       # explicit "off" values win over the defaults
    finally:
        for k, v in saved.items():
            setattr(model.generation_config, k, v)
    assert torch.equal(model.generate(**gen, **kw).sequences, base.sequences)                   # and the rule-less graph is untouched


def test_generation_config_object_and_output_logits_policy(setup):
    cfg, w, model, U, kw = setup
    from transformers import GenerationConfig
    L = kw["input_ids"].shape[1]
    gen = dict(max_new_tokens=T_REC, schedule=SCHED)
    btok = model.generate(**gen, **kw).sequences[:, L:].cpu()
    rules = _rules_from(btok)
    want = model.generate(**rules, **gen, **kw).sequences
    got = model.generate(generation_config=GenerationConfig(max_new_tokens=T_REC, **rules), schedule=SCHED, **kw).sequences
    assert torch.equal(got, want)
    got = model.generate(generation_config=dict(rules, max_new_tokens=3), **gen, **kw).sequences                   # the explicit max_new_tokens wins
    assert torch.equal(got, want)
    # in the hooked loop the built-in bans run first: a caller's processor already sees -inf there, and what it returns is selected from
    seen = []

    def caller(input_ids, scores):
        seen.append(bool((scores[:, rules["suppress_tokens"]] == -INF).all()) and (input_ids.shape[1] > L or bool((scores[:, rules["begin_suppress_tokens"]] == -INF).all())))
        return scores
    got = model.generate(logits_processor=[caller], **rules, **gen, **kw).sequences
    assert len(seen) == got.shape[1] - L and all(seen) and torch.equal(got, want)
    with pytest.raises(NotImplementedError, match="output_logits"):
        model.generate(output_logits=True, max_new_tokens=4, suppress_tokens=[5], **kw)
    with pytest.raises(NotImplementedError, match="suppress_tokens"):
        model.generate(max_new_tokens=4, suppress_tokens=[cfg.vocab_size], **kw)                                   # a VRT id in a rule
    out = model.generate(output_logits=True, output_scores=True, max_new_tokens=4, do_sample=True, top_k=0, seed=1, suppress_tokens=[5], **kw)
    assert all(bool((lg[:, 5] == -INF).all()) for lg in out.logits)             # under sampling the raw rows are the head's: bans applied


def test_merged_groups_share_rules_or_do_not_merge(setup):
    """PipelinedRunner(merge=2): two batches of different prompt length with the same rules decode in one session (the second batch's VRT ids
    shifted in history and token buffer alike) and equal each batch run alone; batches with different rules do not share a group."""
    cfg, w, model, U, kw0 = setup
    import padt_amd
    from padt_amd import pipeline
    T = 10
    sched = ["t"] * 3 + ["v"] * 4 + ["t"] * 2 + ["e"]
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 40), 2)
    proc.model_embed_token_size = cfg.vocab_size
    batches = []
    for s, g in enumerate([[[1, 8, 8], [1, 10, 12]], [[1, 6, 10], [1, 8, 8]]]):
        grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5 + 3 * s, n_post=7, seed=100 + s, ragged=True)
        batches.append((ids.cuda(), am.cuda(), pix.cuda(), grid))
    assert batches[0][0].shape[1] != batches[1][0].shape[1]
    free = [pipeline.rec_batch(model, proc, b[0].clone(), b[1], b[2], b[3], max_new_tokens=T, schedule=sched) for b in batches]
    rules = dict(no_repeat_ngram_size=1, suppress_tokens=[3, 9], bad_words_ids=[[1, 2]])         # n = 1: a VRT run cannot repeat a VRT
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), b[1], b[2], b[3], max_new_tokens=T, schedule=sched, **rules) for b in batches]
    assert all(a[3] != f[3] or a[1] != f[1] for a, f in zip(alone, free)), "the rules did not bite"
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b in batches:
        got += runner.submit(b[0].clone(), b[1], b[2], b[3], max_new_tokens=T, schedule=sched, **rules)
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2
    for (d0, c0, l0, v0), (d1, c1, l1, v1) in zip(alone, got):
        assert c0 == c1 and v0 == v1
        assert torch.equal(d0["pred_boxes"], d1["pred_boxes"]) and torch.equal(d0["pred_mask"], d1["pred_mask"])
    # different rules: the second batch opens a group of its own, results as alone
    other = dict(rules, suppress_tokens=[3])
    alone1 = pipeline.rec_batch(model, proc, batches[1][0].clone(), *batches[1][1:], max_new_tokens=T, schedule=sched, **other)
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = runner.submit(batches[0][0].clone(), *batches[0][1:], max_new_tokens=T, schedule=sched, **rules)
    got += runner.submit(batches[1][0].clone(), *batches[1][1:], max_new_tokens=T, schedule=sched, **other)
    got += runner.flush()
    assert runner.n_groups == 2 and len(got) == 2
    for (d0, c0, l0, v0), (d1, c1, l1, v1) in zip([alone[0], alone1], got):
        assert c0 == c1 and v0 == v1 and torch.equal(d0["pred_boxes"], d1["pred_boxes"])


def test_sampling_never_draws_a_suppressed_token(setup):
    cfg, w, model, U, kw = setup
    L = kw["input_ids"].shape[1]
    gen = dict(max_new_tokens=24, schedule=["t"] * 24, do_sample=True, top_k=8, seed=7)
    drawn = model.generate(**gen, **kw).sequences[:, L:].cpu()
    sup = sorted(set(drawn.flatten().tolist()) - {cfg.eos_token_id, cfg.pad_token_id})          # everything the free run drew
    assert len(sup) >= 8
    out = model.generate(output_scores=True, suppress_tokens=sup, **gen, **kw)
    tok = out.sequences[:, L:].cpu()
    assert not torch.isin(tok, torch.tensor(sup)).any()
    assert all(bool((s[:, sup] == -INF).all()) for s in out.scores)
    assert all(bool(torch.isfinite(s).any(-1).all()) for s in out.scores)


def test_reference_precision_run_with_a_bad_word_equals_its_hooked_twin():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    model = PaDTForConditionalGeneration(cfg, U.bf16_weights(cfg, seed=5, std=0.05), device="cuda", precision="reference")
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 10, 12], [1, 8, 8]], n_pre=6, n_post=9, ragged=True, seed=91)
    kw = dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    L, gen = ids.shape[1], dict(max_new_tokens=T_REC, schedule=SCHED)
    btok = model.generate(**gen, **kw).sequences[:, L:].cpu()
    rules = dict(bad_words_ids=_rules_from(btok)["bad_words_ids"])
    dev, hooked = _twin(model, cfg, kw, rules, **gen)
    _assert_same(dev, hooked)
    assert not torch.equal(dev.sequences[:, L:].cpu(), btok)


@pytest.mark.parametrize("llm_weights", ["fp8", "fp4"])
def test_quantised_llm_weights_with_all_four_bans_equal_the_hooked_twin(llm_weights):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dataclasses
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    cfg = dataclasses.replace(cfg, tie_word_embeddings=False, num_attention_heads=4, num_key_value_heads=2, hidden_size=512)
    cfg = dataclasses.replace(cfg, vision_config=dataclasses.replace(cfg.vision_config, out_hidden_size=512))
    model = PaDTForConditionalGeneration(cfg, U.bf16_weights(cfg, seed=19, std=0.05), device="cuda", llm_weights=llm_weights)
    assert model.W.llm_weights == llm_weights
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8], [1, 10, 12]], n_pre=5, n_post=8, ragged=True, seed=77)
    kw = dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    L, gen = ids.shape[1], dict(max_new_tokens=T_REC, schedule=SCHED)
    btok = model.generate(**gen, **kw).sequences[:, L:].cpu()
    rules = dict(_rules_from(btok), no_repeat_ngram_size=2)
    dev, hooked = _twin(model, cfg, kw, rules, **gen)
    _assert_same(dev, hooked)
    assert not torch.equal(dev.sequences[:, L:].cpu(), btok)


def test_bf16_fallback_rerun_keeps_the_rules():
    """operands="auto": a batch whose SwiGLU hidden exceeds fp16's range is re-run on the bf16 twin WITH the bans — the result is the bf16
    model's own constrained run (the weight edit is test_range_guard_gpu.py's `llm_swiglu` case)."""
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
    L, gen = ids.shape[1], dict(max_new_tokens=T_REC, schedule=SCHED)
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16")
    btok = ref.generate(**gen, **kw).sequences[:, L:].cpu()
    rules = dict(_rules_from(btok), no_repeat_ngram_size=2)
    want = ref.generate(**rules, **gen, **kw)
    assert not torch.equal(want.sequences[:, L:].cpu(), btok)
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(**rules, **gen, **kw)
    assert auto.overflow_reruns == 1 and torch.equal(got.sequences, want.sequences)
    assert torch.equal(got.hidden_states.last_layer_rows(), want.hidden_states.last_layer_rows())
