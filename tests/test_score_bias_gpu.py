"""generate(logit_bias=, patch_bias=, exponential_decay_length_penalty=) on the device.

Kernel level: padt_vrt_head_bias on the smallest table that still has every corner — D = 64, 96 text rows + patch ranges of 5 and 12 = 113
columns (the last 16-column block holds one column), 2 and 17 rows (a second 16-row sample block), packed and row-major table, both operand
twins, the plain / LSE / probe heads — against generation.score_bias_row, the plain statement of the specification that
test_score_bias_cpu.py pins to HF's processors bit for bit, evaluated in fp32 torch on the parent head's penalty-free row: the written row bit
for bit, the arg-max partials, the LSE fold (test_token_logprobs_gpu.within: 5e-6 + 2^-22 |ref|, derived there for this fold of the same
logit bits), the probe value, null pointers against the four older entry points, guard words around every output.

End to end (the small synthetic model, two ragged samples): the captured step against the HOOKED loop running HF's own processor (or one
that adds the same vector) as ``logits_processor=`` — sequences, every score row and the hidden rows equal."""
import types

import pytest
import torch

import test_token_logprobs_gpu as TL
import test_token_selection_gpu as TS

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
X16 = TL.X16
INF = float("inf")
PAD = TL.PAD
i32, bits, within, ref_logprob = TS.i32, TS.bits, TL.within, TL.ref_logprob
GUARD = 8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------ kernel level
D, V, COUNTS = 64, 96, (5, 12)
NTOT = V + sum(COUNTS)                                                # 113: block 7 holds column 112 alone
EOS, EOS2 = 37, 41
PEN = 1.3
START, FACTOR, T_DECAY = 2, 1.3, 6
MODE_TABLE = [0, 1, 0, 2, 0, 3, 0, 0]                                 # step 1 text only, 3 own patches only, 5 EOS forced
STEPS = [0, 1, 2, 3, 4, 5, 7]                                         # both sides of START (2 itself: no edit yet; 3: EOS masked), 7: past the decay table


def guarded(n, dtype=torch.float32):
    """an n-element buffer of NaN / -5 between two runs of guard words → (flat, view)"""
    g, fill = (12345.0, float("nan")) if dtype == torch.float32 else (12345, -5)
    flat = torch.full((2 * GUARD + n,), g, device="cuda", dtype=dtype)
    flat[GUARD: GUARD + n] = fill
    return flat, flat[GUARD: GUARD + n]


def guards_ok(flat):
    g = 12345.0 if flat.dtype == torch.float32 else 12345
    return bool((flat[:GUARD] == g).all()) and bool((flat[-GUARD:] == g).all())


@pytest.fixture(scope="module")
def problem():
    """per (B, dt): operands, the parent head's penalty-free rows per mode (computed once, left unchanged), seen / ban bitmaps, bias, table"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops
    from padt_amd.generation import decay_table
    out = {}
    for B in (2, 17):
        for dt in (BF, F16):
            counts = list(COUNTS) + [0] * (B - 2)
            E, P, h, off = TS.head_problem(B, V, counts, D, dt, seed=700 + B)
            g = torch.Generator().manual_seed(900 + B)
            words = (NTOT + 31) // 32
            seen_b = torch.rand(B, NTOT, generator=g) < 0.3
            ban_b = torch.rand(B, NTOT, generator=g) < 0.1
            bias = torch.zeros(NTOT)
            pick = torch.randperm(NTOT, generator=g)[:48]
            bias[pick] = torch.randn(48, generator=g) * 6                # positive and negative, larger than most logits: signs flip under the penalty
            bias[[3, 20, 95]] = -INF                                      # text bans
            bias[[0, 15, 16, EOS]] = torch.tensor([4.0, -4.0, 2.5, -1.75])
            bias[[V, V + 4, V + 5, V + 16]] = torch.tensor([3.0, -INF, 9.0, 5.5])      # row 0's first / last patch, row 1's first / last (column 112)
            seen_b[:, [0, 15, EOS, V + 16, V]] = True                    # biased AND penalised columns
            ban_b[:, [EOS, EOS2, V + 16, V, 0]] = False
            ban_b[0, EOS2] = True                                         # a banned EOS column stays -inf under the decay
            ban_b[1, 16] = True

            def bitmap(m):
                w = torch.zeros(B, words * 32, dtype=torch.int64)
                w[:, :NTOT] = m.long()
                packed = (w.view(B, words, 32) << torch.arange(32)).sum(-1)             # bit c of row b: column c, in [0, 2^32)
                return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32).cuda()
            base = {}
            for mode in (0, 1, 2, 3):                                     # the parent head: masked, penalty-free, unbanned
                lg = torch.full((B, NTOT), float("nan"), device="cuda")
                nblk = ops.vrt_head_nblk(V, P.shape[0])
                ops.vrt_head(h, E, P, i32(off), torch.empty(nblk * B, device="cuda"), torch.empty(nblk * B, dtype=torch.int32, device="cuda"), EOS,
                             mode_table=i32([mode]), step=i32([0]), logits=lg)
                base[mode] = lg.cpu()
            assert bool((base[0][0, V + 5:] == -INF).all()) and bool(torch.isfinite(base[0][1, V + 5:]).all())      # another row's patches are masked
            out[(B, dt)] = types.SimpleNamespace(B=B, E=E, P=P, h=h, off=off, seen_b=seen_b, ban_b=ban_b, seen=bitmap(seen_b), ban=bitmap(ban_b),
                                                 bias=bias, bias_d=bias.cuda(), decay=decay_table((START, FACTOR), T_DECAY), base=base,
                                                 cfg=ops.gen_cfg_tensor(PEN, (EOS, EOS2), "cuda"))
            out[(B, dt)].decay_d = out[(B, dt)].decay.cuda()
    return out


def run(ops, p, packed, head, step, on=True, with_ban=True, old=False):
    """one launch of padt_vrt_head_bias (old: of the entry point it must equal with null pointers) + the bookkeeping kernel, every output
    between guard words; head: plain / lse / probe"""
    B = p.B
    nblk = ops.vrt_head_nblk(V, p.P.shape[0])
    r = types.SimpleNamespace(nblk=nblk, step=step)
    fl = {}
    fl["pv"], r.pv = guarded(nblk * B)
    fl["pi"], r.pi = guarded(nblk * B, torch.int32)
    fl["lg"], lg = guarded(B * NTOT)
    r.lg = lg.view(B, NTOT)
    fl["ps"], r.ps = guarded(nblk * B)
    fl["probe"], r.probe = guarded(B)
    t_max = 8
    fl["lp"], lp = guarded(B * t_max)
    r.lp = lp.view(B, t_max)
    st = i32([step])
    # the forced column of row b at this step: biased text, EOS, own patches (first / the lone column of the last block), a -inf bias, free
    cols = [0, EOS, V, V + 16, 3, -1, 15, EOS2]
    forced = [[cols[(b + s) % len(cols)] for s in range(t_max)] for b in range(B)]         # a column outside the row's own patches: -inf
    r.forced = torch.tensor(forced)
    tab = i32(forced)
    hin, kw = p.h, dict(mode_table=i32(MODE_TABLE), step=st, logits=r.lg, gen_cfg=p.cfg, seen=p.seen, ban=p.ban if with_ban else None)
    if packed:
        hin = torch.zeros((B + 15) // 16 * 16, D, device="cuda", dtype=p.h.dtype)
        ops.pack_rows(p.h, hin, B, to_packed=True)
        kw.update(table_packed=ops.pack_weight(p.E), rows=B)
    args = (hin, p.E, p.P, i32(p.off), r.pv, r.pi, EOS)
    if old:
        if head == "probe":
            ops.vrt_head_probe(*args, r.ps, tab, r.probe, **kw)
        else:
            ops.vrt_head(*args, part_sum=r.ps if head == "lse" else None, **kw)
    else:
        ops.vrt_head_bias(*args, bias=p.bias_d if on else None, decay=p.decay_d if on else None, part_sum=None if head == "plain" else r.ps,
                          forced=tab if head == "probe" else None, probe_val=r.probe if head == "probe" else None, **kw)
    if head != "plain":                                               # the fold of the LSE partials: padt_greedy_step_lp
        hid = torch.zeros(B, 8, device="cuda", dtype=BF)
        z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
        r.tok = torch.full((B, t_max), -9, dtype=torch.int64, device="cuda")
        ops.greedy_step(r.pv, r.pi, nblk, hid, torch.zeros(t_max, B, 8, device="cuda", dtype=BF), torch.ones(B, dtype=torch.int32, device="cuda"),
                        r.tok, torch.zeros(B, dtype=torch.int64, device="cuda"), st.clone(), z(B), z(B), z(3, B), EOS, PAD, gen_cfg=p.cfg,
                        part_sum=r.ps, logprobs=r.lp)
    torch.cuda.synchronize()
    for name, f in fl.items():
        assert guards_ok(f), f"guard words around {name} overwritten"
    return r


def specification(p, step, with_ban=True):
    from padt_amd.generation import score_bias_row
    a_t = float(p.decay[step]) if step < T_DECAY else 0.0
    return score_bias_row(p.base[MODE_TABLE[step]], bias=p.bias, penalty=PEN, seen=p.seen_b, banned=p.ban_b if with_ban else None,
                          eos_ids=(EOS, EOS2), a_t=a_t)


def first_argmax(pv, pi, nblk, B):
    """the partials [nblk][B] reduced as padt_greedy_step reduces them: the largest value, ties to the lowest column"""
    pv, pi = pv.view(nblk, B).cpu(), pi.view(nblk, B).cpu()
    best = pv.max(0).values
    idx = torch.where(pv == best[None], pi, torch.full_like(pi, 2 ** 31 - 1)).min(0).values
    return best, idx


@X16
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("B", [2, 17])
@pytest.mark.parametrize("head", ["plain", "lse", "probe"])
def test_head_bias_is_the_specification_bit_for_bit(ops, problem, dt, packed, B, head):
    p = problem[(B, dt)]
    edited, worst = 0, 0.0
    for step in STEPS:
        for with_ban in ((True, False) if step == 3 else (True,)):
            r = run(ops, p, packed, head, step, with_ban=with_ban)
            want = specification(p, step, with_ban)
            got = r.lg.cpu()
            assert not bool(torch.isnan(got).any()) and torch.equal(bits(got), bits(want)), f"step {step}: the written row is not the specification"
            # the partials reduce to the row's first arg-max
            best, idx = first_argmax(r.pv, r.pi, r.nblk, B)
            wbest = want.max(-1).values
            live = torch.isfinite(wbest)                              # the own-patches-only step leaves a row without patches no candidate
            assert bool(live[:2].all()) and (bool(live.all()) or MODE_TABLE[step] == 2)
            widx = torch.stack([(want[b] == wbest[b]).nonzero()[0, 0] for b in range(B)])
            assert torch.equal(bits(best), bits(wbest)) and torch.equal(idx.long()[live], widx[live]), \
                f"step {step}: partials do not reduce to the first arg-max"
            if head != "plain":                                       # the LSE partials fold to the row's log-softmax at the selected token
                assert torch.equal(r.tok[:, step].cpu()[live], widx[live])
                worst = max(worst, within(r.lp[:, step].cpu(), ref_logprob(want, widx)))
            if head == "probe":                                       # the probe value is the row's value at the forced column
                col = r.forced[:, step]
                has = col >= 0
                assert torch.equal(bits(r.probe.cpu()[has]), bits(want[torch.arange(B)[has], col[has]])), f"step {step}: probe_val"
                assert bool(torch.isnan(r.probe.cpu()[~has]).all()), "a free row's probe_val was written"
            else:
                assert bool(torch.isnan(r.probe).all())
            if step in (0, 7):                                        # the decay changes nothing there; later it does
                off_decay = run(ops, types.SimpleNamespace(**dict(vars(p), decay_d=torch.zeros_like(p.decay_d))), packed, head, step)
                assert torch.equal(bits(off_decay.lg), bits(r.lg))
            edited += int(not torch.equal(want[:, EOS], specification(types.SimpleNamespace(**dict(vars(p), decay=torch.zeros(T_DECAY))), step, with_ban)[:, EOS]))
    assert edited >= 2, "precondition: the decay edits the EOS column at the steps past `start`"
    want3 = specification(p, 3)
    assert want3[0, EOS2] == -INF and not bool(torch.isnan(want3).any())                  # the banned EOS column: -inf, not HF's NaN
    print(f"\n[head_bias {head} B={B} packed={packed} {dt}] largest |LSE fold - fp64 log-softmax| {worst:.3e}")


@X16
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("B", [2, 17])
def test_null_pointers_are_the_older_entry_points_bit_for_bit(ops, problem, dt, packed, B):
    p = problem[(B, dt)]
    for head in ("plain", "lse", "probe"):
        for with_ban in (False, True):                                # padt_vrt_head / _ban / _lse / _probe
            for step in (1, 5):
                a = run(ops, p, packed, head, step, on=False, with_ban=with_ban)
                b = run(ops, p, packed, head, step, with_ban=with_ban, old=True)
                for name in ("pv", "pi", "lg", "ps", "probe", "lp"):
                    x, y = getattr(a, name), getattr(b, name)
                    assert torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y) if y.dtype == torch.float32 else y), (head, with_ban, step, name)
    on = run(ops, p, packed, "lse", 3)
    assert not torch.equal(bits(on.lg), bits(run(ops, p, packed, "lse", 3, on=False).lg)), "precondition: the bias changes the row"


def test_entry_point_validates_its_arguments(ops):
    from padt_amd._lib import load
    lib = load()
    P_ = 4096                                                         # fake non-null pointers: the calls are refused on the host
    call = lambda fn, part_sum=P_, forced=0, t=0, probe=0, step=P_, bias=P_, decay=P_, t_decay=4, batch=2: fn(
        0, P_, 64, P_, 64, P_, 4, P_, 0, step, 0, 0, P_, P_, batch, 64, 1, 0, 0, 0, 0, 0, 0, part_sum, forced, t, probe, bias, decay, t_decay)
    for fn in (lib.padt_vrt_head_bias, lib.padt_vrt_head_bias_f16):
        for bad in (dict(step=0), dict(t_decay=0), dict(forced=P_, t=4, probe=0), dict(forced=P_, t=0, probe=P_), dict(forced=P_, t=4, probe=P_, part_sum=0),
                    dict(forced=P_, t=4, probe=P_, step=0, decay=0)):
            assert call(fn, **bad) == -1 and b"padt_vrt_head_bias" in lib.padt_last_error(), bad
        assert call(fn, batch=0, step=0) == 0


# ------------------------------------------------------------------------------------------------------------ end to end
T_NEW, SCHED, TEXT = TL.T_NEW, TL.SCHED, TL.TEXT


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model()
    return cfg, U, model, TL.two_ragged(cfg, U)


def hidden_bits(out):
    h = out.hidden_states.last_layer_rows()
    return h.view(torch.int16 if h.element_size() == 2 else torch.int32)


def assert_same_run(a, b, scores=True):
    assert torch.equal(a.sequences, b.sequences), "sequences differ"
    assert torch.equal(hidden_bits(a), hidden_bits(b)), "hidden rows differ"
    if scores:
        assert len(a.scores) == len(b.scores) > 0
        for t, (x, y) in enumerate(zip(a.scores, b.scores)):
            assert not bool(torch.isnan(x).any()) and torch.equal(x, y), f"scores[{t}] differ"


def text_bias(model, cfg, kw, gen):
    """a logit_bias that changes the run: the plain run's first tokens banned or pushed down, a few other ids pushed up"""
    L = kw["input_ids"].shape[1]
    tok = model.generate(**gen, **kw).sequences[:, L:].cpu()
    lb = {21: 7.25, 22: 5.0, 1500: 3.125, cfg.eos_token_id: -2.0}
    lb[int(tok[1, 1])] = -6.5
    lb[int(tok[0, 0])] = -INF
    return lb, tok


def hf_sequence_bias(lb):
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    return SequenceBiasLogitsProcessor({(k,): v for k, v in lb.items()})


LB_MODES = {
    "greedy": dict(),
    "eager_steps": dict(use_graph=False),
    "sampling": dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=11),
    "schedule_and_bans": dict(schedule=SCHED, no_repeat_ngram_size=2, suppress_tokens=[22]),
}


@pytest.mark.parametrize("mode", list(LB_MODES))
def test_logit_bias_is_hfs_sequence_bias_on_the_hooked_loop(setup, mode):
    cfg, U, model, kw = setup
    gen = dict(dict(max_new_tokens=T_NEW, schedule=TEXT, output_scores=True, repetition_penalty=1.0), **LB_MODES[mode])
    lb, plain_tok = text_bias(model, cfg, kw, gen)
    got = model.generate(logit_bias=lb, **gen, **kw)
    assert got.past_key_values.mode.bias and not got.past_key_values.mode.processors
    hooked = model.generate(logits_processor=[hf_sequence_bias(lb)], **gen, **kw)
    assert hooked.past_key_values.mode.processors and not hooked.past_key_values.mode.bias
    assert_same_run(got, hooked)
    L = kw["input_ids"].shape[1]
    assert not torch.equal(got.sequences[:, L:].cpu(), plain_tok), "precondition: the bias changes the run"
    assert bool((got.scores[0][:, int(plain_tok[0, 0])] == -INF).all())
    as_list = model.generate(logit_bias=[[k, v] for k, v in lb.items()], **gen, **kw)      # the other spelling: the same options, the same run
    assert_same_run(got, as_list)


def test_logit_bias_token_and_top_logprobs(setup):
    cfg, U, model, kw = setup
    gen = dict(max_new_tokens=T_NEW, schedule=TEXT)
    lb, _ = text_bias(model, cfg, kw, gen)
    L = kw["input_ids"].shape[1]
    flagged = model.generate(logit_bias=lb, output_token_logprobs=True, **gen, **kw)      # the fused LSE path: no row in memory
    scored = model.generate(logit_bias=lb, output_scores=True, top_logprobs=3, output_token_logprobs=True, **gen, **kw)
    hooked = model.generate(logits_processor=[hf_sequence_bias(lb)], output_scores=True, top_logprobs=3, output_token_logprobs=True, **gen, **kw)
    assert flagged.scores is None and torch.equal(flagged.sequences, scored.sequences)
    assert_same_run(scored, hooked)
    tok = scored.sequences[:, L:].cpu()
    ref = torch.stack([ref_logprob(scored.scores[t], tok[:, t]) for t in range(tok.shape[1])], 1)
    d = max(within(flagged.token_logprobs, ref), within(scored.token_logprobs, ref), within(hooked.token_logprobs, ref))
    assert torch.equal(scored.top_token_ids, hooked.top_token_ids) and torch.equal(bits(scored.top_logprobs), bits(hooked.top_logprobs))
    assert torch.equal(scored.top_token_ids[:, :, 0].cpu(), tok)
    print(f"\n[logit_bias log-probs] largest |token_logprobs - log_softmax(scores)| {d:.3e}")


def test_logit_bias_reference_precision():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model(precision="reference")
    kw = TL.two_ragged(cfg, U)
    gen = dict(max_new_tokens=T_NEW, schedule=TEXT, output_scores=True)
    lb, plain_tok = text_bias(model, cfg, kw, gen)
    got = model.generate(logit_bias=lb, **gen, **kw)
    assert got.past_key_values.mode.bias and got.past_key_values.mode.reference
    assert_same_run(got, model.generate(logits_processor=[hf_sequence_bias(lb)], **gen, **kw))
    assert not torch.equal(got.sequences[:, kw["input_ids"].shape[1]:].cpu(), plain_tok)


def make_processor(cfg, U):
    import padt_amd
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 64), 2)
    proc.model_embed_token_size = cfg.vocab_size
    return proc


def test_merged_decode_group_with_equal_options_and_separate_groups_otherwise(setup):
    cfg, U, model, _ = setup
    from padt_amd import pipeline
    proc = make_processor(cfg, U)
    batches = []
    for s, g in enumerate([[[1, 8, 8], [1, 10, 12]], [[1, 6, 10], [1, 8, 8]]]):
        grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5 + 3 * s, n_post=7, seed=100 + s, ragged=True)
        batches.append((ids.cuda(), am.cuda(), pix.cuda(), grid))
    T = 10
    sched = ["t"] * 3 + ["v"] * 4 + ["t"] * 2 + ["e"]
    lb = {21: 7.25, 22: 5.0, 30: -INF}
    pbs = []
    for g in ([[1, 8, 8], [1, 10, 12]], [[1, 6, 10], [1, 8, 8]]):                         # each batch its own patch prior: a window per sample
        pb = []
        for _, hh, ww in g:
            m = torch.full((hh // 2, ww // 2), -INF)
            m[1:3, 0:2] = torch.tensor([[0.0, 1.5], [-2.0, 0.25]])
            pb.append(m)
        pbs.append(pb)
    gen = dict(max_new_tokens=T, schedule=sched, output_token_logprobs=True, logit_bias=lb, exponential_decay_length_penalty=(1, 1.5))
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], patch_bias=pb, **gen) for b, pb in zip(batches, pbs)]
    plain = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], max_new_tokens=T, schedule=sched) for b in batches]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b, pb in zip(batches, pbs):
        got += runner.submit(b[0].clone(), *b[1:], patch_bias=pb, **gen)
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2, "batches with equal options share a decode group"
    for (d0, c0, l0, v0), (d1, c1, l1, v1), (_, cp, _, vp) in zip(alone, got, plain):
        assert c0 == c1 and v0 == v1, "tokens of the merged group differ from the batch alone"
        assert torch.equal(bits(d0["token_logprobs"]), bits(d1["token_logprobs"]))
        assert (c0, v0) != (cp, vp), "precondition: the edits change the batch's run"
    # another logit_bias / decay, or a patch_bias on one batch only: groups of their own
    for other in (dict(logit_bias={21: 7.0}), dict(exponential_decay_length_penalty=(1, 1.25)), dict(patch_bias=None)):
        runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
        out = runner.submit(batches[0][0].clone(), *batches[0][1:], patch_bias=pbs[0], **gen)
        out += runner.submit(batches[1][0].clone(), *batches[1][1:], **dict(dict(gen, patch_bias=pbs[1]), **other))
        out += runner.flush()
        assert runner.n_groups == 2 and len(out) == 2, other
        assert out[0][1] == alone[0][1] and out[0][3] == alone[0][3]


# ---- patch_bias
def regions(grids):
    """per sample: a (h/2, w/2) map, -inf outside a window, a graded prior inside"""
    out = []
    for b, (_, h, w) in enumerate(grids):
        m = torch.full((h // 2, w // 2), -INF)
        m[b: b + 2, 1: 4] = torch.tensor([[0.0, 2.0, -1.5], [0.5, 0.0, 3.0]])
        out.append(m)
    return out


def patch_offsets(grids):
    off = [0]
    for _, h, w in grids:
        off.append(off[-1] + (h // 2) * (w // 2))
    return off


def add_patch_vector(cfg, grids, maps):
    """the hooked loop's processor: adds the same values at every row's own patch columns"""
    off = patch_offsets(grids)

    def proc(input_ids, scores):
        add = torch.zeros_like(scores)
        for b, m in enumerate(maps):
            if m is not None:
                add[b, cfg.vocab_size + off[b]: cfg.vocab_size + off[b + 1]] = m.reshape(-1).to(scores.device)
        return scores + add
    return proc


def check_region_run(cfg, out, scored_rows, grids, maps, L, sched):
    off = patch_offsets(grids)
    V_ = cfg.vocab_size
    tok = out.sequences[:, L:].cpu()
    n_vrt = 0
    for b, m in enumerate(maps):
        inside = torch.isfinite(m.reshape(-1))
        for t in range(tok.shape[1]):
            if int(tok[b, t]) >= V_:
                j = int(tok[b, t]) - V_ - off[b]
                assert 0 <= j < inside.numel() and bool(inside[j]), f"row {b} step {t}: VRT id {int(tok[b, t])} lies outside the region"
                n_vrt += 1
            plp = out.patch_logprobs[b, t, : inside.numel()].cpu()
            assert bool((plp[~inside] == -INF).all()), "patch_logprobs outside the region must be -inf"
            row = scored_rows[t][b].cpu().double()
            mass = torch.softmax(row, -1)[V_ + off[b]: V_ + off[b + 1]].sum()
            # each log-prob is within 5e-6 + 2^-22 |ref| of the row's log-softmax (within()): 5e-6 relative per probability, so 5e-6 x mass
            # <= 5e-6 on the sum, plus the fp32 roundings of up to 30 terms — 1e-5 covers both
            assert abs(float(plp.double().exp().sum() - mass)) <= 1e-5, f"row {b} step {t}: patch_logprobs do not sum to the row's VRT mass"
            if sched[t] == "v":
                assert abs(float(mass) - 1.0) <= 1e-5 and bool(torch.isfinite(plp[inside]).all())
    assert n_vrt == len(maps) * sum(s == "v" for s in sched), "precondition: every VRT step emitted a VRT id"


def test_patch_bias_keeps_the_pointers_inside_the_region(setup):
    cfg, U, model, kw = setup
    grids = kw["image_grid_thw"].tolist()
    maps = regions(grids)
    L = kw["input_ids"].shape[1]
    gen = dict(max_new_tokens=T_NEW, schedule=SCHED, output_scores=True, output_patch_logprobs=True)
    plain = model.generate(**gen, **kw)
    got = model.generate(patch_bias=maps, **gen, **kw)
    assert got.past_key_values.mode.bias
    hooked = model.generate(logits_processor=[add_patch_vector(cfg, grids, maps)], **gen, **kw)
    assert_same_run(got, hooked)
    assert torch.equal(bits(got.patch_logprobs), bits(hooked.patch_logprobs))
    assert not torch.equal(got.sequences, plain.sequences), "precondition: the plain run points outside the region"
    check_region_run(cfg, got, got.scores, grids, maps, L, SCHED)
    flat = model.generate(patch_bias=[maps[0].reshape(-1), maps[1].reshape(-1).tolist()], **gen, **kw)      # 1-D spellings: the same run
    assert_same_run(got, flat)
    one = model.generate(patch_bias=[None, maps[1]], **gen, **kw)                         # a row without an entry keeps its plain scores
    assert torch.equal(one.sequences[0], plain.sequences[0]) and torch.equal(one.sequences[1], got.sequences[1])
    for t in range(len(one.scores)):
        assert torch.equal(one.scores[t][0], plain.scores[t][0]) and torch.equal(one.scores[t][1], got.scores[t][1])
    with pytest.raises(ValueError, match="patch_bias.*row 1"):
        model.generate(patch_bias=[None, torch.zeros(15)], **gen, **kw)
    with pytest.raises(ValueError, match="patch_bias.*row 0.*map"):
        model.generate(patch_bias=[torch.zeros(6, 5), None], **gen, **kw)


def test_patch_bias_with_image_index_each_query_its_own_region(setup):
    cfg, U, model, _ = setup
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8]], n_pre=6, n_post=9, seed=93)
    ids = ids.repeat(2, 1)
    ids[1, -4:] = torch.tensor([5, 6, 7, 8])
    kw = dict(input_ids=ids.cuda(), attention_mask=am.repeat(2, 1).cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, image_index=[0, 0])
    grids = grid[[0, 0]].tolist()
    a, b = torch.full((4, 4), -INF), torch.full((4, 4), -INF)
    a[0:2, 0:2], b[2:4, 1:4] = 0.0, torch.tensor([[0.0, 1.0, 2.0], [0.5, 0.0, -1.0]])
    assert not bool((torch.isfinite(a) & torch.isfinite(b)).any())                       # disjoint regions on the one image
    gen = dict(max_new_tokens=T_NEW, schedule=SCHED, output_scores=True, output_patch_logprobs=True)
    got = model.generate(patch_bias=[a, b], **gen, **kw)
    check_region_run(cfg, got, got.scores, grids, [a, b], ids.shape[1], SCHED)
    assert_same_run(got, model.generate(logits_processor=[add_patch_vector(cfg, grids, [a, b])], **gen, **kw))


# ---- the decay
def test_decay_is_hfs_exponential_decay_length_penalty_on_the_hooked_loop(setup):
    from transformers.generation.logits_process import ExponentialDecayLengthPenalty
    cfg, U, model, kw = setup
    L = kw["input_ids"].shape[1]
    eos = [cfg.eos_token_id, 11]
    gen = dict(max_new_tokens=T_NEW, schedule=TEXT, output_scores=True, eos_token_id=eos)
    plain = model.generate(**gen, **kw)
    assert plain.sequences.shape[1] == L + T_NEW and not bool(torch.isin(plain.sequences[:, L:].cpu(), torch.tensor(eos)).any()), \
        "precondition: random weights do not emit EOS on their own"
    chosen = None
    for start, factor in ((2, 2.0), (2, 4.0), (1, 16.0), (0, 64.0)):                      # judged on the HF run itself
        hf = model.generate(logits_processor=[ExponentialDecayLengthPenalty((start, factor), eos, L)], **gen, **kw)
        tok = hf.sequences[:, L:].cpu()
        ends = [int(torch.isin(tok[b], torch.tensor(eos)).nonzero()[0]) if bool(torch.isin(tok[b], torch.tensor(eos)).any()) else None for b in range(2)]
        if any(e is not None and start < e < T_NEW - 1 for e in ends):
            chosen = (start, factor, hf, ends)
            break
    assert chosen is not None, "precondition: no candidate (start, factor) ends a row of the HF run after `start` and before max_new_tokens"
    start, factor, hf, ends = chosen
    got = model.generate(exponential_decay_length_penalty=(start, factor), **gen, **kw)
    assert got.past_key_values.mode.bias and not got.past_key_values.mode.processors
    assert_same_run(got, hf)
    cfgd = model.generate(generation_config=dict(exponential_decay_length_penalty=[start, factor]), **gen, **kw)      # ... from a generation config
    assert_same_run(got, cfgd)
    lp = model.generate(exponential_decay_length_penalty=(start, factor), output_token_logprobs=True, **dict(gen, output_scores=False), **kw)
    assert torch.equal(lp.sequences, got.sequences)
    tok = got.sequences[:, L:].cpu()
    ref = torch.stack([ref_logprob(got.scores[t], tok[:, t]) for t in range(tok.shape[1])], 1)
    after = torch.zeros_like(tok, dtype=torch.bool)
    for b, e in enumerate(ends):
        if e is not None:
            after[b, e + 1:] = True
    d = within(lp.token_logprobs.cpu()[~after], ref[~after])
    print(f"\n[decay] (start, factor) = ({start}, {factor}); rows end at {ends}; largest |token_logprobs - log_softmax(scores)| {d:.3e}")


def test_decay_on_a_session_longer_than_the_call(setup):
    """the lane's session keeps the longest t_max it has seen: a decay validated for 12 steps meets a 1024-step table, whose later powers
    (4 ** 1000) do not fit a double"""
    from transformers.generation.logits_process import ExponentialDecayLengthPenalty
    cfg, U, model, kw = setup
    L = kw["input_ids"].shape[1]
    long_call = model.generate(max_new_tokens=1024, schedule=["t", "e"], **kw)            # both rows end at the second step
    sess = long_call.past_key_values
    assert sess.t_max >= 1024 and long_call.sequences.shape[1] == L + 2
    gen = dict(max_new_tokens=T_NEW, schedule=TEXT, output_scores=True)
    got = model.generate(exponential_decay_length_penalty=(2, 4.0), **gen, **kw)
    assert got.past_key_values is sess and sess.t_max >= 1024 and sess.mode.bias
    assert bool(torch.isfinite(sess.decay).all()) and bool((sess.decay[T_NEW:] == 0).all()) and bool((sess.decay[3:T_NEW] > 0).all())
    hf = model.generate(logits_processor=[ExponentialDecayLengthPenalty((2, 4.0), [cfg.eos_token_id], L)], **gen, **kw)
    assert_same_run(got, hf)
    assert got.sequences.shape[1] < L + T_NEW, "precondition: the decay ends the run early"


# ---- combinations
def test_a_forced_token_at_a_biased_column_is_scored_at_the_biased_value(setup):
    cfg, U, model, kw = setup
    L = kw["input_ids"].shape[1]
    table = torch.tensor([[25, 26, 27, 28], [35, 36, 37, 38]])
    lb = {26: -3.0, 37: 2.5, 28: -INF}
    gen = dict(max_new_tokens=4, schedule=TEXT[:4], forced_tokens=table, output_token_logprobs=True)
    base = model.generate(output_scores=True, **gen, **kw)
    got = model.generate(output_scores=True, logit_bias=lb, **gen, **kw)
    fused = model.generate(logit_bias=lb, **gen, **kw)                                    # the probe head with the bias: no row in memory
    assert got.past_key_values.mode.forced and got.past_key_values.mode.bias
    assert torch.equal(got.sequences[:, L:].cpu(), table) and torch.equal(fused.sequences, got.sequences)
    add = torch.zeros(got.scores[0].shape[1])
    for k, v in lb.items():
        add[k] = v
    for t in range(4):                                                # the same forced prefix: the same hidden rows, so the rows differ by the bias alone
        assert torch.equal(got.scores[t].cpu(), base.scores[t].cpu() + add)
    ref = torch.stack([ref_logprob(got.scores[t], table[:, t]) for t in range(4)], 1)
    d = max(within(got.token_logprobs, ref), within(fused.token_logprobs, ref))
    assert float(got.token_logprobs[0, 3]) == -INF and float(fused.token_logprobs[0, 3]) == -INF
    assert float(fused.token_logprobs[0, 1]) < float(base.token_logprobs[0, 1]) and float(fused.token_logprobs[1, 2]) > float(base.token_logprobs[1, 2])
    print(f"\n[forced + bias] largest |token_logprobs - log_softmax(scores)| {d:.3e}")


def test_the_three_arguments_off_are_the_call_without_them(setup):
    from padt_amd.generation import DECAY_OFF, StepMode
    cfg, U, model, kw = setup
    gen = dict(max_new_tokens=T_NEW, schedule=SCHED, output_scores=True, output_token_logprobs=True)
    base = model.generate(**gen, **kw)
    sess = base.past_key_values
    mode, n_graphs = sess.mode, len(sess.graphs)
    assert mode == StepMode(keep_scores=True, token_logprobs=True) and not mode.bias
    for off in (dict(logit_bias=None, patch_bias=None, exponential_decay_length_penalty=None),
                dict(logit_bias={}, patch_bias=[None, None], exponential_decay_length_penalty=DECAY_OFF), dict(logit_bias={21: 0.0})):
        out = model.generate(**off, **gen, **kw)
        assert_same_run(base, out)
        assert torch.equal(bits(base.token_logprobs), bits(out.token_logprobs))
        assert out.past_key_values is sess and sess.mode == mode and len(sess.graphs) == n_graphs, "an off call must launch the parent's step mode"
    on = model.generate(logit_bias={21: 7.25}, **gen, **kw)
    assert sess.mode == mode._replace(bias=True) and len(sess.graphs) == n_graphs + 1
    model.generate(logit_bias={22: -1.0}, exponential_decay_length_penalty=(1, 1.5), patch_bias=[None, torch.zeros(16)], **gen, **kw)
    assert len(sess.graphs) == n_graphs + 1, "one captured graph serves every value"
    again = model.generate(**gen, **kw)                                # ... and nothing of an earlier call's bias is left behind
    assert_same_run(base, again)
    assert not torch.equal(on.sequences, base.sequences) or not torch.equal(on.scores[0], base.scores[0])
    with pytest.raises(NotImplementedError, match="output_logits"):
        model.generate(logit_bias={21: 7.25}, output_logits=True, max_new_tokens=4, **kw)
