"""generate(forced_tokens=F): the caller's completion tokens, forced inside the decode loop, and their log-probs.

Kernel level: padt_vrt_head_probe + padt_forced_step (the fused path) against padt_vrt_head_lse + padt_greedy_step_lp on the same inputs — the
partials, part_sum and logits bit for bit, the free rows' tokens and log-prob bits, the forced rows' log-probs against fp64 log_softmax of the
row the SAME launch wrote — with the forced column where indexing can go wrong, rows that are forced, free and finished, NaN-filled outputs and
guard words around probe_val / part_sum / logprobs; padt_forced_override on the row path.  End to end (the small synthetic model, two ragged
samples): forcing a run's own output must return that run bit for bit in every mode; an off-policy table against the call's own scores and
against the fp32 oracle.

The kernel-level bound is test_token_logprobs_gpu.within(): 5e-6 + 2^-22 |ref|, derived there for (log Σ exp) of the same logit bits; the forced
log-prob adds ONE fp32 subtraction, (probe - M) - log S: probe - M is exact or rounds once (2^-24 |probe - M|) and the outer subtraction rounds
once more (2^-24 |ref|) — together 2^-23 |ref| at most when |probe - M| ~ |ref|, inside the 2^-22 |ref| term.  Every test prints the largest
difference it saw.
"""
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
i32, bits, within, ref_logprob, guarded, guards_ok = TS.i32, TS.bits, TL.within, TL.ref_logprob, TL.guarded, TL.guards_ok


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def forced_fused(ops, h, E, P, off, packed, table, lp=True, t_max=3, step=1, eos=-3, mode_table=None, gen_cfg=None, seen=None, ban=None, unf=None):
    """TL.fused with the forced table: the probe head (the plain head when lp is off) and padt_forced_step, on NaN / garbage filled outputs"""
    B, D = h.shape
    V, NP = E.shape[0], P.shape[0]
    nblk = ops.vrt_head_nblk(V, NP)
    r = types.SimpleNamespace(nblk=nblk, t_max=t_max, step=step)
    r.pv = torch.full((nblk * B,), float("nan"), device="cuda")
    r.pi = torch.full((nblk * B,), -5, dtype=torch.int32, device="cuda")
    r.lg = torch.full((B, V + NP), float("nan"), device="cuda")
    r.ps_flat, r.ps = guarded(nblk * B)
    r.lp_flat, lpb = guarded(B * t_max)
    r.lp = lpb.view(B, t_max)
    r.pr_flat, r.probe = guarded(B)
    st = i32([step])
    tab = i32(table)
    hin, kw = h, dict(mode_table=mode_table, logits=r.lg, gen_cfg=gen_cfg, seen=seen, ban=ban)
    if packed:
        hin = torch.zeros((B + 15) // 16 * 16, D, device="cuda", dtype=h.dtype)
        ops.pack_rows(h, hin, B, to_packed=True)
        kw.update(table_packed=ops.pack_weight(E), rows=B)
    if lp:
        ops.vrt_head_probe(hin, E, P, i32(off), r.pv, r.pi, eos, r.ps, tab, r.probe, st, **kw)
    else:
        ops.vrt_head(hin, E, P, i32(off), r.pv, r.pi, eos, step=st if mode_table is not None else None, **kw)
    hid = torch.zeros(B, 8, device="cuda", dtype=BF)
    r.unf = torch.ones(B, dtype=torch.int32, device="cuda") if unf is None else i32(unf)
    r.tok = torch.full((B, t_max), -9, dtype=torch.int64, device="cuda")
    r.cur = torch.full((B,), -9, dtype=torch.int64, device="cuda")
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    gk = dict(part_sum=r.ps, logprobs=r.lp, probe_val=r.probe) if lp else {}
    ops.forced_step(r.pv, r.pi, nblk, hid, torch.zeros(t_max, B, 8, device="cuda", dtype=BF), r.unf, r.tok, r.cur, st, z(B), z(B), z(3, B),
                    eos, PAD, tab, V + NP, gen_cfg=gen_cfg, seen=seen, **gk)
    torch.cuda.synchronize()
    assert int(st) == step + 1
    assert guards_ok(r.ps_flat) and guards_ok(r.lp_flat) and guards_ok(r.pr_flat), "guard words around part_sum / logprobs / probe_val overwritten"
    return r


def same_head(a, b):
    return (torch.equal(bits(a.pv), bits(b.pv)) and torch.equal(a.pi, b.pi) and torch.equal(bits(a.lg), bits(b.lg))
            and torch.equal(bits(a.ps), bits(b.ps)))


KINDS = ["col0", "blk_last", "v_last", "first_proto", "tail_last", "argmax", "free", "finished"]


def placed_table(B, V, NTOT, argmax, shift=0, width=2, col=1):
    """(table, unfinished, kinds): row b's entry at column `col` by KINDS[(b + B + shift) % 8]; the other columns hold another valid id, so
    that a kernel reading the wrong step shows"""
    table, unf, kinds = [], [], []
    for b in range(B):
        kind = KINDS[(b + B + shift) % len(KINDS)]
        f = {"col0": 0, "blk_last": 15, "v_last": V - 1, "first_proto": V, "tail_last": NTOT - 1, "argmax": int(argmax[b]), "free": -1,
             "finished": 3}[kind]
        row = [(7 + b) % V] * width
        row[col] = f
        table.append(row), unf.append(0 if kind == "finished" else 1), kinds.append(kind)
    return table, unf, kinds


# ------------------------------------------------------------------------------------------------------------ fused path
@X16
@pytest.mark.parametrize("layout", TL.FUSED_LAYOUTS)
@pytest.mark.parametrize("B", TL.FUSED_B)
def test_probe_head_and_forced_step_every_dispatch_variant(ops, dt, layout, B):
    counts, V, D = TL.fused_shape(layout, B)
    E, P, h, off = TS.head_problem(B, V, counts, D, dt, seed=3000 + B)
    NTOT = V + sum(counts)
    packed = layout == "packed"
    free = TL.fused(ops, h, E, P, off, packed)                                      # every row live and free: where the arg-max is
    for shift in range(0, len(KINDS) if B < len(KINDS) else 1, B):                  # fewer rows than placements: further launches cover the rest
        check_placements(ops, h, E, P, off, packed, free, placed_table(B, V, NTOT, free.cur.cpu(), shift), f"{layout} B={B} {dt}")


def check_placements(ops, h, E, P, off, packed, free, placed, what):
    table, unf, kinds = placed
    B, V, NTOT = h.shape[0], E.shape[0], E.shape[0] + P.shape[0]
    a = TL.fused(ops, h, E, P, off, packed, unf=unf)                                # padt_vrt_head_lse + padt_greedy_step_lp
    f = forced_fused(ops, h, E, P, off, packed, table, unf=unf)
    # (a) the head is padt_vrt_head_lse's bit for bit; the probe is the written logit of the forced column, nothing for a free row
    assert same_head(a, f), "partials / part_sum / logits of the probe head differ from padt_vrt_head_lse"
    col = torch.tensor([r[1] for r in table])
    has = col >= 0
    lg = f.lg.cpu()
    want = lg[torch.arange(B)[has], col[has]]
    assert torch.equal(bits(f.probe.cpu()[has]), bits(want)), "probe_val is not the written logit at the forced column"
    assert bool(torch.isnan(f.probe.cpu()[~has]).all()), "a free row's probe_val was written"
    # (b) tokens: the table where forced and live, padt_greedy_step_lp's elsewhere — with its log-prob bits
    live = torch.tensor(unf, dtype=torch.bool)
    forced = has & live
    tok, lp, alp = f.cur.cpu(), f.lp[:, f.step].cpu(), a.lp[:, a.step].cpu()
    assert torch.equal(tok[forced], col[forced]) and torch.equal(tok[~forced], a.cur.cpu()[~forced])
    assert torch.equal(f.tok[:, f.step].cpu(), tok) and TL.only_column_written(f)
    assert torch.equal(bits(lp[~forced]), bits(alp[~forced])) and bool((lp[~live] == 0.0).all()) and bool((tok[~live] == PAD).all())
    assert torch.equal(f.unf.cpu()[~forced], a.unf.cpu()[~forced])
    # (c) forced log-probs against fp64 log_softmax of the written row; a column outside the row's own VRT range is -inf, never NaN
    d = within(lp[forced], ref_logprob(lg[forced], col[forced])) if forced.any() else 0.0
    assert not bool(torch.isnan(lp).any())
    print(f"\n[forced {what}] largest |log-prob - fp64 reference| {d:.3e}  kinds {sorted(set(kinds))}")
    # (d) a forced arg-max carries exactly the bits of the free step
    am = torch.tensor([k == "argmax" for k in kinds])
    assert torch.equal(bits(lp[am]), bits(free.lp[:, free.step].cpu()[am])) and torch.equal(tok[am], free.cur.cpu()[am])
    # two launches: the same bits
    g = forced_fused(ops, h, E, P, off, packed, table, unf=unf)
    assert same_head(f, g) and torch.equal(bits(f.lp), bits(g.lp)) and torch.equal(bits(f.probe), bits(g.probe)) and torch.equal(f.tok, g.tok)
    # without log-probs: the plain head + forced step select the same tokens
    n = forced_fused(ops, h, E, P, off, packed, table, unf=unf, lp=False)
    assert torch.equal(n.cur, f.cur) and torch.equal(n.unf, f.unf) and torch.equal(bits(n.pv), bits(f.pv)) and bool(torch.isnan(n.lp).all())
    if B == 5:
        # *step >= n (the table is 2 wide, the token ring 3): a free step; *step >= t_max: nothing is written
        past = forced_fused(ops, h, E, P, off, packed, table, unf=unf, step=2)
        ref = TL.fused(ops, h, E, P, off, packed, unf=unf, step=2)
        assert torch.equal(past.cur, ref.cur) and torch.equal(bits(past.lp), bits(ref.lp)) and bool(torch.isnan(past.probe).all())
        wide = [r + [r[1]] * 6 for r in table]                                       # a table wider than the ring: the ring's bound holds
        for step in (3, 8):
            out = forced_fused(ops, h, E, P, off, packed, wide, unf=unf, step=step)
            assert bool(torch.isnan(out.lp).all()) and bool((out.tok == -9).all())


@X16
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
def test_forced_minus_inf_penalised_and_eos_columns(ops, dt, packed):
    B, D, eos, eos2 = 5, 64, 37, 41
    counts = TS.ragged_counts(B)                                                     # row 0 has no patches
    V = TS.vocab_for(counts, 3)
    E, P, h, off = TS.head_problem(B, V, counts, D, dt, seed=59)
    NTOT = V + sum(counts)
    words = (NTOT + 31) // 32
    cfg = ops.gen_cfg_tensor(1.3, (eos, eos2), "cuda")
    banned, pen = 50, 60
    ban = torch.zeros(B, words, dtype=torch.int32)
    ban[2, banned >> 5] = 1 << (banned & 31)
    seen = torch.zeros(B, words, dtype=torch.int32)
    seen[3, pen >> 5] = 1 << (pen & 31)
    foreign = V + off[3]                                                             # row 1 names a patch of row 3
    table = [[eos], [foreign], [banned], [pen], [eos2]]
    f = forced_fused(ops, h, E, P, off, packed, table, step=0, eos=eos, gen_cfg=cfg, seen=seen.cuda(), ban=ban.cuda())
    a = TL.fused(ops, h, E, P, off, packed, step=0, eos=eos, gen_cfg=cfg, seen=seen.cuda(), ban=ban.cuda())
    unpen = TL.fused(ops, h, E, P, off, packed, step=0, eos=eos, ban=ban.cuda())
    assert same_head(a, f)
    tok, lp, lg = f.cur.cpu(), f.lp[:, 0].cpu(), f.lg.cpu()
    assert tok.tolist() == [eos, foreign, banned, pen, eos2], "a forced token was not emitted"
    assert lp[1] == -INF and lp[2] == -INF and lg[1, foreign] == -INF and lg[2, banned] == -INF
    assert not bool(torch.isnan(lp).any()) and not bool(torch.isnan(f.probe).any()) and not bool(torch.isnan(f.ps).any())
    assert lg[3, pen] != unpen.lg.cpu()[3, pen] and bits(f.probe.cpu())[3] == bits(lg[3, pen:pen + 1])[0]      # scored after the penalty
    keep = torch.tensor([0, 3, 4])
    d = within(lp[keep], ref_logprob(lg[keep], tok[keep]))
    assert f.unf.cpu().tolist() == [0, 1, 1, 1, 0], "a forced EOS (config id / gen_cfg list) must finish its row"
    # a column the mode table masks: text-only step, the row's OWN patch forced
    own = V + off[4]
    m = forced_fused(ops, h, E, P, off, packed, [[3], [-1], [3], [3], [own]], step=0, eos=eos, mode_table=i32([1, 0, 0]))
    assert int(m.cur[4]) == own and m.lp[4, 0] == -INF and not bool(torch.isnan(m.lp[:, 0]).any())
    within(m.lp[:, 0].cpu()[[0, 2, 3]], ref_logprob(m.lg.cpu()[[0, 2, 3]], torch.tensor([3, 3, 3])))
    print(f"\n[forced exact cases {dt} packed={packed}] largest |log-prob - fp64 reference| {d:.3e}")


def test_forced_token_enters_the_seen_bitmap(ops):
    B, D = 2, 64
    counts = [4, 4]
    V = 64
    E, P, h, off = TS.head_problem(B, V, counts, D, BF, seed=61)
    words = (V + 8 + 31) // 32
    seen = torch.zeros(B, words, dtype=torch.int32, device="cuda")
    cfg = ops.gen_cfg_tensor(1.3, (), "cuda")
    f = forced_fused(ops, h, E, P, off, False, [[40], [-1]], step=0, gen_cfg=cfg, seen=seen)
    s = seen.cpu()
    assert (int(s[0, 40 >> 5]) >> (40 & 31)) & 1 == 1 and int(f.cur[0]) == 40
    c = int(f.cur[1])
    assert (int(s[1, c >> 5]) >> (c & 31)) & 1 == 1 and int(s[0].ne(0).sum()) == 1


# ------------------------------------------------------------------------------------------------------------ row path
@pytest.mark.parametrize("n", [113, 1029])
def test_override_on_the_row_path(ops, n):
    g = torch.Generator().manual_seed(n)
    B, ld, t_max = 6, n + 3, 4
    x = torch.full((B, ld), float("nan"))
    x[:, :n] = torch.randn(B, n, generator=g) * 4
    x[:, :n][torch.rand(B, n, generator=g) < 0.3] = -INF
    x[0, 0], x[1, n - 1], x[2, 17], x[4, 9] = 1.0, -2.0, 0.5, -INF
    xd = x.cuda()
    unf = i32([1, 1, 1, 0, 1, 1])
    table = i32([[5, 0], [5, n - 1], [5, 17], [5, 3], [5, 9], [5, -1]])                 # read at step 1; row 3 finished, row 4 -inf, row 5 free
    st = i32([1])
    pv, pi = torch.zeros(B, device="cuda"), torch.full((B,), -5, dtype=torch.int32, device="cuda")
    ops.argmax_rows(xd, n, pv, pi, B)
    before = pi.clone()
    ops.forced_override(pi, table, st, unf, n, B)
    assert pi.tolist()[:3] == [0, n - 1, 17] and int(pi[4]) == 9 and int(pi[3]) == int(before[3]) and int(pi[5]) == int(before[5])
    flat, lp = guarded(B * t_max)
    lp = lp.view(B, t_max)
    ops.token_logprob_rows(xd, n, pi, unf, st, lp, B)
    torch.cuda.synchronize()
    got = lp[:, 1].cpu()
    assert guards_ok(flat) and got[3] == 0.0 and got[4] == -INF
    live = torch.tensor([0, 1, 2, 5])
    d = within(got[live], ref_logprob(x[live, :n], pi.cpu()[live]))
    # past the table / a negative step: nothing is overridden
    for s in (2, 7, -1):
        p2 = before.clone()
        ops.forced_override(p2, table, i32([s]), unf, n, B)
        assert torch.equal(p2, before)
    # ... and after padt_sample_token with write-back: the forced column of the WARPED row
    cfg = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=3, temperature=0.7, top_k=20, top_p=0.9, write_back=True)
    xs = x.cuda()
    ops.sample_token(xs, n, cfg, st, pv, pi, B)
    drawn = pi.clone()
    warped = xs.cpu()[:, :n]
    best = warped.argmax(-1)
    tab2 = i32([[5, int(best[0])], [5, int(drawn[1])], [5, int((warped[2] == -INF).nonzero()[0])], [5, 3], [5, -1], [5, -1]])
    ops.forced_override(pi, tab2, st, unf, n, B)
    assert int(pi[0]) == int(best[0]) and torch.equal(pi[3:], drawn[3:]), "the draw of a free / finished row was touched"
    flat2, lp2 = guarded(B * t_max)
    lp2 = lp2.view(B, t_max)
    ops.token_logprob_rows(xs, n, pi, unf, st, lp2, B)
    # ... appended by the forced bookkeeping kernel (one partial per row)
    tok = torch.full((B, t_max), -9, dtype=torch.int64, device="cuda")
    cur = torch.full((B,), -9, dtype=torch.int64, device="cuda")
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    u2 = unf.clone()
    ops.forced_step(pv, pi, 1, torch.zeros(B, 8, device="cuda", dtype=BF), torch.zeros(t_max, B, 8, device="cuda", dtype=BF), u2, tok, cur, st,
                    z(B), z(B), z(3, B), -3, PAD, tab2, n)
    torch.cuda.synchronize()
    got2 = lp2[:, 1].cpu()
    assert guards_ok(flat2) and got2[2] == -INF and got2[3] == 0.0
    live = torch.tensor([0, 1, 4, 5])
    d2 = within(got2[live], ref_logprob(warped[live], pi.cpu()[live]))
    assert cur.tolist() == [int(best[0]), int(drawn[1]), int(tab2[2, 1]), PAD, int(drawn[4]), int(drawn[5])]
    print(f"\n[forced rows n={n}] largest |log-prob - fp64 reference| arg-max {d:.3e}  warped {d2:.3e}")


def test_entry_points_validate_their_arguments(ops):
    from padt_amd._lib import load
    lib = load()
    P_ = 4096                                                      # fake non-null pointers: never dereferenced, the calls are refused on the host
    head = lambda fn, part_sum=P_, forced=P_, t=4, probe=P_, step=P_, batch=2: fn(0, P_, 64, P_, 64, P_, 4, P_, 0, step, 0, 0, P_, P_, batch, 64,
                                                                                   1, 0, 0, 0, 0, 0, 0, part_sum, forced, t, probe)
    for fn, name in ((lib.padt_vrt_head_probe, b"padt_vrt_head_probe"), (lib.padt_vrt_head_probe_f16, b"padt_vrt_head_probe")):
        for bad in (dict(part_sum=0), dict(forced=0), dict(probe=0), dict(step=0), dict(t=0)):
            assert head(fn, **bad) == -1 and name in lib.padt_last_error(), bad
        assert head(fn, batch=0, forced=0) == 0
    step = lambda ps=P_, lp=P_, forced=P_, t=4, probe=P_, n_cols=68, batch=2, D=64, st=P_: lib.padt_forced_step(
        0, P_, P_, 5, batch, D, 1, 0, 4, P_, P_, P_, st, P_, P_, P_, P_, P_, 1, 0, 0, 0, ps, lp, forced, t, probe, n_cols)
    for bad in (dict(forced=0), dict(t=0), dict(n_cols=0), dict(ps=0), dict(lp=0), dict(probe=0), dict(ps=0, lp=0), dict(D=63), dict(st=0)):
        assert step(**bad) == -1 and b"padt_forced_step" in lib.padt_last_error(), bad
    assert step(batch=0, forced=0) == 0
    over = lambda pi=P_, forced=P_, t=4, st=P_, unf=P_, n_cols=68, batch=2: lib.padt_forced_override(0, pi, forced, t, st, unf, n_cols, batch)
    for bad in (dict(pi=0), dict(forced=0), dict(t=0), dict(st=0), dict(unf=0), dict(n_cols=0)):
        assert over(**bad) == -1 and b"padt_forced_override" in lib.padt_last_error(), bad
    assert over(batch=0, pi=0) == 0


# ------------------------------------------------------------------------------------------------------------ end to end
T_NEW, SCHED = TL.T_NEW, TL.SCHED                                   # 12 steps: 5 text, 3 VRT, 3 text, EOS


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model()
    return cfg, U, model, TL.two_ragged(cfg, U)


def decode_objects(model, cfg, U, out, grid, L):
    """parseVRTintoCompletion + vl_decode on a generate output → (feats, decoded)"""
    import padt_amd
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 64), 2)
    proc.model_embed_token_size = cfg.vocab_size
    local = proc.assign_to_local_vrt_id(out.sequences.cpu().clone(), grid)[:, L:]
    _, feats, _, _, _ = padt_amd.parseVRTintoCompletion(proc, local, out["hidden_states"], torch.Tensor([False] * local.shape[0]))
    return feats, model.vl_decode(feats, out.past_image_embeds, out.past_high_res_image_embeds, grid, out.past_visual_pe)


def assert_same_run(model, cfg, U, a, b, grid, L):
    assert torch.equal(a.sequences, b.sequences), "sequences differ"
    assert torch.equal(bits(a.token_logprobs), bits(b.token_logprobs)), "token_logprobs differ"
    assert torch.equal(a.top_token_ids, b.top_token_ids) and torch.equal(bits(a.top_logprobs), bits(b.top_logprobs)), "top_* differ"
    ha, hb = a.hidden_states.last_layer_rows(), b.hidden_states.last_layer_rows()
    assert ha.dtype == hb.dtype and torch.equal(ha.view(torch.int16 if ha.element_size() == 2 else torch.int32),
                                                hb.view(torch.int16 if hb.element_size() == 2 else torch.int32)), "hidden rows differ"
    (fa, da), (fb, db) = decode_objects(model, cfg, U, a, grid, L), decode_objects(model, cfg, U, b, grid, L)
    assert [len(f) for f in fa] == [len(f) for f in fb] and sum(len(f) for f in fa) > 0, "precondition: the run decodes objects"
    for k in ("pred_boxes", "pred_score", "pred_mask"):
        assert torch.equal(da[k], db[k]), k


def replay(model, cfg, U, kw, gen, grid=None):
    """run, then force the run's own output: every returned field comes back bit for bit"""
    L = kw["input_ids"].shape[1]
    gen = dict(dict(max_new_tokens=T_NEW, schedule=SCHED, output_token_logprobs=True, top_logprobs=3), **gen)
    base = model.generate(**gen, **kw)
    again = model.generate(forced_tokens=base.sequences[:, L:], **gen, **kw)
    assert_same_run(model, cfg, U, base, again, kw["image_grid_thw"] if grid is None else grid, L)
    return base


REPLAY = {
    "captured": dict(),
    "eager_steps": dict(use_graph=False),
    "penalty_and_ngram": dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
    "sampling": dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=11),
}


@pytest.mark.parametrize("mode", list(REPLAY))
def test_forcing_a_runs_own_output_returns_the_run(setup, mode):
    cfg, U, model, kw = setup
    base = replay(model, cfg, U, kw, REPLAY[mode])
    if mode == "sampling":
        assert bool((base.token_logprobs < 0).any())


def test_replay_reference_precision():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model(precision="reference")
    replay(model, cfg, U, TL.two_ragged(cfg, U), dict())


def test_replay_with_image_index(setup):
    cfg, U, model, _ = setup
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8]], n_pre=6, n_post=9, seed=93)
    ids = ids.repeat(2, 1)
    ids[1, -4:] = torch.tensor([5, 6, 7, 8])
    kw = dict(input_ids=ids.cuda(), attention_mask=am.repeat(2, 1).cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, image_index=[0, 0])
    replay(model, cfg, U, kw, dict(), grid=grid[[0, 0]])


def test_a_forced_prefix_then_free_steps_return_the_run(setup):
    cfg, U, model, kw = setup
    L = kw["input_ids"].shape[1]
    gen = dict(max_new_tokens=T_NEW, schedule=SCHED, output_token_logprobs=True, top_logprobs=3)
    base = model.generate(**gen, **kw)
    tok = base.sequences[:, L:]
    padded = tok.clone()
    padded[:, 5:] = -1
    for table in (tok[:, :5], padded, [tok[0, :5].tolist(), tok[1, :3].tolist()]):
        again = model.generate(forced_tokens=table, **gen, **kw)
        assert_same_run(model, cfg, U, base, again, kw["image_grid_thw"], L)
    # an all-free table is the call without the argument: no forced step mode, no new graph
    sess = base.past_key_values
    n_graphs = len(sess.graphs)
    free = model.generate(forced_tokens=torch.full_like(tok, -1), **gen, **kw)
    assert_same_run(model, cfg, U, base, free, kw["image_grid_thw"], L)
    assert len(sess.graphs) == n_graphs and not sess.mode.forced


def off_policy_table(cfg, grids, T=T_NEW, sched=SCHED, eos_row=1, eos_at=9, foreign_row=0):
    """a completion that is not the model's choice: text ids below image_token_id at the text steps, each sample's own patches at the VRT
    steps, an early EOS in one row, one entry of the other sample's patch range, EOS at the last step"""
    n_m = [g[1] * g[2] // 4 for g in grids]
    off = [0]
    for n in n_m:
        off.append(off[-1] + n)
    V = cfg.vocab_size
    table = torch.zeros(len(grids), T, dtype=torch.int64)
    vrt_steps = [t for t in range(T) if sched[t] == "v"]
    for b in range(len(grids)):
        for t in range(T):
            text = 20 + 3 * t + b
            assert text < min(cfg.image_token_id, V) and text not in (cfg.eos_token_id, cfg.pad_token_id)
            table[b, t] = V + off[b] + (5 * t + b) % n_m[b] if sched[t] == "v" else text
        table[b, T - 1] = cfg.eos_token_id
    other = (foreign_row + 1) % len(grids)
    foreign_at = vrt_steps[-1]
    table[foreign_row, foreign_at] = V + off[other] + 3
    table[eos_row, eos_at] = cfg.eos_token_id
    return table, vrt_steps, foreign_at, off


def test_off_policy_table_against_the_calls_own_scores(setup):
    cfg, U, model, kw = setup
    L = kw["input_ids"].shape[1]
    grids = kw["image_grid_thw"].tolist()
    table, vrt_steps, foreign_at, off = off_policy_table(cfg, grids)
    gen = dict(max_new_tokens=T_NEW, schedule=SCHED, output_token_logprobs=True, output_patch_logprobs=True, forced_tokens=table)
    own = model.generate(max_new_tokens=T_NEW, schedule=SCHED, **kw).sequences[:, L:].cpu()
    assert not torch.equal(own, table), "precondition: the table is the model's own choice"
    flagged = model.generate(**gen, **kw)
    scored = model.generate(output_scores=True, **gen, **kw)
    assert flagged.scores is None and torch.equal(flagged.sequences, scored.sequences)
    tok, lp = flagged.sequences[:, L:].cpu(), flagged.token_logprobs.cpu()
    assert tuple(tok.shape) == (2, T_NEW)
    assert torch.equal(tok[0], table[0]) and torch.equal(tok[1, :10], table[1, :10]) and bool((tok[1, 10:] == cfg.pad_token_id).all())
    ref = torch.stack([ref_logprob(scored.scores[t], tok[:, t]) for t in range(T_NEW)], 1)
    live = torch.ones(2, T_NEW, dtype=torch.bool)
    live[1, 10:] = False
    d = within(lp[live], ref[live])
    d2 = within(scored.token_logprobs.cpu()[live], ref[live])
    assert lp[0, foreign_at] == -INF and bool((lp[1, 10:] == 0.0).all()) and not bool(torch.isnan(lp).any())
    assert int(torch.isinf(lp).sum()) == 1, "only the foreign VRT is outside the processed row"
    assert bool((lp[live] < 0).sum() > T_NEW), "precondition: off-policy tokens are not certain"
    for t in vrt_steps:                                            # the pointing distribution at a forced VRT step: a sub-distribution
        p = flagged.patch_logprobs[:, t].double().exp().sum(-1)
        assert bool((p <= 1 + 1e-5).all()) and bool((p > 0).all())
    feats, dec = decode_objects(model, cfg, U, flagged, kw["image_grid_thw"], L)
    hid = flagged.hidden_states.last_layer_rows()
    assert [len(f) for f in feats] == [1, 1] and dec["sample_idx"] == [0, 1] and dec["pred_boxes"].shape[0] == 2
    for b in range(2):
        assert torch.equal(feats[b][0], hid[vrt_steps[0]: vrt_steps[-1] + 1, b])
    print(f"\n[off-policy] largest |token_logprobs - log_softmax(scores)| fused {d:.3e}  with output_scores {d2:.3e}")


def test_hooked_loop_processors_shape_the_scores_and_the_forced_token_wins(setup):
    cfg, U, model, kw = setup
    L = kw["input_ids"].shape[1]
    table, *_ = off_policy_table(cfg, kw["image_grid_thw"].tolist())
    out = model.generate(max_new_tokens=T_NEW, schedule=SCHED, output_token_logprobs=True, output_scores=True, forced_tokens=table,
                         logits_processor=[TL._bias_even_columns], stopping_criteria=[TL._never_stop], **kw)
    tok = out.sequences[:, L:].cpu()
    assert torch.equal(tok[0], table[0]) and torch.equal(tok[1, :10], table[1, :10])
    plain = model.generate(max_new_tokens=T_NEW, schedule=SCHED, output_scores=True, forced_tokens=table, **kw)
    assert not torch.equal(out.scores[0], plain.scores[0]), "the processor did not shape the scores"
    ref = torch.stack([ref_logprob(out.scores[t], tok[:, t]) for t in range(T_NEW)], 1)
    live = torch.ones(2, T_NEW, dtype=torch.bool)
    live[1, 10:] = False
    within(out.token_logprobs.cpu()[live], ref[live])


@pytest.mark.parametrize("operands", ["fp16", "bf16"])
def test_off_policy_table_against_the_oracle(operands):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import padt_amd
    import parity_util as U
    import test_e2e_gpu as E2E
    from padt_amd.modeling import PaDTForConditionalGeneration
    cfg = padt_amd.small_test_config()
    w = U.bf16_weights(cfg, seed=5, std=0.05)
    model = PaDTForConditionalGeneration(cfg, w, device="cuda", operands=operands)
    oc = U.oracle_config(cfg)
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 10, 12], [1, 8, 8]], n_pre=6, n_post=9, ragged=True, seed=91)
    table, vrt_steps, foreign_at, off = off_policy_table(cfg, grid.tolist())
    out = model.generate(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, max_new_tokens=T_NEW,
                         schedule=SCHED, output_token_logprobs=True, forced_tokens=table)
    ores = U.O.generate(w, oc, ids, am, pix, grid, T_NEW, schedule=SCHED, collect_logits=True, force_tokens=table)
    assert torch.equal(ores["sequences"], out.sequences.cpu())
    hid = out.hidden_states.last_layer_rows().cpu().float()
    lp = out.token_logprobs.cpu().double()
    worst, worst_rel = 0.0, 0.0
    for t in range(T_NEW):
        mx, rms = E2E.rel_err(hid[t], ores["hidden"][t][:, -1].float())
        assert rms < E2E.tol(model, 2e-2, 3e-3) and mx < E2E.tol(model, 8e-2, 1.2e-2), f"hidden step {t}: rel err max {mx:.3e} rms {rms:.3e}"
        lg = ores["logits"][t].double()
        floor = E2E.tol(model, 2e-2, 4e-3) * lg[torch.isfinite(lg)].abs().max().item()
        ref = torch.log_softmax(lg, -1).gather(1, out.sequences[:, ids.shape[1] + t].cpu()[:, None])[:, 0]
        for b in range(2):
            if b == 1 and t >= 10:                                 # after the row's EOS
                assert lp[b, t] == 0.0
            elif ref[b] == -INF:
                assert lp[b, t] == -INF and (b, t) == (0, foreign_at)
            else:
                diff = abs(float(lp[b, t] - ref[b]))
                worst, worst_rel = max(worst, diff), max(worst_rel, diff / (2 * floor) if floor > 0 else 0.0)     # forced-EOS step: one finite logit, 0
                assert diff <= 2 * floor, f"step {t} row {b}: |log-prob - oracle| {diff:.3e} > 2 x floor {floor:.3e}"
    print(f"\n[off-policy vs oracle, {operands}] largest |log-prob - oracle| {worst:.3e} ({worst_rel:.2f} of the bound)")


def test_merged_decode_group_each_batch_its_own_table(setup):
    cfg, U, model, _ = setup
    import padt_amd
    from padt_amd import pipeline
    T = 10
    sched = ["t"] * 3 + ["v"] * 4 + ["t"] * 2 + ["e"]
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 64), 2)
    proc.model_embed_token_size = cfg.vocab_size
    batches, tables = [], []
    for s, g in enumerate([[[1, 8, 8], [1, 10, 12]], [[1, 6, 10], [1, 8, 8]]]):
        grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5 + 3 * s, n_post=7, seed=100 + s, ragged=True)
        batches.append((ids.cuda(), am.cuda(), pix.cuda(), grid))
        tables.append(off_policy_table(cfg, g, T=T, sched=sched, eos_row=s, eos_at=7 + s, foreign_row=1 - s)[0])
    gen = dict(max_new_tokens=T, schedule=sched, output_token_logprobs=True)
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], forced_tokens=t, **gen) for b, t in zip(batches, tables)]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b, t in zip(batches, tables):
        got += runner.submit(b[0].clone(), *b[1:], forced_tokens=t, **gen)
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2
    for (d0, c0, l0, v0), (d1, c1, l1, v1), t in zip(alone, got, tables):
        assert c0 == c1 and v0 == v1, "tokens of the merged group differ from the batch alone"
        assert torch.equal(bits(d0["token_logprobs"]), bits(d1["token_logprobs"])) and int(torch.isinf(d1["token_logprobs"]).sum()) == 1
        assert bool((d0["token_logprobs"] < 0).any())
    # a batch that forces and one that does not never share a group
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = runner.submit(batches[0][0].clone(), *batches[0][1:], forced_tokens=tables[0], **gen)
    got += runner.submit(batches[1][0].clone(), *batches[1][1:], **gen)
    got += runner.flush()
    assert runner.n_groups == 2 and len(got) == 2
    assert torch.equal(bits(got[0][0]["token_logprobs"]), bits(alone[0][0]["token_logprobs"]))
    assert got[1][1] != alone[1][1], "precondition: the unforced batch makes its own choice"


def test_range_guard_rerun_passes_the_table_on():
    """operands="auto": the forced batch whose SwiGLU hidden exceeds fp16's range (test_range_guard_gpu's `llm_swiglu` weights) is answered by the
    bf16 twin with the caller's table — what the bf16 model gives directly"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_range_guard_gpu as RG
    from padt_amd.modeling import PaDTForConditionalGeneration
    cfg, w, U = RG._weights("llm_swiglu")
    g = [[1, 8, 8], [1, 10, 12]]
    grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5, n_post=8, ragged=True, seed=41)
    kw = dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    table = off_policy_table(cfg, g)[0]
    gen = dict(max_new_tokens=T_NEW, schedule=SCHED, output_token_logprobs=True, forced_tokens=table)
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16").generate(**gen, **kw)
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(**gen, **kw)
    assert auto.overflow_reruns == 1
    assert torch.equal(got.sequences, ref.sequences) and torch.equal(bits(got.token_logprobs), bits(ref.token_logprobs))
    assert torch.equal(got.sequences[0, ids.shape[1]:].cpu(), table[0])


def test_score_completions_ranks_candidates_of_one_image(setup):
    cfg, U, model, _ = setup
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8]], n_pre=6, n_post=9, seed=93)
    kw = dict(input_ids=ids.repeat(2, 1).cuda(), attention_mask=am.repeat(2, 1).cuda(), pixel_values=pix.cuda(), image_grid_thw=grid,
              image_index=[0, 0])
    eos, V = cfg.eos_token_id, cfg.vocab_size
    cands = [[21, 22, V + 3, V + 4, 23, eos], [31, eos, 33]]        # ragged; the second ends early: its third entry must not count
    out = model.score_completions(completions=cands, **kw)
    plain = model.generate(forced_tokens=cands, max_new_tokens=6, output_token_logprobs=True, **kw)
    assert torch.equal(out.sequences, plain.sequences) and torch.equal(bits(out.token_logprobs), bits(plain.token_logprobs))
    lp = plain.token_logprobs
    masked = lp.clone()
    masked[1, 2:] = 0.0
    want = masked.sum(1)
    assert tuple(lp.shape) == (2, 6) and bool((lp[1, 2:] == 0.0).all())      # after the second row's EOS: already 0.0
    assert torch.equal(bits(out.completion_logprobs), bits(want)) and bool(torch.isfinite(want).all()) and bool((want < 0).all())
    per = out.completion_token_logprobs
    assert torch.equal(bits(per[0]), bits(lp[0])) and torch.equal(bits(per[1, :2]), bits(lp[1, :2])) and bool((per[1, 2:] == 0.0).all())
    with pytest.raises(ValueError, match="forced_tokens"):
        model.score_completions(completions=[[21], [V + 32]], **kw)       # two samples x 16 patches: one past the table
    with pytest.raises(ValueError, match="max_new_tokens"):
        model.score_completions(completions=cands, max_new_tokens=3, **kw)
    # without the argument generate returns token_logprobs as before
    a = model.generate(max_new_tokens=6, output_token_logprobs=True, **kw)
    b = model.generate(max_new_tokens=6, output_token_logprobs=True, output_scores=True, **kw)
    assert "completion_logprobs" not in a and torch.equal(a.sequences, b.sequences)
    tok = a.sequences[:, ids.shape[1]:].cpu()
    within(a.token_logprobs, torch.stack([ref_logprob(b.scores[t], tok[:, t]) for t in range(tok.shape[1])], 1))
    with pytest.raises(ValueError, match="forced_token"):
        model.generate(max_new_tokens=4, forced_token=cands, **kw)
