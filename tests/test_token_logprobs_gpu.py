"""generate(output_token_logprobs=True): the log-prob of every token generate picks, without a logit row in memory.

Kernel level: padt_vrt_head_lse + padt_greedy_step_lp (the fused path) and padt_token_logprob_rows_f32 (the row path) against
torch.log_softmax in fp64 of the fp32 row the SAME launch wrote, in every dispatch variant of the head, with NaN-filled outputs and guard words
around part_sum / logprobs.  End to end (the small synthetic model, two ragged samples): the flagged call against the same call with
output_scores=True in every mode the flag is wired into.

The bound |got - ref| <= 5e-6 + 2^-22 |ref| is derived, not tuned: the logits are the same bits, so only the log-sum-exp differs — v_exp_f32
on x * log2e (relative error ~2^-23 + 6e-8 |x| per term, weighted by softmax mass: < 1e-6), blocked + tree fp32 summation ((log2 N + 16) 2^-24),
the final subtraction (2^-24 |ref|).  Every kernel-level test prints the largest difference it saw (profiles/token_logprobs.md quotes them).
"""
import types

import pytest
import torch

import test_token_selection_gpu as TS

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
X16 = pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
INF = float("inf")
GUARD, GUARD_VAL = 8, 12345.0
PAD = 7


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


i32, bits = TS.i32, TS.bits


def within(got, ref):
    """|got - ref| <= 5e-6 + 2^-22 |ref| element-wise (fp64); -inf only where the reference is -inf.  → the largest difference"""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape
    ninf = ref == -INF
    assert torch.equal(got == -INF, ninf), "-inf entries differ from the reference"
    assert bool(torch.isfinite(got[~ninf]).all()), "a log-prob is NaN / +inf"
    d = (got[~ninf] - ref[~ninf]).abs()
    bad = d > 5e-6 + 2.0 ** -22 * ref[~ninf].abs()
    assert not bad.any(), f"{int(bad.sum())} log-probs outside 5e-6 + 2^-22 |ref|, largest difference {d.max().item():.3e}"
    return d.max().item() if d.numel() else 0.0


def ref_logprob(rows, tok):
    """log_softmax(row.double())[token] on the CPU; a row without any candidate → -inf"""
    rows = rows.cpu().double()
    ls = torch.log_softmax(rows, -1)
    out = ls.gather(1, tok.cpu().long().clamp(0, rows.shape[1] - 1)[:, None])[:, 0]
    out[(rows == -INF).all(-1)] = -INF
    return out


def guarded(n, fill=float("nan")):
    """a NaN-filled fp32 buffer of n elements between two runs of guard words → (flat, view)"""
    flat = torch.full((2 * GUARD + n,), GUARD_VAL, device="cuda")
    view = flat[GUARD: GUARD + n]
    view.fill_(fill)
    return flat, view


def guards_ok(flat):
    return bool((flat[:GUARD] == GUARD_VAL).all()) and bool((flat[-GUARD:] == GUARD_VAL).all())


def fused(ops, h, E, P, off, packed, lse=True, t_max=3, step=1, eos=-3, mode_table=None, gen_cfg=None, seen=None, ban=None, unf=None):
    """One step of the fused path — head (with its logits row) then the greedy step — on NaN / garbage filled outputs."""
    B, D = h.shape
    V, NP = E.shape[0], P.shape[0]
    nblk = ops.vrt_head_nblk(V, NP)
    r = types.SimpleNamespace(nblk=nblk, t_max=t_max, step=step)
    r.pv = torch.full((nblk * B,), float("nan"), device="cuda")
    r.pi = torch.full((nblk * B,), -5, dtype=torch.int32, device="cuda")
    r.lg = torch.full((B, V + NP), float("nan"), device="cuda")
    r.ps_flat, r.ps = guarded(nblk * B)
    r.lp_flat, lp = guarded(B * t_max)
    r.lp = lp.view(B, t_max)
    st = i32([step])
    kw = dict(mode_table=mode_table, step=st if mode_table is not None else None, logits=r.lg, gen_cfg=gen_cfg, seen=seen, ban=ban)
    if lse:
        kw["part_sum"] = r.ps
    if packed:
        hp = torch.zeros((B + 15) // 16 * 16, D, device="cuda", dtype=h.dtype)
        ops.pack_rows(h, hp, B, to_packed=True)
        ops.vrt_head(hp, E, P, i32(off), r.pv, r.pi, eos, table_packed=ops.pack_weight(E), rows=B, **kw)
    else:
        ops.vrt_head(h, E, P, i32(off), r.pv, r.pi, eos, **kw)
    hid = torch.zeros(B, 8, device="cuda", dtype=BF)
    r.unf = torch.ones(B, dtype=torch.int32, device="cuda") if unf is None else i32(unf)
    r.tok = torch.full((B, t_max), -9, dtype=torch.int64, device="cuda")
    r.cur = torch.full((B,), -9, dtype=torch.int64, device="cuda")
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    gk = dict(part_sum=r.ps, logprobs=r.lp) if lse else {}
    ops.greedy_step(r.pv, r.pi, nblk, hid, torch.zeros(t_max, B, 8, device="cuda", dtype=BF), r.unf, r.tok, r.cur, st, z(B), z(B), z(3, B),
                    eos, PAD, gen_cfg=gen_cfg, **gk)
    torch.cuda.synchronize()
    assert int(st) == step + 1
    assert guards_ok(r.ps_flat) and guards_ok(r.lp_flat), "guard words around part_sum / logprobs overwritten"
    return r


def only_column_written(r):
    """logprobs: exactly column `step` is written, every other entry is still the NaN fill"""
    other = torch.ones(r.t_max, dtype=torch.bool)
    if r.step < r.t_max:
        other[r.step] = False
    return bool(torch.isnan(r.lp[:, other.cuda()]).all())


def same_selection(a, b):
    return (torch.equal(bits(a.pv), bits(b.pv)) and torch.equal(a.pi, b.pi) and torch.equal(bits(a.lg), bits(b.lg)) and torch.equal(a.cur, b.cur)
            and torch.equal(a.tok, b.tok) and torch.equal(a.unf, b.unf))


# ------------------------------------------------------------------------------------------------------------ fused path
FUSED_LAYOUTS = ["rowmajor", "packed", "rowmajor_vtail", "rowmajor_d200"]
FUSED_B = [1, 5, 17, 33, 65]


def fused_shape(layout, B):
    counts = TS.ragged_counts(B)                                   # sample 0 has no prototypes (B > 1)
    r = 1 if FUSED_B.index(B) % 2 == 0 else 3                      # block count 1 / 3 mod 4
    D = 200 if layout == "rowmajor_d200" else 64
    return counts, TS.vocab_for(counts, r, tail=5 if layout == "rowmajor_vtail" else 0), D


@X16
@pytest.mark.parametrize("layout", FUSED_LAYOUTS)
@pytest.mark.parametrize("B", FUSED_B)
def test_fused_logprob_every_dispatch_variant(ops, dt, layout, B):
    counts, V, D = fused_shape(layout, B)
    E, P, h, off = TS.head_problem(B, V, counts, D, dt, seed=2000 + B)
    packed = layout == "packed"
    a = fused(ops, h, E, P, off, packed)
    plain = fused(ops, h, E, P, off, packed, lse=False)
    assert same_selection(a, plain), "tokens / partials / written logits with LSE differ from the non-LSE kernel"
    again = fused(ops, h, E, P, off, packed)
    assert torch.equal(bits(a.ps), bits(again.ps)) and torch.equal(bits(a.lp), bits(again.lp)), "two launches differ"
    assert bool(torch.isfinite(a.ps).all()) and bool((a.ps >= 0).all())
    assert torch.equal(a.cur.cpu(), a.lg.cpu().argmax(-1)) and only_column_written(a)
    d = within(a.lp[:, a.step], ref_logprob(a.lg, a.cur))
    print(f"\n[fused {layout} B={B} {dt}] largest |log-prob - fp64 reference| {d:.3e}")
    if packed:
        rm = fused(ops, h, E, P, off, False)
        assert torch.equal(bits(a.ps), bits(rm.ps)) and torch.equal(bits(a.lp), bits(rm.lp)), "packed part_sum differs from row-major"


@X16
def test_fused_logprob_more_blocks_than_threads(ops, dt):
    """nblk > 256: the greedy step's strided loop takes more than one block per thread (V % 16 == 5)"""
    B, D = 5, 64
    counts = TS.ragged_counts(B)
    E, P, h, off = TS.head_problem(B, 16 * 300 + 5, counts, D, dt, seed=31)
    a = fused(ops, h, E, P, off, False)
    assert a.nblk > 256 and same_selection(a, fused(ops, h, E, P, off, False, lse=False))
    d = within(a.lp[:, a.step], ref_logprob(a.lg, a.cur))
    print(f"\n[fused nblk={a.nblk} {dt}] largest |log-prob - fp64 reference| {d:.3e}")


@X16
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
def test_fused_logprob_scripted_modes(ops, dt, packed):
    """mode 3: one allowed column → exactly 0.0; mode 2: a sample without prototypes has no candidate → -inf, pad, no NaN in part_sum;
    modes 1 / 2 leave whole blocks masked → their part_sum is an exact 0"""
    B, D, eos = 5, 64, 37
    counts = TS.ragged_counts(B)
    V = TS.vocab_for(counts, 3)
    E, P, h, off = TS.head_problem(B, V, counts, D, dt, seed=41)
    for mode in (1, 2, 3):
        a = fused(ops, h, E, P, off, packed, eos=eos, mode_table=i32([0, mode, 0]))
        assert same_selection(a, fused(ops, h, E, P, off, packed, lse=False, eos=eos, mode_table=i32([0, mode, 0])))
        ps = a.ps.view(a.nblk, B).cpu()
        assert bool(torch.isfinite(ps).all()) and bool((ps >= 0).all()), f"mode {mode}: part_sum holds NaN / inf / negative entries"
        lp, tok = a.lp[:, a.step].cpu(), a.cur.cpu()
        if mode == 3:
            assert bool((lp == 0.0).all()) and bool((tok == eos).all())
            assert bool((ps.sum(0) == 1.0).all()) and bool(((ps == 0) | (ps == 1)).all())
        elif mode == 2:
            assert counts[0] == 0 and lp[0] == -INF and int(tok[0]) == PAD
            assert bool((ps[: V // 16] == 0).all()), "a text block under mode 2 must add an exact 0"
            within(lp, ref_logprob(a.lg, tok))
        else:
            assert bool((ps[V // 16:] == 0).all()), "a prototype block under mode 1 must add an exact 0"
            within(lp, ref_logprob(a.lg, tok))


@X16
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
def test_fused_logprob_with_ban_bitmap_and_repetition_penalty(ops, dt, packed):
    B, D = 17, 64
    counts = TS.ragged_counts(B)
    V = TS.vocab_for(counts, 1)
    E, P, h, off = TS.head_problem(B, V, counts, D, dt, seed=43)
    words = (V + sum(counts) + 31) // 32
    g = torch.Generator().manual_seed(5)
    rnd_bits = lambda p: (torch.rand(B, words * 32, generator=g) < p).view(B, words, 32).long().mul(1 << torch.arange(32)).sum(-1)
    to_i32 = lambda t: torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32).cuda()
    ban = rnd_bits(0.3)
    ban[3] = 2 ** 32 - 1                                            # row 3: every column banned
    ban, seen = to_i32(ban), to_i32(rnd_bits(0.5))
    cfg = ops.gen_cfg_tensor(1.3, (), "cuda")
    a = fused(ops, h, E, P, off, packed, gen_cfg=cfg, seen=seen.clone(), ban=ban)
    assert same_selection(a, fused(ops, h, E, P, off, packed, lse=False, gen_cfg=cfg, seen=seen.clone(), ban=ban))
    unpen = fused(ops, h, E, P, off, packed, ban=ban)
    assert not torch.equal(bits(a.lg), bits(unpen.lg)), "the penalty changed nothing"
    lg, lp, tok = a.lg.cpu(), a.lp[:, a.step].cpu(), a.cur.cpu()
    assert float((lg == -INF).float().mean()) > 0.25
    assert lp[3] == -INF and int(tok[3]) == PAD and bool((lg[3] == -INF).all())
    assert bool(torch.isfinite(a.ps).all())
    d = within(lp, ref_logprob(lg, tok))
    print(f"\n[fused ban + penalty {dt} packed={packed}] largest |log-prob - fp64 reference| {d:.3e}")


@X16
def test_fused_logprob_logits_of_magnitude_80(ops, dt):
    """hidden rows scaled until the logits reach +-80: exp(80) overflows nothing only because the maximum is subtracted first"""
    B, D = 5, 64
    counts = TS.ragged_counts(B)
    E, P, h, off = TS.head_problem(B, TS.vocab_for(counts, 1), counts, D, dt, seed=47)
    h = (h.float() * 4).to(dt)
    a = fused(ops, h, E, P, off, False)
    lg = a.lg.cpu()
    fin = lg[torch.isfinite(lg)]
    assert fin.max() > 80 and fin.min() < -80, "precondition: the logits do not reach +-80"
    d = within(a.lp[:, a.step], ref_logprob(lg, a.cur))
    print(f"\n[fused +-80 {dt}] largest |log-prob - fp64 reference| {d:.3e}")


def test_fused_logprob_finished_rows_and_steps_past_t_max(ops):
    B, D = 5, 64
    counts = TS.ragged_counts(B)
    E, P, h, off = TS.head_problem(B, TS.vocab_for(counts, 1), counts, D, BF, seed=53)
    unf = [1, 0, 1, 0, 1]
    a = fused(ops, h, E, P, off, False, unf=unf)
    lp, tok = a.lp[:, a.step].cpu(), a.cur.cpu()
    live = torch.tensor(unf, dtype=torch.bool)
    assert bool((lp[~live] == 0.0).all()) and bool((tok[~live] == PAD).all())
    within(lp[live], ref_logprob(a.lg[live.cuda()], tok[live]))
    for step in (3, 8):                                              # step >= T_max: nothing is written (fused() checks the guard words)
        b = fused(ops, h, E, P, off, False, step=step)
        assert bool(torch.isnan(b.lp).all()) and bool((b.tok == -9).all())


# ------------------------------------------------------------------------------------------------------------ row path
def row_lp(ops, x, n, pi, unf, step, t_max=4):
    B = x.shape[0]
    flat, lp = guarded(B * t_max)
    lp = lp.view(B, t_max)
    st = i32([step])
    ops.token_logprob_rows(x, n, pi, unf, st, lp, B)
    torch.cuda.synchronize()
    assert guards_ok(flat) and int(st) == step
    return lp


@pytest.mark.parametrize("n", [113, 1029])
def test_row_logprob_against_fp64_log_softmax(ops, n):
    g = torch.Generator().manual_seed(n)
    B, ld = 6, n + 3
    x = torch.full((B, ld), float("nan"))                            # past n_cols: NaN — a read past the row would poison the sum
    x[:, :n] = torch.randn(B, n, generator=g) * 6
    x[:, :n][torch.rand(B, n, generator=g) < 0.3] = -INF
    x[5, :n] = -INF
    x[5, 40] = 2.5                                                   # one candidate: exactly 0.0
    x[0, 0], x[1, n - 1], x[2, 17], x[4, 9] = 1.0, -2.0, 0.5, -INF
    pi = i32([0, n - 1, 17, 3, 9, 40])                               # the chosen column at index 0 and n_cols - 1; row 4 chose a masked column
    unf = i32([1, 1, 1, 0, 1, 1])                                    # row 3 finished earlier
    xd = x.cuda()
    lp = row_lp(ops, xd, n, pi, unf, step=2)
    assert torch.equal(bits(xd), bits(x.cuda())), "the row kernel wrote to its input"
    assert bool(torch.isnan(lp[:, [0, 1, 3]]).all())
    got = lp[:, 2].cpu()
    assert got[3] == 0.0 and got[4] == -INF and got[5] == 0.0
    live = torch.tensor([0, 1, 2, 5])
    d = within(got[live], ref_logprob(x[live, :n], pi.cpu()[live]))
    print(f"\n[rows n={n}] largest |log-prob - fp64 reference| {d:.3e}")
    assert torch.equal(bits(row_lp(ops, xd, n, pi, unf, step=2)), bits(lp)), "two launches differ"
    assert bool(torch.isnan(row_lp(ops, xd, n, pi, unf, step=4)).all()) and bool(torch.isnan(row_lp(ops, xd, n, pi, unf, step=-1)).all())


@pytest.mark.parametrize("n", [113, 1029])
def test_row_logprob_of_a_row_warped_by_sample_token(ops, n):
    g = torch.Generator().manual_seed(7 + n)
    B, ld = 5, n + 3
    x = torch.full((B, ld), float("nan"))
    x[:, :n] = torch.randn(B, n, generator=g) * 3
    xd = x.cuda()
    cfg = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=3, temperature=0.7, top_k=20, top_p=0.9, write_back=True)
    pv, pi, st = torch.zeros(B, device="cuda"), torch.full((B,), -5, dtype=torch.int32, device="cuda"), i32([1])
    ops.sample_token(xd, n, cfg, st, pv, pi, B)
    lp = row_lp(ops, xd, n, pi, torch.ones(B, dtype=torch.int32, device="cuda"), step=1)
    warped = xd.cpu()[:, :n]
    kept = torch.isfinite(warped).sum(-1)
    assert bool((kept >= 1).all()) and bool((kept <= 20).all()), "precondition: the rows are the warped ones"
    d = within(lp[:, 1], ref_logprob(warped, pi))
    assert bool(torch.isfinite(lp[:, 1]).all())
    print(f"\n[rows warped n={n}] largest |log-prob - fp64 reference| {d:.3e}")


def test_entry_points_validate_their_arguments(ops):
    from padt_amd._lib import PaDTHipError, load
    lib = load()
    assert lib.padt_token_logprob_rows_f32(0, 0, 8, 8, 0, 0, 0, 0, 4, 2) == -1 and b"padt_token_logprob_rows_f32" in lib.padt_last_error()
    assert lib.padt_token_logprob_rows_f32(0, 0, 8, 8, 0, 0, 0, 0, 4, 0) == 0                                     # no rows: nothing to do
    x = torch.zeros(2, 8, device="cuda")
    with pytest.raises(PaDTHipError, match="padt_token_logprob_rows_f32"):
        ops.token_logprob_rows(x, 0, i32([0, 0]), i32([1, 1]), i32([0]), torch.zeros(2, 4, device="cuda"), 2)


# ------------------------------------------------------------------------------------------------------------ end to end
T_NEW = 12
SCHED = ["t"] * 5 + ["v"] * 3 + ["t"] * 3 + ["e"]
TEXT = ["t"] * T_NEW                                               # text rows only, nothing forced: the rows end where their own EOS ids say


def small_model(**kw):
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    return cfg, U, PaDTForConditionalGeneration(cfg, U.bf16_weights(cfg, seed=5, std=0.05), device="cuda", **kw)


def two_ragged(cfg, U, seed=91):
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 10, 12], [1, 8, 8]], n_pre=6, n_post=9, ragged=True, seed=seed)
    return dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = small_model()
    return cfg, U, model, two_ragged(cfg, U)


def early_eos(model, cfg, kw, gen):
    """An EOS list under which one row finishes before the other: config.eos_token_id plus a text token that one row of the SAME run emits
    (for the first time) at a step up to which no other row has emitted it."""
    L = kw["input_ids"].shape[1]
    tok = model.generate(**gen, **kw).sequences[:, L:].cpu()
    B, T = tok.shape
    for t in range(T - 2):
        for b in range(B):
            x = int(tok[b, t])
            others = torch.cat([tok[:b, : t + 2], tok[b + 1:, : t + 2]]).flatten().tolist()
            if x < min(cfg.vocab_size, cfg.image_token_id) and x not in tok[b, :t].tolist() and x not in others and cfg.eos_token_id not in others:
                return [cfg.eos_token_id, x]
    raise AssertionError(f"precondition: no token of the run can serve as an early EOS: {tok.tolist()}")


def check_against_scores(flagged, scored, L, eos):
    """sequences equal; token_logprobs[b, t] = log_softmax(scores[t][b])[token] up to and including the row's EOS step, 0.0 after it"""
    assert torch.equal(flagged.sequences, scored.sequences)
    tok = flagged.sequences[:, L:].cpu()
    lp = flagged.token_logprobs
    assert lp.dtype == torch.float32 and lp.device == flagged.sequences.device and tuple(lp.shape) == tuple(tok.shape) == (tok.shape[0], len(scored.scores))
    lp = lp.cpu()
    is_eos = torch.isin(tok, torch.tensor(eos))
    done_before = (is_eos.long().cumsum(1) - is_eos.long()) > 0                      # the row finished at an earlier step
    assert done_before.any() and not done_before.any(1).all(), "precondition: one row finishes before the other"
    assert bool((lp[done_before] == 0.0).all()), "steps after a row's EOS must hold 0.0"
    ref = torch.stack([ref_logprob(scored.scores[t], tok[:, t]) for t in range(tok.shape[1])], 1)
    assert bool(torch.isfinite(ref[~done_before]).all())
    return within(lp[~done_before], ref[~done_before])


def flagged_vs_scored(model, cfg, kw, gen):
    eos = early_eos(model, cfg, kw, gen)
    flagged = model.generate(output_token_logprobs=True, eos_token_id=eos, **gen, **kw)
    assert flagged.scores is None
    scored = model.generate(output_scores=True, eos_token_id=eos, **gen, **kw)
    assert scored.token_logprobs is None
    return check_against_scores(flagged, scored, kw["input_ids"].shape[1], eos), flagged


def _bias_even_columns(input_ids, scores):
    out = scores.clone()
    out[:, ::2] += 1.5
    return out


def _never_stop(input_ids, scores):
    return torch.zeros(input_ids.shape[0], dtype=torch.bool, device=input_ids.device)


MODES = {
    "captured_greedy": dict(max_new_tokens=T_NEW, schedule=TEXT),
    "eager_steps": dict(max_new_tokens=T_NEW, schedule=TEXT, use_graph=False),
    "penalty_and_ngram": dict(max_new_tokens=T_NEW, schedule=TEXT, repetition_penalty=1.3, no_repeat_ngram_size=2),
    "schedule": dict(max_new_tokens=T_NEW, schedule=SCHED),
    "sampling": dict(max_new_tokens=T_NEW, schedule=TEXT, do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=11),
    "caller_processor": dict(max_new_tokens=T_NEW, schedule=TEXT, logits_processor=[_bias_even_columns]),
    "caller_criteria_only": dict(max_new_tokens=T_NEW, schedule=TEXT, stopping_criteria=[_never_stop]),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_generate_token_logprobs_equal_log_softmax_of_the_scores(setup, mode):
    cfg, U, model, kw = setup
    d, flagged = flagged_vs_scored(model, cfg, kw, MODES[mode])
    print(f"\n[generate {mode}] largest |token_logprobs - log_softmax(scores)| {d:.3e}")
    if mode == "sampling":                                          # the warpers bite: some drawn token is not the row's only candidate
        assert bool((flagged.token_logprobs < 0).any())
    if mode == "schedule" and flagged.token_logprobs.shape[1] == T_NEW:        # the forced EOS step of the row still live there: one candidate
        assert float(flagged.token_logprobs[:, -1].abs().max()) == 0.0


def test_generate_without_the_flag_returns_none_and_unknown_spelling_still_raises(setup):
    cfg, U, model, kw = setup
    out = model.generate(max_new_tokens=4, **kw)
    assert "token_logprobs" in out and out.token_logprobs is None
    with pytest.raises(ValueError, match="output_token_logprob"):
        model.generate(max_new_tokens=4, output_token_logprob=True, **kw)


def test_generate_token_logprobs_with_image_index(setup):
    """two queries on one image: the prompt pass is the shared one, the decode steps are what they are without an index"""
    cfg, U, model, _ = setup
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8]], n_pre=6, n_post=9, seed=93)
    ids = ids.repeat(2, 1)
    ids[1, -4:] = torch.tensor([5, 6, 7, 8])                        # the queries part after the image
    kw = dict(input_ids=ids.cuda(), attention_mask=am.repeat(2, 1).cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, image_index=[0, 0])
    d, _ = flagged_vs_scored(model, cfg, kw, dict(max_new_tokens=T_NEW, schedule=SCHED))
    print(f"\n[generate image_index] largest difference {d:.3e}")


def test_generate_token_logprobs_reference_precision():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = small_model(precision="reference")
    d, _ = flagged_vs_scored(model, cfg, two_ragged(cfg, U), dict(max_new_tokens=T_NEW, schedule=SCHED))
    print(f"\n[generate precision=reference] largest difference {d:.3e}")


def test_merged_decode_group_token_logprobs_equal_each_batch_alone(setup):
    cfg, U, model, _ = setup
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
    gen = dict(max_new_tokens=T, schedule=sched, output_token_logprobs=True)
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], **gen) for b in batches]
    plain = pipeline.rec_batch(model, proc, batches[0][0].clone(), *batches[0][1:], max_new_tokens=T, schedule=sched)
    assert "token_logprobs" not in plain[0]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b in batches:
        got += runner.submit(b[0].clone(), *b[1:], **gen)
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2
    for (d0, c0, l0, v0), (d1, c1, l1, v1) in zip(alone, got):
        assert c0 == c1 and v0 == v1, "tokens of the merged group differ from the batch alone"
        assert tuple(d1["token_logprobs"].shape) == (2, T) and bool((d0["token_logprobs"] < 0).any())
        d = within(d1["token_logprobs"], d0["token_logprobs"])
        print(f"\n[merged group] largest |merged - alone| {d:.3e}")
    # batches that disagree on the flag never share a group
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = runner.submit(batches[0][0].clone(), *batches[0][1:], **gen)
    got += runner.submit(batches[1][0].clone(), *batches[1][1:], max_new_tokens=T, schedule=sched)
    got += runner.flush()
    assert runner.n_groups == 2 and len(got) == 2
    within(got[0][0]["token_logprobs"], alone[0][0]["token_logprobs"])
    assert "token_logprobs" not in got[1][0]


def test_generate_launch_collect_all_batches_carry_one_field_per_batch(setup):
    cfg, U, model, kw = setup
    args = (kw["input_ids"], kw["attention_mask"], kw["pixel_values"], kw["image_grid_thw"])
    ctx = model.generate_launch(*args, max_new_tokens=6, n_slots=2, lane=3, output_token_logprobs=True)
    ctx = model.generate_launch(*args, max_new_tokens=6, n_slots=2, lane=3, output_token_logprobs=True, group=ctx)
    outs = model.generate_collect(ctx, all_batches=True)
    alone = model.generate(max_new_tokens=6, output_token_logprobs=True, **kw)
    assert len(outs) == 2
    for o in outs:
        assert torch.equal(o.sequences, alone.sequences) and tuple(o.token_logprobs.shape) == (2, o.sequences.shape[1] - args[0].shape[1])
        within(o.token_logprobs, alone.token_logprobs)
    o = alone.token_logprobs.clone()                               # the caller owns what it got: a later generate of the same session
    model.generate(max_new_tokens=6, output_token_logprobs=True, schedule=["e"] * 6, **kw)
    assert torch.equal(o, alone.token_logprobs) and bool((o < 0).any())


def test_range_guard_rerun_on_the_bf16_twin_carries_the_field():
    """operands="auto": the batch whose SwiGLU hidden exceeds fp16's range (test_range_guard_gpu.py's `llm_swiglu` weights) is answered by the
    bf16 twin — with token_logprobs, equal to log_softmax of the bf16 model's own scores"""
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
    gen = dict(max_new_tokens=T_NEW, schedule=SCHED)
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16")
    eos = early_eos(ref, cfg, kw, gen)
    scored = ref.generate(output_scores=True, eos_token_id=eos, **gen, **kw)
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(output_token_logprobs=True, eos_token_id=eos, **gen, **kw)
    assert auto.overflow_reruns == 1 and got.token_logprobs is not None
    d = check_against_scores(got, scored, ids.shape[1], eos)
    print(f"\n[range-guard re-run] largest difference {d:.3e}")


# ------------------------------------------------------------------------------------------------------------ what is launched
def _recorded(monkeypatch, ops, model, kw, **gen):
    """the ops wrappers a generate goes through, in order; vrt_head / greedy_step calls that carry part_sum are marked '+lse'"""
    calls = []
    with monkeypatch.context() as mp:
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_"):
                def stub(*a, _fn=fn, _name=name, **k):
                    calls.append(_name + ("+lse" if k.get("part_sum") is not None else ""))
                    return _fn(*a, **k)
                mp.setattr(ops, name, stub)
        out = model.generate(use_graph=False, **gen, **kw)
    return calls, out


@pytest.mark.parametrize("mode", ["captured_greedy", "sampling"])
def test_the_flag_changes_only_the_lse_variants_and_the_row_kernel(setup, ops, monkeypatch, mode):
    cfg, U, model, kw = setup
    gen = {k: v for k, v in MODES[mode].items() if k != "use_graph"}
    plain, a = _recorded(monkeypatch, ops, model, kw, **gen)
    flagged, b = _recorded(monkeypatch, ops, model, kw, output_token_logprobs=True, **gen)
    assert torch.equal(a.sequences, b.sequences)
    n_steps = b.token_logprobs.shape[1]
    assert not any(c.endswith("+lse") or c == "token_logprob_rows" for c in plain)
    assert [c.replace("+lse", "") for c in flagged if c != "token_logprob_rows"] == plain
    heads = [c for c in flagged if c.startswith(("vrt_head", "greedy_step")) and "nblk" not in c]
    if mode == "sampling":
        assert flagged.count("token_logprob_rows") >= n_steps and not any(c.endswith("+lse") for c in flagged)
    else:
        assert "token_logprob_rows" not in flagged and len(heads) >= 2 * n_steps and all(c.endswith("+lse") for c in heads)
