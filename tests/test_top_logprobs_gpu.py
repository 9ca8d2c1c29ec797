"""generate(top_logprobs=k, output_patch_logprobs=True): the k best candidates of every step and the sample's own patch distribution.

Kernel level: padt_topk_logprob_rows_f32 against a CPU reference in fp64 of the SAME fp32 rows — ids from a stable descending sort (equal values in
ascending column order: checked below), values from log_softmax — on strided rows with NaN past n_cols and NaN / garbage filled outputs between
guard words.  Ids must be EQUAL (same bits in, exact selection); log-probs within |got - ref| <= 5e-6 + 2^-22 |ref|, the bound derived in the
header of test_token_logprobs_gpu.py (only the log-sum-exp is inexact: the derivation carries over); -inf exactly where the reference has it.
End to end (the small synthetic model, the two ragged samples of test_token_logprobs_gpu.py): the flagged call against the same call with
output_scores=True in every mode the flags are wired into.  Every test prints the largest difference it saw (profiles/top_logprobs.md).
"""
import types

import pytest
import torch

import test_token_logprobs_gpu as TL

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD = TL.GUARD
IGUARD, IFILL = 424242, -7
i32, bits, within = TL.i32, TL.bits, TL.within
ops = TL.ops


def guarded_i(n):
    flat = torch.full((2 * GUARD + n,), IGUARD, dtype=torch.int32, device="cuda")
    flat[GUARD: GUARD + n] = IFILL
    return flat, flat[GUARD: GUARD + n]


def iguards_ok(flat):
    return bool((flat[:GUARD] == IGUARD).all()) and bool((flat[-GUARD:] == IGUARD).all())


def tied_rows(B, n, seed):
    """(B, n + 3) fp32: randn * 6 rounded to multiples of 0.5 with 30 % of the entries -inf, NaN past n_cols"""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B, n + 3), float("nan"))
    v = torch.round(torch.randn(B, n, generator=g) * 12) / 2
    v[torch.rand(B, n, generator=g) < 0.3] = -INF
    x[:, :n] = v
    return x


def ref_topk(rows, k):
    """rows (B, n) fp32 on the CPU → ids (B, k) int64, log-probs (B, k) fp64: stable descending sort + log_softmax in fp64, -1 / -inf past the
    finite columns"""
    d = rows.double()
    B, n = d.shape
    vals, idx = torch.sort(d, dim=1, descending=True, stable=True)
    ls = torch.log_softmax(d, -1)
    ids = torch.full((B, k), -1, dtype=torch.int64)
    lp = torch.full((B, k), -INF, dtype=torch.float64)
    m = min(n, k)
    ids[:, :m] = idx[:, :m]
    lp[:, :m] = ls.gather(1, idx[:, :m])
    dead = torch.ones(B, k, dtype=torch.bool)
    dead[:, :m] = vals[:, :m] == -INF
    ids[dead] = -1
    lp[dead] = -INF
    return ids, lp


def launch(ops, xd, n, k, unf, step, t_max=3, vrt_off=None, vocab=0, p_cap=0):
    """one launch into NaN / garbage filled outputs between guard words → namespace(idx, val, patch (views), flats)"""
    B = unf.numel()
    r = types.SimpleNamespace(idx=None, val=None, patch=None, flats=[], iflats=[])
    if k:
        f, v = guarded_i(B * t_max * k)
        r.iflats.append(f)
        r.idx = v.view(B, t_max, k)
        f, v = TL.guarded(B * t_max * k)
        r.flats.append(f)
        r.val = v.view(B, t_max, k)
    if p_cap:
        f, v = TL.guarded(B * t_max * p_cap)
        r.flats.append(f)
        r.patch = v.view(B, t_max, p_cap)
    ws = torch.full((ops.topk_rows_workspace(n, k, B) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    ops.topk_logprob_rows(xd, n, unf, i32([step]), ws, B, top_idx=r.idx, top_val=r.val, vrt_off=vrt_off, vocab=vocab, patch_lp=r.patch)
    torch.cuda.synchronize()
    assert all(TL.guards_ok(f) for f in r.flats) and all(iguards_ok(f) for f in r.iflats), "a guard word was overwritten"
    return r


def untouched(r, but=None):
    """every slot except step `but` still holds its fill"""
    ok = True
    for t in range(r.idx.shape[1] if r.idx is not None else r.patch.shape[1]):
        if t == but:
            continue
        if r.idx is not None:
            ok = ok and bool((r.idx[:, t] == IFILL).all()) and bool(torch.isnan(r.val[:, t]).all())
        if r.patch is not None:
            ok = ok and bool(torch.isnan(r.patch[:, t]).all())
    return ok


def test_the_reference_sort_puts_equal_values_in_ascending_column_order():
    x = tied_rows(4, 1029, 3)[:, :1029]
    vals, idx = torch.sort(x.double(), dim=1, descending=True, stable=True)
    ties = 0
    for b in range(4):
        v, i = vals[b, :33], idx[b, :33]
        same = v[1:] == v[:-1]
        assert bool((i[1:][same] > i[:-1][same]).all())
        ties += int(same[:31].sum())
    assert ties >= 4 * 10, "precondition: the inputs exercise the tie rule"


# n_cols = chunks * ops.TOPK_ROWS_CHUNK + extra (the width is the library's, read when the test runs); 8 C + 1: 9 chunks x 32 candidates
# outnumber stage 2's 256 threads
SHAPES = [(0, 1), (0, 7), (0, 113), (0, 1029), (1, -1), (1, 0), (1, 5), (3, 1), (8, 1)]


@pytest.mark.parametrize("chunks,extra", SHAPES, ids=[f"{c}C{e:+d}" if c else str(e) for c, e in SHAPES])
def test_topk_rows_against_the_fp64_reference(ops, chunks, extra):
    n = chunks * ops.TOPK_ROWS_CHUNK + extra
    assert ops.TOPK_ROWS_CHUNK >= 2048, "the fixed shapes 113 / 1029 are meant to lie inside one chunk"
    BMAX = 65
    x = tied_rows(BMAX, n, 1000 + n)
    # special rows (used when the batch has them): 1 all -inf, 2 exactly one candidate, 3 finished, 4 best at column 0, 5 best at column n - 1
    x[1, :n] = -INF
    x[2, :n] = -INF
    x[2, n // 2] = 2.5
    x[4, 0] = 99.0
    x[5, n - 1] = 99.0
    xd = x.cuda()
    worst = 0.0
    for k in (1, 5, 32):
        ids_ref, lp_ref = ref_topk(x[:, :n], k)
        for B in (1, 6, 65):
            unf = torch.ones(B, dtype=torch.int32)
            if B > 3:
                unf[3] = 0
            unf = unf.cuda()
            r = launch(ops, xd, n, k, unf, step=1)
            assert torch.equal(bits(xd), bits(x.cuda())), "the kernel wrote to its input rows"
            assert untouched(r, but=1), "a slot other than *step was written"
            idx, val = r.idx[:, 1].cpu().long(), r.val[:, 1].cpu()
            live = torch.ones(B, dtype=torch.bool)
            if B > 3:
                live[3] = False
                assert bool((idx[3] == -1).all()) and bool((val[3] == -INF).all()), "a finished row must hold -1 / -inf"
            assert torch.equal(idx[live], ids_ref[:B][live]), f"ids differ from the stable sort (n={n} k={k} B={B})"
            worst = max(worst, within(val[live], lp_ref[:B][live]))
            if B > 5:
                assert bool((idx[1] == -1).all()) and bool((val[1] == -INF).all())
                assert idx[2, 0] == n // 2 and float(val[2, 0]) == 0.0 and bool((idx[2, 1:] == -1).all())
                assert idx[4, 0] == 0 and idx[5, 0] == n - 1
            r2 = launch(ops, xd, n, k, unf, step=1)
            assert torch.equal(r2.idx, r.idx) and torch.equal(bits(r2.val), bits(r.val)), "two launches differ"
    print(f"\n[topk rows n={n}] largest |log-prob - fp64 reference| {worst:.3e}")
    unf = torch.ones(6, dtype=torch.int32, device="cuda")
    for step in (-1, 3, 8):                                            # t_max = 3: nothing is written
        assert untouched(launch(ops, xd, n, 5, unf, step=step, p_cap=4, vrt_off=i32([0] * 7), vocab=0))


@pytest.mark.parametrize("k", [1, 5, 32])
def test_equal_kth_and_next_value_in_different_chunks_go_to_the_lower_column(ops, k):
    C = ops.TOPK_ROWS_CHUNK
    n = 2 * C + 5
    x = torch.full((2, n + 1), -INF)
    x[:, n:] = float("nan")
    big = torch.arange(k - 1, dtype=torch.float32) + 10.0
    x[0, torch.arange(k - 1) * 97 + C // 2] = big                      # k - 1 larger values, then three equal ones in three chunks
    x[0, [20, C + 10, 2 * C + 1]] = 1.0
    x[1, :n] = x[0, :n].flip(0)                                        # the mirrored row
    r = launch(ops, x.cuda(), n, k, i32([1, 1]), step=0)
    ids_ref, lp_ref = ref_topk(x[:, :n], k)
    idx = r.idx[:, 0].cpu().long()
    assert torch.equal(idx, ids_ref)
    assert idx[0, k - 1] == 20 and idx[1, k - 1] == n - 1 - (2 * C + 1)
    within(r.val[:, 0].cpu(), lp_ref)
    if k + 1 <= 32:
        r = launch(ops, x.cuda(), n, k + 1, i32([1, 1]), step=0)
        assert r.idx[0, 0, k].item() == C + 10 and r.idx[1, 0, k].item() == n - 1 - (C + 10)


@pytest.mark.parametrize("n", [113, 1029])
def test_topk_of_a_row_warped_by_sample_token(ops, n):
    g = torch.Generator().manual_seed(17 + n)
    B = 5
    x = torch.full((B, n + 3), float("nan"))
    x[:, :n] = torch.randn(B, n, generator=g) * 3
    xd = x.cuda()
    cfg = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=3, temperature=0.7, top_k=20, top_p=1.0, write_back=True)
    pv, pi, st = torch.zeros(B, device="cuda"), torch.full((B,), -5, dtype=torch.int32, device="cuda"), i32([1])
    ops.sample_token(xd, n, cfg, st, pv, pi, B)
    r = launch(ops, xd, n, 32, torch.ones(B, dtype=torch.int32, device="cuda"), step=1)
    warped = xd.cpu()[:, :n]
    kept = torch.isfinite(warped).sum(-1)
    assert bool((kept >= 1).all()) and bool((kept <= 20).all()), "precondition: the rows are the warped ones"
    idx, val = r.idx[:, 1].cpu().long(), r.val[:, 1].cpu()
    assert bool(((idx >= 0).sum(-1) == kept).all()) and bool((idx[:, 20:] == -1).all()) and bool((val[:, 20:] == -INF).all())
    ids_ref, lp_ref = ref_topk(warped, 32)
    assert torch.equal(idx, ids_ref)
    d = within(val, lp_ref)
    print(f"\n[topk warped n={n}] largest |log-prob - fp64 reference| {d:.3e}")


@pytest.mark.parametrize("k", [0, 5])
def test_patch_logprobs_with_ragged_offsets(ops, k):
    C = ops.TOPK_ROWS_CHUNK
    V, counts = C - 40, [12, 0, 30, 7, 1]                               # the patch columns straddle the first chunk boundary
    B, p_cap = len(counts), 33
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    n = V + off[-1] + 6                                                 # columns after the last sample's patches exist too
    x = tied_rows(B, n, 77)
    unf = i32([1, 1, 1, 0, 1])
    xd = x.cuda()
    r = launch(ops, xd, n, k, unf, step=2, vrt_off=i32(off), vocab=V, p_cap=p_cap)
    assert untouched(r, but=2) and torch.equal(bits(xd), bits(x.cuda()))
    ls = torch.log_softmax(x[:, :n].double(), -1)
    ref = torch.full((B, p_cap), -INF, dtype=torch.float64)
    for b, c in enumerate(counts):
        if b != 3:
            ref[b, :c] = ls[b, V + off[b]: V + off[b] + c]
    d = within(r.patch[:, 2].cpu(), ref)
    assert bool(torch.isfinite(ref).any()) and bool((ref[2, :30] == -INF).any()), "precondition: kept and removed patch columns both occur"
    print(f"\n[patch rows k={k}] largest |log-prob - fp64 reference| {d:.3e}")
    if k:                                                              # the same launch's top-k, and top-k alone (patch_lp null)
        ids_ref, lp_ref = ref_topk(x[:, :n], k)
        live = torch.tensor([0, 1, 2, 4])
        for rr in (r, launch(ops, xd, n, k, unf, step=2)):
            assert torch.equal(rr.idx[:, 2].cpu().long()[live], ids_ref[live])
            within(rr.val[:, 2].cpu()[live], lp_ref[live])
        assert rr.patch is None


def test_wrapper_refuses_what_the_library_refuses(ops):
    from padt_amd._lib import PaDTHipError
    x = torch.zeros(2, 64, device="cuda")
    unf, st = i32([1, 1]), i32([0])
    ws = torch.zeros(ops.topk_rows_workspace(64, 32, 2), dtype=torch.uint8, device="cuda")
    with pytest.raises(PaDTHipError, match="padt_topk_logprob_rows_f32"):
        ops.topk_logprob_rows(x, 64, unf, st, ws, 2, top_idx=torch.zeros(2, 3, 33, dtype=torch.int32, device="cuda"),
                              top_val=torch.zeros(2, 3, 33, device="cuda"))
    with pytest.raises(PaDTHipError, match="padt_topk_logprob_rows_f32"):
        ops.topk_logprob_rows(x, 0, unf, st, ws, 2, top_idx=torch.zeros(2, 3, 4, dtype=torch.int32, device="cuda"),
                              top_val=torch.zeros(2, 3, 4, device="cuda"))
    with pytest.raises(AssertionError):
        ops.topk_logprob_rows(x, 64, unf, st, ws, 2)


# ------------------------------------------------------------------------------------------------------------ end to end
T_NEW, SCHED, TEXT, MODES = TL.T_NEW, TL.SCHED, TL.TEXT, TL.MODES
K = 5


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model()
    return cfg, U, model, TL.two_ragged(cfg, U)


def own_patches(out, V):
    """→ per sample (first own patch column - V, count) from past_logit_mask (text columns + the sample's own patch columns)"""
    m = out.past_logit_mask[:, V:].cpu().bool()
    res = []
    for b in range(m.shape[0]):
        nz = m[b].nonzero()[:, 0]
        res.append((int(nz[0]), int(nz.numel())) if nz.numel() else (0, 0))
    return res


def check_against_scores(flagged, scored, L, eos, V, k=K, patches=True, need_early=True):
    """sequences equal; ids / values / patch log-probs from scores[t][b] up to and including the row's EOS step, the sentinels after it"""
    assert torch.equal(flagged.sequences, scored.sequences)
    tok = flagged.sequences[:, L:].cpu()
    B, T = tok.shape
    assert T == len(scored.scores)
    is_eos = torch.isin(tok, torch.tensor(eos))
    done_before = (is_eos.long().cumsum(1) - is_eos.long()) > 0
    if need_early:
        assert done_before.any() and not done_before.any(1).all(), "precondition: one row finishes before the other"
    worst = 0.0
    if k:
        ids, lp = flagged.top_token_ids, flagged.top_logprobs
        assert ids.dtype == torch.int64 and lp.dtype == torch.float32 and tuple(ids.shape) == tuple(lp.shape) == (B, T, k)
        assert ids.device == flagged.sequences.device
        ids, lp = ids.cpu(), lp.cpu()
        assert bool((ids[done_before] == -1).all()) and bool((lp[done_before] == -INF).all()), "steps after a row's EOS hold -1 / -inf"
        for t in range(T):
            ids_ref, lp_ref = ref_topk(scored.scores[t].cpu(), k)
            live = ~done_before[:, t]
            assert torch.equal(ids[live, t], ids_ref[live]), f"step {t}: ids differ from the stable sort of the scores"
            worst = max(worst, within(lp[live, t], lp_ref[live]))
    else:
        assert flagged.top_token_ids is None and flagged.top_logprobs is None
    if patches:
        pl = flagged.patch_logprobs
        own = own_patches(flagged, V)
        P = max(c for _, c in own)
        assert pl.dtype == torch.float32 and tuple(pl.shape) == (B, T, P)
        pl = pl.cpu()
        assert bool((pl[done_before] == -INF).all())
        for t in range(T):
            ls = torch.log_softmax(scored.scores[t].cpu().double(), -1)
            ref = torch.full((B, P), -INF, dtype=torch.float64)
            for b, (o, c) in enumerate(own):
                if not done_before[b, t]:
                    ref[b, :c] = ls[b, V + o: V + o + c]
            worst = max(worst, within(pl[:, t], ref))
    else:
        assert flagged.patch_logprobs is None
    return worst


def flagged_vs_scored(model, cfg, kw, gen, k=K, patches=True, **extra):
    eos = TL.early_eos(model, cfg, kw, gen)
    flagged = model.generate(top_logprobs=k, output_patch_logprobs=patches, eos_token_id=eos, **gen, **kw, **extra)
    assert flagged.scores is None
    scored = model.generate(output_scores=True, eos_token_id=eos, **gen, **kw)
    assert scored.top_token_ids is None and scored.top_logprobs is None and scored.patch_logprobs is None
    return check_against_scores(flagged, scored, kw["input_ids"].shape[1], eos, cfg.vocab_size, k, patches), flagged, eos


@pytest.mark.parametrize("mode", list(MODES))
def test_generate_top_and_patch_logprobs_equal_the_scores(setup, mode):
    cfg, U, model, kw = setup
    d, flagged, eos = flagged_vs_scored(model, cfg, kw, MODES[mode], output_token_logprobs=True)
    print(f"\n[generate {mode}] largest |top / patch log-prob - log_softmax(scores)| {d:.3e}")
    L = kw["input_ids"].shape[1]
    tok = flagged.sequences[:, L:].cpu()
    is_eos = torch.isin(tok, torch.tensor(eos))
    live = ~((is_eos.long().cumsum(1) - is_eos.long()) > 0)           # up to and including the row's EOS step: from the tokens, not from the outputs
    ids, lp, tlp = flagged.top_token_ids.cpu(), flagged.top_logprobs.cpu(), flagged.token_logprobs.cpu()
    if "do_sample" not in MODES[mode]:                                # greedy: entry 0 is the generated token, its value the token's log-prob
        assert torch.equal(flagged.top_token_ids[..., 0].cpu()[live], tok[live])
        within(flagged.top_logprobs[..., 0].cpu()[live], flagged.token_logprobs.cpu()[live])
    else:                                                              # the warpers bite: top_k = 20 leaves K = 5 finite, the drawn token among the kept
        assert bool(torch.isfinite(lp[..., 0][live]).all()) and bool((tlp[live] <= lp[..., 0][live] + 1e-5).all()), "the drawn token beats the best candidate"
        hit = (ids == tok[..., None]) & live[..., None]              # where the drawn token is among the K best, its slot holds the token's log-prob
        assert hit.any() and bool((hit.sum(-1) <= 1).all())
        within(lp[hit], tlp[..., None].expand_as(lp)[hit])
    if mode == "schedule":                                             # 'v' steps: only own patch columns survive, and they carry all the mass
        v_steps = [t for t, m in enumerate(SCHED) if m == "v" and t < tok.shape[1]]
        p = flagged.patch_logprobs.cpu()[:, v_steps].double().exp().sum(-1)
        ids = flagged.top_token_ids.cpu()[:, v_steps]
        rows = live[:, v_steps]
        assert rows.any() and bool(((p[rows] - 1).abs() < 1e-4).all()) and bool((ids[rows] >= cfg.vocab_size).all())
        if tok.shape[1] == T_NEW:                                      # the forced EOS: one candidate, log-prob exactly 0, the rest -1 / -inf
            last = flagged.top_token_ids[:, -1].cpu()
            lrow = live[:, -1]
            assert bool((last[lrow][:, 1:] == -1).all()) and float(flagged.top_logprobs[:, -1, 0].cpu()[lrow].abs().max()) == 0.0


@pytest.mark.parametrize("k,patches", [(3, False), (0, True), (32, False)])
def test_the_two_flags_are_independent(setup, k, patches):
    cfg, U, model, kw = setup
    d, flagged, _ = flagged_vs_scored(model, cfg, kw, MODES["schedule"], k=k, patches=patches)
    assert flagged.token_logprobs is None
    print(f"\n[generate k={k} patches={patches}] largest difference {d:.3e}")


def test_flags_off_fields_are_none_and_the_value_policy_holds(setup):
    cfg, U, model, kw = setup
    out = model.generate(max_new_tokens=4, **kw)
    for name in ("top_token_ids", "top_logprobs", "patch_logprobs"):
        assert name in out and out[name] is None
    out = model.generate(max_new_tokens=4, top_logprobs=0, **kw)
    assert out.top_token_ids is None
    with pytest.raises(ValueError, match="top_logprob"):
        model.generate(max_new_tokens=4, top_logprob=3, **kw)
    with pytest.raises(ValueError, match="top_logprobs"):
        model.generate(max_new_tokens=4, top_logprobs=-2, **kw)
    with pytest.raises(ValueError, match="top_logprobs"):
        model.generate(max_new_tokens=4, top_logprobs=2.5, **kw)
    with pytest.raises(NotImplementedError, match="top_logprobs=33"):
        model.generate(max_new_tokens=4, top_logprobs=33, **kw)
    via_cfg = model.generate(max_new_tokens=4, generation_config={"top_logprobs": 2, "output_patch_logprobs": True}, **kw)
    assert tuple(via_cfg.top_token_ids.shape[::2]) == (2, 2) and via_cfg.patch_logprobs is not None
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(max_new_tokens=4, generation_config={"top_logprobs": 2, "num_beams": 4}, **kw)


def test_generate_with_image_index(setup):
    cfg, U, model, _ = setup
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8]], n_pre=6, n_post=9, seed=93)
    ids = ids.repeat(2, 1)
    ids[1, -4:] = torch.tensor([5, 6, 7, 8])
    kw = dict(input_ids=ids.cuda(), attention_mask=am.repeat(2, 1).cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, image_index=[0, 0])
    d, _, _ = flagged_vs_scored(model, cfg, kw, dict(max_new_tokens=T_NEW, schedule=SCHED))
    print(f"\n[generate image_index] largest difference {d:.3e}")


def test_generate_reference_precision():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model(precision="reference")
    d, _, _ = flagged_vs_scored(model, cfg, TL.two_ragged(cfg, U), dict(max_new_tokens=T_NEW, schedule=SCHED))
    print(f"\n[generate precision=reference] largest difference {d:.3e}")


def test_merged_decode_group_equals_each_batch_alone(setup):
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
    gen = dict(max_new_tokens=T, schedule=sched, top_logprobs=K, output_patch_logprobs=True)
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], **gen) for b in batches]
    plain = pipeline.rec_batch(model, proc, batches[0][0].clone(), *batches[0][1:], max_new_tokens=T, schedule=sched)
    assert not any(name in plain[0] for name in ("top_token_ids", "top_logprobs", "patch_logprobs"))
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b in batches:
        got += runner.submit(b[0].clone(), *b[1:], **gen)
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2
    for s, ((d0, c0, l0, v0), (d1, c1, l1, v1)) in enumerate(zip(alone, got)):
        assert c0 == c1 and v0 == v1, "tokens of the merged group differ from the batch alone"
        n_own = sum(int(g[0] * g[1] * g[2]) // 4 for g in batches[s][3].tolist())
        assert tuple(d1["top_token_ids"].shape) == (2, T, K) and d1["top_token_ids"].dtype == torch.int64
        assert torch.equal(d1["top_token_ids"], d0["top_token_ids"]), "ids of the merged group are not in the batch's own numbering"
        ids = d1["top_token_ids"]
        assert bool((ids >= cfg.vocab_size).any()) and int(ids.max()) < cfg.vocab_size + n_own
        d = max(within(d1["top_logprobs"], d0["top_logprobs"]), within(d1["patch_logprobs"], d0["patch_logprobs"]))
        assert d1["patch_logprobs"].shape == d0["patch_logprobs"].shape and bool(torch.isfinite(d1["patch_logprobs"]).any())
        print(f"\n[merged group] largest |merged - alone| {d:.3e}")
    # batches that disagree on either flag never share a group
    for other in (dict(top_logprobs=K), dict(top_logprobs=3, output_patch_logprobs=True), dict()):
        runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
        got = runner.submit(batches[0][0].clone(), *batches[0][1:], **gen)
        got += runner.submit(batches[1][0].clone(), *batches[1][1:], max_new_tokens=T, schedule=sched, **other)
        got += runner.flush()
        assert runner.n_groups == 2 and len(got) == 2
        assert torch.equal(got[0][0]["top_token_ids"], alone[0][0]["top_token_ids"])
        assert ("patch_logprobs" in got[1][0]) == ("output_patch_logprobs" in other) and ("top_logprobs" in got[1][0]) == ("top_logprobs" in other)


def test_generate_launch_collect_all_batches_carry_the_fields(setup):
    cfg, U, model, kw = setup
    args = (kw["input_ids"], kw["attention_mask"], kw["pixel_values"], kw["image_grid_thw"])
    gen = dict(max_new_tokens=6, top_logprobs=4, output_patch_logprobs=True)
    ctx = model.generate_launch(*args, n_slots=2, lane=3, **gen)
    ctx = model.generate_launch(*args, n_slots=2, lane=3, group=ctx, **gen)
    outs = model.generate_collect(ctx, all_batches=True)
    alone = model.generate(**gen, **kw)
    assert len(outs) == 2
    for o in outs:
        assert torch.equal(o.sequences, alone.sequences) and torch.equal(o.top_token_ids, alone.top_token_ids)
        within(o.top_logprobs, alone.top_logprobs)
        within(o.patch_logprobs, alone.patch_logprobs)
    keep = alone.top_logprobs.clone(), alone.top_token_ids.clone(), alone.patch_logprobs.clone()      # the caller owns what it got
    model.generate(schedule=["e"] * 6, **gen, **kw)
    assert torch.equal(keep[0], alone.top_logprobs) and torch.equal(keep[1], alone.top_token_ids) and torch.equal(keep[2], alone.patch_logprobs)


def same_output(a, b):
    """every returned field of two generate() results is bit-equal (the session itself aside)"""
    assert a.keys() == b.keys()
    for name in a:
        x, y = a[name], b[name]
        if name == "past_key_values":
            continue
        if name == "hidden_states":
            x, y = x.last_layer_rows(), y.last_layer_rows()
        if isinstance(x, (tuple, list)):
            assert len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y)), name
        else:
            assert (x is None and y is None) or torch.equal(x, y), name


def test_mode_changes_on_one_lane_replay_what_the_eager_steps_compute(setup):
    """One lane's session goes through plain → top_logprobs → output_patch_logprobs on a small image → on a larger one (the patch buffer grows:
    the graphs captured over the outgrown one must go) → the small one again → plain, with captured steps; every result equals the same call
    with eager steps on another lane.  The first call sizes the session for the larger image, so all six share ONE session and its graphs."""
    cfg, U, model, _ = setup
    def batch(g, seed):
        grid, pix, ids, am = U.synthetic_batch(cfg, [g], n_pre=6, n_post=9, seed=seed)
        return dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    small, large = batch([1, 4, 4], 71), batch([1, 8, 8], 72)
    calls = [(large, dict()), (large, dict(top_logprobs=3)), (small, dict(output_patch_logprobs=True)), (large, dict(output_patch_logprobs=True)),
             (small, dict(output_patch_logprobs=True)), (large, dict())]
    sessions, p_caps, n_graphs = [], [], []
    for kw, gen in calls:
        got = model.generate(max_new_tokens=5, sync_every=2, use_graph=True, lane=11, **gen, **kw)
        sess = got.past_key_values
        sessions.append(sess)
        p_caps.append(sess.p_cap)
        n_graphs.append(len(sess.graphs))
        same_output(got, model.generate(max_new_tokens=5, sync_every=2, use_graph=False, lane=12, **gen, **kw))
        if "output_patch_logprobs" in gen:
            assert bool(torch.isfinite(got.patch_logprobs[:, 0]).any())
    assert all(s is sessions[0] for s in sessions), "the lane's session was replaced: the patch buffer did not grow inside one session"
    assert p_caps[2] < p_caps[3] == p_caps[4], p_caps                # the buffer grew once ...
    assert n_graphs == [1, 2, 3, 3, 3, 3], n_graphs                  # ... and took the graph captured over the smaller one with it


def test_range_guard_rerun_on_the_bf16_twin_carries_the_fields():
    """operands="auto": the batch whose SwiGLU hidden exceeds fp16's range is answered by the bf16 twin — with the new fields, equal to the
    reference of the bf16 model's own scores (the weights of test_token_logprobs_gpu.py's re-run test)"""
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
    eos = TL.early_eos(ref, cfg, kw, gen)
    scored = ref.generate(output_scores=True, eos_token_id=eos, **gen, **kw)
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(top_logprobs=K, output_patch_logprobs=True, eos_token_id=eos, **gen, **kw)
    assert auto.overflow_reruns == 1 and got.top_token_ids is not None and got.patch_logprobs is not None
    d = check_against_scores(got, scored, ids.shape[1], eos, cfg.vocab_size)
    print(f"\n[range-guard re-run] largest difference {d:.3e}")


# ------------------------------------------------------------------------------------------------------------ what is launched
NEW_WRAPPERS = ("topk_logprob_rows", "topk_rows_workspace")            # the launch, and the size query of the session's first allocation


def _recorded(monkeypatch, ops, model, kw, **gen):
    """the ops wrappers a generate goes through, in order; a vrt_head call that writes the logits row is marked '+logits'"""
    calls = []
    with monkeypatch.context() as mp:
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_"):
                def stub(*a, _fn=fn, _name=name, **k):
                    calls.append(_name + ("+logits" if _name == "vrt_head" and k.get("logits") is not None else ""))
                    return _fn(*a, **k)
                mp.setattr(ops, name, stub)
        out = model.generate(use_graph=False, **gen, **kw)
    return calls, out


@pytest.mark.parametrize("mode", ["captured_greedy", "sampling"])
def test_the_flags_add_one_launch_per_step_and_the_heads_row_output(setup, ops, monkeypatch, mode):
    cfg, U, model, kw = setup
    gen = {k: v for k, v in MODES[mode].items() if k != "use_graph"}
    plain, a = _recorded(monkeypatch, ops, model, kw, **gen)
    off, a2 = _recorded(monkeypatch, ops, model, kw, top_logprobs=None, output_patch_logprobs=False, **gen)
    assert off == plain and a2.top_token_ids is None and a2.patch_logprobs is None
    assert not any(c in NEW_WRAPPERS for c in plain)
    if mode == "captured_greedy":
        assert "vrt_head+logits" not in plain                         # plain greedy decoding writes no row
    flagged, b = _recorded(monkeypatch, ops, model, kw, top_logprobs=K, output_patch_logprobs=True, **gen)
    assert torch.equal(a.sequences, b.sequences)
    n_steps = b.top_token_ids.shape[1]
    assert [c.replace("+logits", "") for c in flagged if c not in NEW_WRAPPERS] == [c.replace("+logits", "") for c in plain]
    assert flagged.count("topk_logprob_rows") == sum(c.startswith("vrt_head") and "nblk" not in c for c in flagged) >= n_steps
    assert flagged.count("topk_rows_workspace") <= 1
    assert all(c == "vrt_head+logits" for c in flagged if c.startswith("vrt_head") and "nblk" not in c)
