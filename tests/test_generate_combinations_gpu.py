"""generate()'s options in combination, on the device: where the kernel families meet (DecodeSession.head_and_select).

Every row of the covering array (generate_combinations_util.build_array: 11 factors, every pair of levels in some row) is run twice on ONE
small synthetic model, one decode session, two ragged samples, 12 steps: with the options as generate() arguments (the captured step, the
fused heads, the device-side bans / automaton / bias / decay), and on the HOOKED loop, which runs none of those kernels — the plain head
writes the row and HF's own processor classes (generate_combinations_util.reference_processors, pinned to generation.score_bias_row on the
CPU) rewrite it.  Selection (arg-max / sampler / warpers, pinned to HF's warpers at kernel level elsewhere), forced tokens and the schedule
are on both sides and are checked directly: against torch.argmax of the row, the row's finite support, the forced table.

Bounds: score rows, sequences, hidden rows, top / patch log-probs between the two runs are compared bit for bit (the same kernels on equal
rows); log-probs against fp64 log_softmax of the reference's row within test_token_logprobs_gpu.within (5e-6 + 2^-22 |ref|, derived there).

Then, over the array as a whole: every factor that edits a score or the selection changes some run when switched off (`outputs` and
`execution` are left out on purpose: they must change nothing, see that test), two rows end one sample early, the device calls
give bit-identical results in array order and in reverse order on the one session (a buffer one mode leaves dirty for another shows there),
and the rows of the cover run through merged decode groups (PipelinedRunner(merge=2)) equal each batch alone."""
import types

import pytest
import torch

import generate_combinations_util as C
import test_score_bias_gpu as SB
import test_token_logprobs_gpu as TL
import test_top_logprobs_gpu as TK

pytestmark = pytest.mark.gpu

INF = float("inf")
ROWS = C.build_array()
IDS = [C.row_id(i, r) for i, r in enumerate(ROWS)]
T_NEW = C.T_NEW


def bits(t):
    return t.contiguous().view(torch.int32)


def make_setup(operands="auto"):
    """the model (MFMA operand type `operands`), the two ragged samples, the session every call of the module shares, and the levels' values"""
    from transformers.generation.logits_process import ExponentialDecayLengthPenalty
    cfg, U, model = TL.small_model(operands=operands)
    kw = TL.two_ragged(cfg, U)
    L = kw["input_ids"].shape[1]
    first = model.generate(max_new_tokens=T_NEW, output_scores=True, **kw)      # the first call of the module: a plain generate at these shapes
    s = types.SimpleNamespace(cfg=cfg, U=U, model=model, kw=kw, L=L, sess=first.past_key_values, grids=kw["image_grid_thw"].tolist(),
                              operands=operands)
    # the second EOS id: a text id of sample 0's prompt — the repetition penalty has SEEN it, so penalty and decay meet on an EOS column — and
    # the one whose plain logit is the most negative: for a positive logit l both orders of the two edits give (1 + a) l / penalty, for a
    # negative one penalty-then-decay gives (1 - a) penalty l and decay-then-penalty (1 - a) l / penalty (a > 1)
    labels = {x for lb in C.LABELS for x in lb}
    prompt = sorted({int(t) for t in kw["input_ids"][0].tolist() if t < min(cfg.vocab_size, cfg.image_token_id) and t not in labels | {1500}})
    worst = torch.stack([sc[0].cpu() for sc in first.scores])[:, prompt].max(0).values      # per prompt id: its largest plain logit over the steps
    x = prompt[int(worst.argmin())]
    assert float(worst.min()) < 0, "precondition: no prompt id of sample 0 keeps a negative logit through the plain run"
    s.eos = [int(cfg.eos_token_id), x]
    plain = call(s, max_new_tokens=T_NEW, eos_token_id=s.eos)
    s.plain_tok = plain.sequences[:, L:].cpu()
    # the decay: the first candidate that, on the HF run itself, ends a row after `start` and before max_new_tokens and changes the run
    s.decay = None
    for start, factor in C.DECAY_CANDIDATES:
        proc = C.on_host(C.keep_minus_inf(ExponentialDecayLengthPenalty((start, factor), s.eos, L)))
        hf = call(s, max_new_tokens=T_NEW, eos_token_id=s.eos, logits_processor=[proc])
        ends = first_eos(hf.sequences[:, L:].cpu(), s.eos)
        if any(e is not None and start < e < T_NEW - 1 for e in ends) and not torch.equal(hf.sequences, plain.sequences):
            s.decay = (start, factor)
            break
    assert s.decay is not None, "precondition: no candidate (start, factor) ends a row of the HF run after `start` and before max_new_tokens"
    s.lv = C.make_levels(cfg, s.grids, s.plain_tok.tolist(), s.eos, s.decay)
    print(f"\n[combinations {operands}] eos {s.eos}  decay {s.decay}  bans {s.lv.bans}  logit_bias {s.lv.logit_bias}\n[combinations] plain run {s.plain_tok.tolist()}")
    return s


@pytest.fixture(scope="module", params=["auto", "bf16"])
def S(request):
    """everything below runs once per 16-bit operand type: the default (fp16 operands under the range guard) and bf16"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make_setup(request.param)


def call(s, **gen):
    """one generate on the shared session; the step mode as of this call rides along"""
    out = s.model.generate(**gen, **s.kw)
    assert out.past_key_values is s.sess, "the call left the module's session"
    out["step_mode"] = s.sess.mode
    return out


def first_eos(tok, eos):
    out = []
    for row in tok.tolist():
        hit = [t for t, x in enumerate(row) if x in eos]
        out.append(hit[0] if hit else None)
    return out


def live_mask(tok, eos):
    """(B, T) bool: the row had not finished before step t (its EOS step itself is live)"""
    is_eos = torch.isin(tok, torch.tensor(eos))
    return (is_eos.long().cumsum(1) - is_eos.long()) == 0


def forced_mask(case, shape):
    m = torch.zeros(shape, dtype=torch.bool)
    want = torch.full(shape, -1, dtype=torch.long)
    if case.forced is not None:
        for b, r in enumerate(case.forced):
            for t, x in enumerate(r[: shape[1]]):
                if x >= 0:
                    m[b, t], want[b, t] = True, x
    return m, want


def patch_offsets(grids):
    off = [0]
    for _, h, w in grids:
        off.append(off[-1] + (h // 2) * (w // 2))
    return off


def run_pair(s, row):
    case = C.bind(row, s.lv)
    dev = call(s, **C.device_kwargs(case))
    ref = call(s, **C.reference_kwargs(case, s.cfg, s.kw, s.L))
    return case, dev, ref


# ------------------------------------------------------------------------------------------------------------ 3. every row against its twin
@pytest.mark.parametrize("k", range(len(ROWS)), ids=IDS)
def test_row_equals_its_hooked_twin(S, k):
    s = S
    cfg, L, eos = s.cfg, s.L, s.eos
    case, dev, ref = run_pair(s, ROWS[k])
    # the modes: the device path runs the new kernels, the twin none of them
    assert dev["step_mode"] == C.expected_mode(case), dev["step_mode"]
    assert ref["step_mode"] == C.expected_mode(case, reference=True), ref["step_mode"]
    assert ref["step_mode"].processors and not (ref["step_mode"].rules or ref["step_mode"].automaton or ref["step_mode"].bias)
    # sequences and hidden rows
    tok, rtok = dev.sequences[:, L:].cpu(), ref.sequences[:, L:].cpu()
    print(f"\n[{IDS[k]}] device {tok.tolist()}\n[{IDS[k]}] hooked {rtok.tolist()}")
    assert torch.equal(dev.sequences, ref.sequences), "sequences differ"
    assert torch.equal(SB.hidden_bits(dev), SB.hidden_bits(ref)), "hidden rows differ"
    B, T = tok.shape
    assert len(ref.scores) == T
    live = live_mask(tok, eos)
    rv = torch.stack([x.cpu() for x in ref.scores], 1)            # (B, T, columns): the reference's rows
    n_cols = rv.shape[-1]
    assert n_cols == cfg.vocab_size + patch_offsets(s.grids)[-1]
    assert not bool(torch.isnan(rv[live]).any()), "the reference chain produced NaN"
    # score rows up to and including a sample's EOS step
    if case.outputs != 3:
        assert len(dev.scores) == T
        dv = torch.stack([x.cpu() for x in dev.scores], 1)
        assert not bool(torch.isnan(dv[live]).any()), "NaN in a device score row"
        assert torch.equal(dv[live] == -INF, rv[live] == -INF), "-inf at other columns than the reference"
        bad = (dv[live] != rv[live]).any(-1)
        assert not bool(bad.any()), f"{int(bad.sum())} live score rows differ from the hooked twin, first (row, step) {live.nonzero()[bad.nonzero()[0, 0]].tolist()}"
    else:
        assert dev.scores is None
    flat_rows, flat_tok = rv[live], tok[live]
    # token log-probs: fp64 log_softmax of the reference's row at the token; 0.0 after the EOS
    if case.outputs >= 1:
        want = TL.ref_logprob(flat_rows, flat_tok)
        for name, out in (("device", dev), ("hooked", ref)):
            lp = out.token_logprobs.cpu()
            assert tuple(lp.shape) == (B, T) and bool((lp[~live] == 0.0).all()), f"{name}: steps after a row's EOS must hold 0.0"
            d = TL.within(lp[live], want)
            print(f"[{IDS[k]}] {name}: largest |token_logprobs - fp64 log_softmax(reference row)| {d:.3e}")
    else:
        assert dev.token_logprobs is None
    # top-k and patch log-probs: the same kernel on rows just shown equal → the reference's bits; and fp64 log_softmax of the row
    if case.outputs == 2:
        assert torch.equal(dev.top_token_ids, ref.top_token_ids) and torch.equal(bits(dev.top_logprobs), bits(ref.top_logprobs))
        assert torch.equal(bits(dev.patch_logprobs), bits(ref.patch_logprobs))
        ids, lps = TK.ref_topk(flat_rows, C.TOP_K)
        tid, tlp, plp = dev.top_token_ids.cpu(), dev.top_logprobs.cpu(), dev.patch_logprobs.cpu()
        assert torch.equal(tid[live], ids), "top_token_ids are not the stable descending sort of the row"
        d_top = TL.within(tlp[live], lps)
        off = patch_offsets(s.grids)
        P = max(off[b + 1] - off[b] for b in range(B))
        assert tuple(plp.shape) == (B, T, P)
        ls = torch.log_softmax(rv.double(), -1)
        ls[(rv == -INF).all(-1)] = -INF                           # a row without any candidate
        want_p = torch.full((B, T, P), -INF, dtype=torch.float64)
        for b in range(B):
            want_p[b, :, : off[b + 1] - off[b]] = ls[b, :, cfg.vocab_size + off[b]: cfg.vocab_size + off[b + 1]]
        d_patch = TL.within(plp[live], want_p[live])
        assert bool((tid[~live] == -1).all()) and bool((tlp[~live] == -INF).all()) and bool((plp[~live] == -INF).all()), "sentinels after the EOS"
        print(f"[{IDS[k]}] largest |top_logprobs - fp64| {d_top:.3e}  |patch_logprobs - fp64| {d_patch:.3e}")
    else:
        assert dev.top_token_ids is None and dev.top_logprobs is None and dev.patch_logprobs is None
    # selection, independent of both runs: every live, unforced step
    forced, table = forced_mask(case, (B, T))
    empty = (rv == -INF).all(-1)
    free = live & ~forced
    assert bool((tok[free & empty] == cfg.pad_token_id).all()), "a row without a candidate continues with pad"
    pick = free & ~empty
    if case.sampling:
        assert bool(torch.isfinite(rv[pick].gather(1, tok[pick][:, None])).all()), "a drawn token lies outside the kept (warped) row's support"
    else:
        assert torch.equal(tok[pick], rv[pick].argmax(-1)), "a greedy token is not the arg-max of its row"
    # forced: the table's entry, scored at the row's log-softmax there (checked with every other log-prob above), -inf where it is a
    # banned / -inf-biased column
    hit = live & forced
    assert torch.equal(tok[hit], table[hit]), "a forced step did not emit the table's entry"
    if case.forced is not None:
        assert bool(hit[0, 0]) and bool(hit[1, 1]), "precondition: both rows are forced while live"
        if case.logit_bias is not None:
            assert bool(hit[0, 2]), "precondition: row 0 is live at its third forced step (21 and 23 are no EOS ids)"
            assert case.forced[0][2] == 24 and rv[0, 2, 24] == -INF
            if case.outputs >= 1:
                assert float(dev.token_logprobs[0, 2]) == -INF and int(tok[0, 2]) == 24
    # the automaton: every live, unforced token of a row with a candidate is one allowed() admits
    if case.automaton is not None:
        import test_token_automaton_gpu as TAG
        A, rng = case.automaton, TAG.patch_ranges(s.kw["image_grid_thw"])
        for b in range(B):
            row = tok[b].tolist()
            clean = True
            for t in range(T):
                if not live[b, t]:
                    break
                ok = A.allowed(row[:t], cfg.vocab_size, rng[b], eos)
                fin = torch.isfinite(rv[b, t]).nonzero().flatten().tolist()
                assert set(fin) <= set(ok), (b, t, "a column outside allowed() is finite")
                if forced[b, t] or empty[b, t]:
                    clean = clean and row[t] in ok
                else:
                    assert row[t] in ok, (b, t, row)
            if clean:
                assert A.accepts(row, cfg.vocab_size, rng[b], eos), (b, row)
    # the patch trio (automaton + patch bias + patch log-probs) without the schedule: sample 1, the one with the prior, stands in a VRT state
    # while live — the step's candidates are its own patch columns and nothing else, none of them one the prior sets to -inf — and emits
    # one; its patch log-probs are finite exactly on the kept columns
    if C.is_patch_trio(ROWS[k]) and case.schedule is None:
        off = patch_offsets(s.grids)
        lo, hi = cfg.vocab_size + off[1], cfg.vocab_size + off[2]
        fin = torch.isfinite(rv[1])
        vrt = live[1] & fin[:, lo:hi].any(-1) & ~fin[:, :lo].any(-1) & ~fin[:, hi:].any(-1)
        assert bool(vrt.any()), f"precondition: sample 1 of {IDS[k]} never stands in a VRT state while live: {tok[1].tolist()}"
        prior = torch.isfinite(case.patch_bias[1].reshape(-1))
        assert not bool(prior.all()) and bool(prior.any())
        for t in vrt.nonzero().flatten().tolist():
            kept = fin[t, lo:hi]                                   # under sampling the kept row is the warped one: a subset of the prior's
            assert not bool((kept & ~prior).any()) and (case.sampling or torch.equal(kept, prior)), (t, kept.tolist())
            assert lo <= int(tok[1, t]) < hi, (t, int(tok[1, t]))
        assert torch.equal(torch.isfinite(dev.patch_logprobs[1].cpu()[vrt][:, : hi - lo]), fin[vrt][:, lo:hi])
        print(f"[{IDS[k]}] sample 1 in a VRT state at steps {vrt.nonzero().flatten().tolist()}")


# ------------------------------------------------------------------------------------------------------------ 4. the array must bite
def test_every_editing_factor_changes_some_run_and_two_rows_end_one_sample_early(S):
    """A deliberate deviation from "for each factor": the loop is over generate_combinations_util.EDITING, nine of the eleven factors.
    `outputs` and `execution` choose what is returned and how the step is launched; switching them must change NO sequence and NO score
    row, which is what every row's comparison with its hooked twin (always eager, always keeping rows) asserts instead."""
    s = S
    L = s.L

    def changed(a, b):
        if not torch.equal(a.sequences, b.sequences):
            return True
        live = live_mask(a.sequences[:, L:].cpu(), s.eos)
        x, y = torch.stack(list(a.scores), 1).cpu(), torch.stack(list(b.scores), 1).cpu()
        return not torch.equal(bits(x[live]), bits(y[live]))
    for factor in C.EDITING:
        bites = False
        for k, row in enumerate(ROWS):
            if not getattr(row, factor):
                continue
            on = call(s, **dict(C.device_kwargs(C.bind(row, s.lv)), output_scores=True))
            off = call(s, **dict(C.device_kwargs(C.bind(C.switched_off(row, factor), s.lv)), output_scores=True))
            if changed(on, off):
                print(f"\n[bite] {factor}: off changes {IDS[k]}")
                bites = True
                break
        assert bites, f"precondition: switching {factor} off changes no row of the array: strengthen the level"
    early = []
    for k, row in enumerate(ROWS):
        tok = call(s, **C.device_kwargs(C.bind(row, s.lv))).sequences[:, L:].cpu()
        ends = first_eos(tok, s.eos)
        done = sorted(e for e in ends if e is not None)
        if done and ends[0] != ends[1] and done[0] + 1 < T_NEW:
            early.append((IDS[k], ends))
    print(f"\n[early] {early}")
    assert len(early) >= 2, f"precondition: one sample finishes before the other and before max_new_tokens in {len(early)} rows only"


# ------------------------------------------------------------------------------------------------------------ 5. order independence
def snapshot(out):
    d = dict(sequences=out.sequences.cpu(), hidden=SB.hidden_bits(out).cpu())
    if out.scores is not None:
        d["scores"] = bits(torch.stack(list(out.scores))).cpu()
    for name in ("token_logprobs", "top_logprobs", "patch_logprobs"):
        if out[name] is not None:
            d[name] = bits(out[name]).cpu()
    if out.top_token_ids is not None:
        d["top_token_ids"] = out.top_token_ids.cpu()
    return d


def test_device_calls_in_array_order_and_in_reverse_give_the_same_bits(S):
    """Both passes on ONE new model: its session has seen nothing when the first pass starts — every buffer is allocated by the first mode
    that needs it — and everything when the second pass starts.  (On the module's own session a buffer that is never cleared would already
    hold every earlier test's values in both passes, and the passes would agree.)"""
    cfg, U, model = TL.small_model(operands=S.operands)
    first = model.generate(max_new_tokens=T_NEW, **S.kw)           # the session's geometry: the plain call at these shapes
    s = types.SimpleNamespace(model=model, kw=S.kw, sess=first.past_key_values, lv=S.lv)
    cases = [C.bind(r, s.lv) for r in ROWS]
    forward = [snapshot(call(s, **C.device_kwargs(c))) for c in cases]
    n_graphs = len(s.sess.graphs)
    backward = [None] * len(cases)
    for k in reversed(range(len(cases))):
        backward[k] = snapshot(call(s, **C.device_kwargs(cases[k])))
    assert len(s.sess.graphs) == n_graphs, "the second pass captured a graph the first had not"
    assert n_graphs >= len({C.expected_mode(c) for c in cases if c.use_graph})
    for k, (a, b) in enumerate(zip(forward, backward)):
        assert set(a) == set(b)
        for name in a:
            assert a[name].shape == b[name].shape and torch.equal(a[name], b[name]), \
                f"{IDS[k]}: {name} depends on which calls ran before it on the session"


# ------------------------------------------------------------------------------------------------------------ 6. merged decode groups
MERGED_GRIDS = ([[1, 8, 8], [1, 10, 12]], [[1, 6, 10], [1, 8, 8]], [[1, 10, 8], [1, 6, 8]])
MERGED_FORCED = ([[21, 23, 24], [-1, 23]], [[-1, 22], [31, 32, 40]], [[21, 22], [-1, -1, 24]])
COVER = C.cover_rows(ROWS)
assert any(C.is_patch_trio(ROWS[k]) for k in COVER), "no row of the cover has the automaton, the patch bias and the patch log-probs on together"


def make_merged(operands="auto"):
    """a model of its own (the batches' shapes would regrow the module's session), three batches of different grids"""
    cfg, U, model = TL.small_model(operands=operands)
    batches = []
    for i, g in enumerate(MERGED_GRIDS):
        grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5 + 3 * (i % 2), n_post=7, seed=100 + i, ragged=True)
        batches.append((ids.cuda(), am.cuda(), pix.cuda(), grid))
    return cfg, U, model, SB.make_processor(cfg, U), batches


@pytest.fixture(scope="module")
def merged(S):
    return make_merged(S.operands)


@pytest.mark.parametrize("k", COVER, ids=[IDS[k] for k in COVER])
def test_merged_decode_groups_equal_each_batch_alone(S, merged, k):
    from padt_amd import pipeline
    cfg, U, model, proc, batches = merged
    per_batch = []
    for i, g in enumerate(MERGED_GRIDS):                           # each batch its own forced table and patch prior; the rest is shared
        lv = types.SimpleNamespace(**vars(S.lv))
        lv.forced = MERGED_FORCED[i]
        lv.patch_bias = [None, C.patch_map(g[1][1] // 2, g[1][2] // 2, shift=i)]
        per_batch.append(C.device_kwargs(C.bind(ROWS[k], lv)))
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], **gen) for b, gen in zip(batches, per_batch)]
    use_graph = per_batch[0]["use_graph"]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2, use_graph=use_graph)
    got = []
    for b, gen in zip(batches, per_batch):
        sub = {n: v for n, v in gen.items() if n not in ("use_graph", "output_scores")}      # the runner's own spellings of the two
        got += runner.submit(b[0].clone(), *b[1:], keep_scores=gen["output_scores"], **sub)
    got += runner.flush()
    assert runner.n_groups == 2 and len(got) == 3, "three batches with equal options: a group of two and a group of one"
    n_obj = 0
    level = ROWS[k].outputs                                      # what the decoded dicts must carry, so that the comparisons below run
    fields = ("token_logprobs",) * (level >= 1) + ("top_token_ids", "top_logprobs", "patch_logprobs") * (level == 2)
    for i, ((d0, c0, l0, v0), (d1, c1, l1, v1)) in enumerate(zip(alone, got)):
        assert {n for n in ("token_logprobs", "top_token_ids", "top_logprobs", "patch_logprobs") if n in d0} == set(fields), f"batch {i}: {sorted(d0)}"
        assert c0 == c1 and l0 == l1 and v0 == v1, f"batch {i}: completions / labels / VRTs of the merged group differ from the batch alone"
        for name in ("pred_boxes", "pred_mask", "pred_score"):
            assert torch.equal(d0[name], d1[name]), f"batch {i}: {name}"
        n_obj += d0["pred_boxes"].shape[0]
        for name in ("token_logprobs", "top_logprobs", "patch_logprobs"):
            assert (name in d0) == (name in d1)
            if name in d0:
                assert torch.equal(bits(d0[name]), bits(d1[name])), f"batch {i}: {name}"
        assert ("top_token_ids" in d0) == ("top_token_ids" in d1)
        if "top_token_ids" in d0:
            assert torch.equal(d0["top_token_ids"], d1["top_token_ids"]), f"batch {i}: top_token_ids"
    print(f"\n[merged {IDS[k]}] {n_obj} decoded objects; completions {[c for _, c, _, _ in got]}")


# ------------------------------------------------------------------------------------------------------------ 7. what the combinations found, kernel level
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def test_a_row_whose_best_value_is_minus_inf_continues_with_pad(ops):
    """Found by r04 (automaton + bans + bias on the hooked twin): padt_argmax_rows_f32 answers column 0 for a row without a finite entry, as
    torch.argmax does, and padt_greedy_step emitted token 0 where every other path — the head's partials, both samplers — emits pad."""
    import test_token_selection_gpu as TS
    pad, n = 17, 40
    x = torch.full((3, n), -INF, device="cuda")
    x[1, 5] = 2.0
    pv, pi = torch.zeros(3, device="cuda"), torch.full((3,), -5, dtype=torch.int32, device="cuda")
    ops.argmax_rows(x, n, pv, pi, 3)
    assert pi.tolist() == [0, 5, 0] and pv.tolist() == [-INF, 2.0, -INF]           # torch.argmax's answer stays
    loop = TS.Loop(3, 2)
    loop.run(pv, pi, 1, -1, pad)
    assert loop.cur.tolist() == [pad, 5, pad] and loop.tok[:, 0].tolist() == [pad, 5, pad]
    assert loop.unf.tolist() == [1, 1, 1], "a row without a candidate is not finished"


def test_keyed_sampler_draws_in_a_group_what_each_batch_draws_alone(ops):
    """Found by the merged run of r01 (sampling without the later warpers): padt_sample_token keyed its generator by the session's row and
    column, so the second batch of a merged decode group drew other tokens than alone.  padt_sample_token_keyed uses the numbering the batch
    has alone, as padt_warp_sample_rows_f32 does."""
    from padt_amd._lib import load
    vocab, counts = 96, ([5, 7], [4, 9])                            # two batches of two rows, ragged patch counts
    p0 = [0, sum(counts[0])]
    n_group = vocab + sum(counts[0]) + sum(counts[1])
    vrt_off = TL.i32([0, 5, 12, 16, 25])
    row_base = TL.i32([0, 0, 2, 2])
    g = torch.Generator().manual_seed(7)
    alone, group = [], torch.full((4, n_group), -INF)
    for k, c in enumerate(counts):
        x = torch.randn(2, vocab + sum(c), generator=g) * 3
        x[0, vocab + c[0]:], x[1, vocab: vocab + c[0]] = -INF, -INF  # the logit mask: a row's own patches only
        alone.append(x)
        group[2 * k: 2 * k + 2, :vocab] = x[:, :vocab]
        group[2 * k: 2 * k + 2, vocab + p0[k]: vocab + p0[k] + sum(c)] = x[:, vocab:]
    cfg = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=3, temperature=1.3, top_k=0, top_p=1.0)
    unkeyed_differs = n_vrt = 0
    for step in range(12):
        st = TL.i32([step])
        want = []
        for k, x in enumerate(alone):
            pv, pi = torch.zeros(2, device="cuda"), torch.full((2,), -5, dtype=torch.int32, device="cuda")
            ops.sample_token(x.cuda(), x.shape[1], cfg, st, pv, pi, 2)
            want += [i if i < vocab else i + p0[k] for i in pi.tolist()]
        pv, pi = torch.zeros(4, device="cuda"), torch.full((4,), -5, dtype=torch.int32, device="cuda")
        ops.sample_token(group.cuda(), n_group, cfg, st, pv, pi, 4, vocab=vocab, vrt_off=vrt_off, row_base=row_base)
        assert pi.tolist() == want, f"step {step}: the group's draws are not the batches' own"
        n_vrt += sum(i >= vocab for i in want[2:])
        ops.sample_token(group.cuda(), n_group, cfg, st, pv, pi, 4)
        assert pi.tolist()[:2] == want[:2]                             # the first batch's numbering is the session's
        unkeyed_differs += pi.tolist()[2:] != want[2:]
    assert unkeyed_differs >= 6 and n_vrt >= 1, "precondition: the key decides the second batch's draws, patch columns among them"
    lib, P_ = load(), 4096                                            # fake non-null pointers: refused on the host
    assert lib.padt_sample_token_keyed(0, P_, 128, 121, P_, 0, P_, P_, 4, vocab, 0, P_) == -1 and b"padt_sample_token_keyed" in lib.padt_last_error()
    assert lib.padt_sample_token_keyed(0, P_, 128, 121, P_, 0, P_, P_, 4, 122, P_, P_) == -1
    assert lib.padt_sample_token_keyed(0, P_, 128, 121, 0, 0, P_, P_, 4, vocab, P_, P_) == -1
    assert lib.padt_sample_token_keyed(0, P_, 128, 121, 0, 0, P_, P_, 0, vocab, P_, P_) == 0
