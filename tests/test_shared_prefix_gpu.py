"""generate(image_index=): several queries on one image share its ViT pass and their common prompt prefix inside one call.

The contract is "what the same call returns on the expanded inputs" (the image's patches repeated per sample, image_grid_thw[image_index], no
index).  Kernel level: padt_llm_qkv_post_shared is padt_llm_qkv_post plus data movement (bit equality in poisoned buffers).  End to end (the
small synthetic model of test_e2e_gpu.py, shared_prefix_util.shared_case: 7 queries over 3 images): against the fp32 oracle run on the
EXPANDED inputs with test_e2e_gpu.py's bounds, and against the expanded call on the same model."""
import dataclasses

import pytest
import torch

from shared_prefix_util import shared_case

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
T_NEW = 12


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------ the fan-out kernel
PREFIX_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)      # destination slots on both sides of the 16- and 32-slot block edges


@pytest.mark.parametrize("head_dim", [128, 64])
@pytest.mark.parametrize("cache_packed", [0, 1])
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
def test_qkv_post_shared_is_qkv_post_plus_data_movement(dt, cache_packed, head_dim):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops
    Hq, Hkv, D, S, B = 4, 2, head_dim, 96, 4
    sec = (16, 24, 24) if D == 128 else (8, 12, 12)
    inv = (1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))).cuda()
    g = torch.Generator().manual_seed(1234 + D + cache_packed)
    poison = lambda *shape: torch.full(shape, 0x7B3D, dtype=torch.int16, device="cuda").view(dt)
    for case, P in enumerate(PREFIX_LENGTHS):
        fan = 1 + case % 4                                        # fan-outs 1 .. 4
        n_own = 3 if P + 3 <= S else 0
        # token list: P prefix tokens (one destination per member), then n_own own tokens per member (one destination each)
        dests = [[(m, j) for m in range(fan)] for j in range(P)] + [[(m, P + j)] for m in range(fan) for j in range(n_own)]
        T = len(dests)
        qkv = (torch.randn(T, (Hq + 2 * Hkv) * D, generator=g) * 2).to(dt).cuda()
        pos = torch.randint(0, 600, (3, T), generator=g, dtype=torch.int32).cuda()
        # reference: padt_llm_qkv_post on the duplicated token list, one copy of the row per destination
        dup_tok = [t for t, d in enumerate(dests) for _ in d]
        dup_sample = [m for d in dests for m, _ in d]
        dup_slot = [s for d in dests for _, s in d]
        n_dup = len(dup_tok)
        n_join = n_dup + P + 2                                    # + join-only copies of the prefix (its own key segment) + 2 rows nobody writes
        perm = torch.randperm(n_join, generator=g).tolist()       # join rows in no particular order
        dup_idx = torch.tensor(dup_tok, device="cuda")
        q_ref, kp = poison(n_dup, Hq * D), poison(n_dup, Hkv * D)
        kc_ref, vt_ref = poison(B, Hkv, S, D), poison(B, Hkv, D, S)
        qkv_dup = qkv[dup_idx].contiguous()
        ops.llm_qkv_post(qkv_dup, pos[:, dup_idx].contiguous(), inv, q_ref, kc_ref, vt_ref, Hq, Hkv, D, S, sec, sample=i32(dup_sample),
                         slot=i32(dup_slot), k_pack=kp, cache_packed=bool(cache_packed))
        # the fan-out call; besides the real destinations: per prefix token one join-only entry (sample -1), and entries that must be skipped
        off, d_sample, d_slot, d_row = [0], [], [], []
        first_dup, n = {}, 0
        kj_ref, vj_ref = poison(n_join, Hkv * D), poison(n_join, Hkv * D)
        j_dst, j_src = [], []                                     # join row <- row of the duplicated list
        for t, d in enumerate(dests):
            first_dup[t] = n
            for m, s in d:
                d_sample.append(m), d_slot.append(s), d_row.append(perm[n])
                j_dst.append(perm[n]), j_src.append(n)
                n += 1
            if t < P:                                             # join row only: no cache image is touched
                r = perm[n_dup + t]
                d_sample.append(-1), d_slot.append(t), d_row.append(r)
                j_dst.append(r), j_src.append(first_dup[t])
            if t % 5 == 0:                                        # out of range on every side: nothing is written
                for bad in ((B, 3, -1), (0, S, n_join), (1, -1, -7), (-2, 0, n_join + 5)):
                    d_sample.append(bad[0]), d_slot.append(bad[1]), d_row.append(bad[2])
            off.append(len(d_sample))
        j_dst, j_src = torch.tensor(j_dst, device="cuda"), torch.tensor(j_src, device="cuda")
        kj_ref[j_dst] = kp[j_src]                                 # against k_pack and the V slice of the duplicated rows
        vj_ref[j_dst] = qkv_dup[j_src, (Hq + Hkv) * D:]
        q = poison(T, Hq * D)
        kj, vj = poison(n_join, Hkv * D), poison(n_join, Hkv * D)
        kc, vt = poison(B, Hkv, S, D), poison(B, Hkv, D, S)
        ops.llm_qkv_post_shared(qkv, pos, inv, q, kc, vt, kj, vj, i32(off), i32(d_sample), i32(d_slot), i32(d_row), Hq, Hkv, D, S, sec,
                                cache_packed=bool(cache_packed))
        torch.cuda.synchronize()
        v16 = lambda t: t.view(torch.int16)
        what = f"P={P} fan-out={fan}"
        assert torch.equal(v16(q), v16(q_ref[torch.tensor([first_dup[t] for t in range(T)], device="cuda")])), what
        assert torch.equal(v16(kc), v16(kc_ref)), what            # whole buffers, poison included: nothing else was written
        assert torch.equal(v16(vt), v16(vt_ref)), what
        assert torch.equal(v16(kj), v16(kj_ref)), what
        assert torch.equal(v16(vj), v16(vj_ref)), what
        assert (v16(kj[perm[n_join - 1]]) == 0x7B3D).all() and (v16(kj[perm[n_join - 2]]) == 0x7B3D).all()


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
    return cfg, w, model, U, U.oracle_config(cfg), shared_case(cfg)


def tol(model, bf16, fp16):
    """The bound for the model's MFMA operand type (test_e2e_gpu.py)."""
    return fp16 if model.dtype == torch.float16 else bf16


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item(), ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()


def sched_rec(U):
    return U.rec_schedule(T_NEW, vrt_at=range(4, 8))


def shared_kw(c):
    return dict(input_ids=c["ids"].cuda(), attention_mask=c["am"].cuda(), pixel_values=c["pix"].cuda(), image_grid_thw=c["grid"],
                image_index=c["image_index"])


def expanded_kw(c):
    return dict(input_ids=c["ids"].cuda(), attention_mask=c["am"].cuda(), pixel_values=c["pix_x"].cuda(), image_grid_thw=c["grid_x"])


def cache_rows(sess, lens):
    """Row-major (K [layer][b][Hkv][len][D], V^T [layer][b][Hkv][D][len]) copies of the session's cache images below each row's length."""
    from padt_amd import ops
    ks, vs = [], []
    for kc, vt in zip(sess.kc, sess.vtc):
        k = ops.unpack_k_cache(kc) if sess.cache_packed else kc
        v = ops.unpack_vt_cache(vt) if sess.cache_packed else vt
        ks.append([k[b, :, :l].clone() for b, l in enumerate(lens)])
        vs.append([v[b, :, :, :l].clone() for b, l in enumerate(lens)])
    return ks, vs


@pytest.fixture(scope="module")
def runs(setup):
    """The shared call and the expanded call on the same model, once per operand type (cache images copied: the two calls use one session)."""
    cfg, w, model, U, oc, c = setup
    gen = dict(max_new_tokens=T_NEW, schedule=sched_rec(U), do_sample=False, output_hidden_states=True, return_dict_in_generate=True)
    lens = [int(x) for x in c["am"].sum(1)]
    plain = model.generate(**gen, **expanded_kw(c))
    plain_cache = cache_rows(plain.past_key_values, [l + T_NEW - 1 for l in lens])
    plain_rope = model.rope_deltas.clone()
    shared = model.generate(**gen, **shared_kw(c))
    shared_cache = cache_rows(shared.past_key_values, [l + T_NEW - 1 for l in lens])
    return dict(plain=plain, plain_cache=plain_cache, plain_rope=plain_rope, shared=shared, shared_cache=shared_cache,
                shared_rope=model.rope_deltas.clone(), lens=lens)


def test_shared_generate_against_the_oracle_on_expanded_inputs(setup, runs):
    """What test_e2e_gpu.py::test_generate_tokens_hidden_and_vl_decode asserts, with its tol(...) numbers, for the shared call against the
    oracle teacher-forced on the EXPANDED inputs: sharing is the same arithmetic on fewer rows, so no bound is wider here."""
    cfg, w, model, U, oc, c = setup
    import padt_amd
    O = U.O
    B, T = 7, T_NEW
    ids, am, grid_x = c["ids"], c["am"], c["grid_x"]
    sched = sched_rec(U)
    out = runs["shared"]
    seq = out.sequences.cpu()
    L = ids.shape[1]
    toks = seq[:, L:]
    assert toks.shape[1] == T and (toks[:, -1] == cfg.eos_token_id).all()
    V = cfg.vocab_size
    n_m = [c["n_merged"][u] for u in c["image_index"]]
    off = [sum(n_m[:b]) for b in range(B)]
    for b in range(B):                                              # VRT ids global, per-sample ranges in sample order
        for t in range(T - 1):
            if sched[t] == "v":
                assert V + off[b] <= toks[b, t] < V + off[b] + n_m[b], (b, t, int(toks[b, t]))
            else:
                assert toks[b, t] < V
    ores = O.generate(w, oc, ids, am, c["pix_x"], grid_x, T, schedule=sched, collect_logits=True, force_tokens=toks)
    assert torch.equal(ores["sequences"], seq)
    noise, n_tie = 0.0, 0
    for t in range(T):
        lg = ores["logits"][t]
        top2 = lg.topk(2, dim=-1).values
        chosen = lg.gather(1, toks[:, t:t + 1]).squeeze(1)
        floor = tol(model, 2e-2, 4e-3) * lg[torch.isfinite(lg)].abs().max().item()
        for b in range(B):
            margin = (top2[b, 0] - (top2[b, 1] if torch.isfinite(top2[b, 1]) else top2[b, 0] - 1)).item()
            if margin > floor:
                assert chosen[b] == top2[b, 0], f"step {t} sample {b}: HIP token is not the oracle argmax (margin {margin:.3e})"
            else:
                n_tie += 1
                assert (top2[b, 0] - chosen[b]).item() <= floor
            noise = max(noise, (top2[b, 0] - chosen[b]).item())
    assert n_tie <= T * B // 4, "too many near-ties: test has no power"      # a quarter of the (step, sample) pairs, as there
    hid = out.hidden_states.last_layer_rows().cpu().float()
    for t in range(T):
        mx, rms = rel_err(hid[t], ores["hidden"][t][:, -1].float())
        assert rms < tol(model, 2e-2, 3e-3) and mx < tol(model, 8e-2, 1.2e-2), f"hidden step {t}: rel err max {mx:.3e} rms {rms:.3e}"
    # step 0 of hidden_states: (B, L_pad, D), left-padded — every prompt row against the oracle's
    h0 = out.hidden_states[0][-1]
    assert h0.shape == (B, L, cfg.hidden_size)
    for b in range(B):
        l = runs["lens"][b]
        assert not h0[b, : L - l].any()
        mx, rms = rel_err(h0[b, L - l:], ores["hidden"][0][b, L - l:].float())
        assert rms < tol(model, 2e-2, 3e-3) and mx < tol(model, 8e-2, 1.2e-2), f"prompt rows of sample {b}: rel err max {mx:.3e} rms {rms:.3e}"
    assert torch.equal(runs["shared_rope"].long().cpu(), ores["state"].rope_deltas.long().reshape(B, 1))
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, max(n_m)), 2)
    proc.model_embed_token_size = V
    local = proc.assign_to_local_vrt_id(seq.clone(), grid_x)[:, L:]
    comps, feats, labels, vrts, _ = padt_amd.parseVRTintoCompletion(proc, local, out["hidden_states"], torch.Tensor([False] * B))
    assert [len(f) for f in feats] == [1] * B and all(f[0].shape == (4, cfg.hidden_size) for f in feats)
    for b in range(B):
        assert torch.equal(feats[b][0].cpu().float(), hid[4:8, b])
        assert vrts[b][0] == "".join("<|VRT_%d|>" % int(i - V) for i in local[b, 4:8])
    dec = model.vl_decode(feats, out.past_image_embeds, out.past_high_res_image_embeds, grid_x, out.past_visual_pe)
    st = ores["state"]
    ofeats = [[torch.cat([ores["hidden"][t][b:b + 1, -1] for t in range(4, 8)], 0)] for b in range(B)]
    odec = O.vl_decode(w, oc, ofeats, st.proto, st.high_res, grid_x, st.visual_pe)
    assert dec["sample_idx"] == odec["sample_idx"] == list(range(B))
    assert torch.equal(dec["pred_mask_valid_hw"][0].cpu(), odec["pred_mask_valid_hw"][0])
    assert torch.equal(dec["pred_mask_valid_hw"][1].cpu(), odec["pred_mask_valid_hw"][1])
    assert dec["pred_mask"].shape == odec["pred_mask"].shape
    db = (dec["pred_boxes"].cpu().float() - odec["pred_boxes"]).abs().max().item()
    ds = (dec["pred_score"].cpu().float() - odec["pred_score"]).abs().max().item()
    mx, rms = rel_err(dec["pred_mask"], odec["pred_mask"])
    print(f"\n[shared e2e parity, {model.dtype}] box |d|max {db:.3e}  score |d|max {ds:.3e}  mask rel max {mx:.3e} rms {rms:.3e}  token noise {noise:.3e}")
    assert db < tol(model, 3e-4, 3e-5), f"box coords differ by {db:.3e}"
    assert ds < tol(model, 5e-3, 8e-4) * (odec["pred_score"].abs().max().item() + 1), f"score logit differs by {ds:.3e}"
    assert rms < tol(model, 1.2e-2, 1.5e-3) and mx < tol(model, 9e-3, 1.1e-3), f"mask logits rel err max {mx:.3e} rms {rms:.3e}"


def test_shared_generate_equals_the_expanded_call(setup, runs):
    """Against the expanded call on the same model.  The ViT blocks, the merger, the prototype projection and every row copy are held to
    bit equality: past_image_embeds, past_high_res_image_embeds, past_visual_pe, past_logit_mask, rope_deltas.

    The prompt pass is NOT bit-identical in general, and this is a property of the tile GEMM, not of sharing: gemm_tile_kernel (gemm.hip)
    computes `acc * row_scale + bias` as one fused multiply-add in a complete 128-row tile and as a rounded product plus the bias in a tile cut
    by M, so the fp32 value of a qkv element before its 16-bit rounding can differ by an ulp with the position of its row in the launch — and
    the shared pass puts a row elsewhere.  Measured on an MI355X with this case (profiles/shared_prefix.md §3): fp16 operands — sequences,
    prompt rows, per-step rows and the K images equal, ONE element of the layer-0 V^T image of sample 6 differs by 2^-23 = 1.2e-7 (one fp16
    ulp of a value in [2^-13, 2^-12)); bf16 operands — everything equal.  The figures are printed below on every run.  Downstream of that GEMM the test asserts
    what the one rounding can do (see the two comments at the end), and the oracle test above holds the tokens and hidden rows to fp32."""
    cfg, w, model, U, oc, c = setup
    a, b = runs["shared"], runs["plain"]
    L = c["ids"].shape[1]
    diffs = {}

    def d(name, x, y):
        assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape, x.dtype, y.dtype)
        diffs[name] = (x.float() - y.float()).abs().max().item() if x.numel() else 0.0
        return torch.equal(x, y)
    # upstream of the prompt pass: bit equality
    assert d("past_image_embeds", a.past_image_embeds, b.past_image_embeds)
    assert d("past_high_res_image_embeds", a.past_high_res_image_embeds, b.past_high_res_image_embeds)
    assert d("past_visual_pe.cos", a.past_visual_pe[0], b.past_visual_pe[0]) and d("past_visual_pe.sin", a.past_visual_pe[1], b.past_visual_pe[1])
    assert d("past_logit_mask", a.past_logit_mask.float(), b.past_logit_mask.float())
    assert torch.equal(runs["shared_rope"], runs["plain_rope"])
    n_x = sum(c["n_merged"][u] for u in c["image_index"])
    assert a.past_image_embeds.shape[0] == n_x and a.past_high_res_image_embeds.shape[0] == c["pix_x"].shape[0] == a.past_visual_pe[0].shape[0]
    assert a.sequences.shape == b.sequences.shape == (7, L + T_NEW)
    assert a.hidden_states[0][-1].shape == b.hidden_states[0][-1].shape == (7, L, cfg.hidden_size)
    # downstream of the prompt pass's first tile GEMM: measured and printed first, then bounded by what that one rounding can do
    d("sequences", a.sequences, b.sequences)
    d("hidden_states[0][-1]", a.hidden_states[0][-1], b.hidden_states[0][-1])
    d("last_layer_rows", a.hidden_states.last_layer_rows(), b.hidden_states.last_layer_rows())
    (ka, va), (kb, vb) = runs["shared_cache"], runs["plain_cache"]
    for name, xa, xb in (("K", ka, kb), ("V^T", va, vb)):
        for i, (la, lb) in enumerate(zip(xa, xb)):
            for r, (x, y) in enumerate(zip(la, lb)):
                d(f"{name} cache layer {i} row {r}", x, y)
    caches = {k: v for k, v in diffs.items() if "cache" in k}
    print(f"\n[shared vs expanded, {model.dtype}] max |difference| per quantity: "
          + ", ".join(f"{k} {v:.3e}" for k, v in diffs.items() if "cache" not in k)
          + f"; cache images (below each row's length): max {max(caches.values()):.3e}, non-zero: { {k: v for k, v in caches.items() if v != 0.0} }")
    # (1) Layer 0's V rows are the qkv GEMM's output itself.  Its input rows are bit-equal on both sides (the embedding rows are copies of
    # equal tables), so the fp32 accumulators are equal and only the epilogue differs: fma(acc, rs, b) against round(acc * rs) + b, at most
    # one fp32 ulp apart, i.e. at most ONE ulp of the 16-bit type after the store — for every element, prompt rows and decode rows alike.
    mant, tiny = (10, 2.0 ** -24) if model.dtype == torch.float16 else (7, 2.0 ** -133)
    for r, (x, y) in enumerate(zip(va[0], vb[0])):
        x, y = x.float(), y.float()
        ulp = torch.exp2((torch.frexp(torch.maximum(x.abs(), y.abs()))[1] - 1 - mant).float()).clamp_min(tiny)
        assert bool(((x - y).abs() <= ulp).all()), f"layer-0 V^T image of row {r}: more than one 16-bit ulp from the expanded call"
    # (2) Everything behind it (K after the rotation, deeper layers, hidden rows) sees such one-ulp inputs through the network, for which
    # no per-element bound exists.  Both calls are the same arithmetic on the same numbers up to that rounding, so they may not be further
    # apart than either may be from the fp32 oracle: the hidden-row bounds of the oracle test (test_e2e_gpu.py's tol numbers), per image.
    # A wrong fan-out destination, key segment or position puts a different token's row there: a relative difference of order one.
    lim_rms, lim_mx = tol(model, 2e-2, 3e-3), tol(model, 8e-2, 1.2e-2)
    pairs = [("hidden_states[0][-1]", a.hidden_states[0][-1], b.hidden_states[0][-1]),
             ("last_layer_rows", a.hidden_states.last_layer_rows(), b.hidden_states.last_layer_rows())]
    for name, xa, xb in (("K", ka, kb), ("V^T", va, vb)):
        for i, (la, lb) in enumerate(zip(xa, xb)):
            pairs += [(f"{name} cache layer {i} row {r}", x, y) for r, (x, y) in enumerate(zip(la, lb))]
    for name, x, y in pairs:
        mx, rms = rel_err(x, y)
        assert rms < lim_rms and mx < lim_mx, f"{name}: shared vs expanded rel err max {mx:.3e} rms {rms:.3e}"


def test_merged_runner_with_image_index_equals_single_calls(setup):
    """PipelinedRunner(merge=2) with image_index on both batches: one decode session, each batch's prompt pass shared on its own rows —
    results equal two plain rec_batch(image_index=) calls."""
    cfg, w, model, U, oc, c = setup
    import padt_amd
    from padt_amd import pipeline
    sched = sched_rec(U)
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 40), 2)
    proc.model_embed_token_size = cfg.vocab_size
    batches = [c, shared_case(cfg, seed=78)]
    args = lambda x: (x["ids"].cuda().clone(), x["am"].cuda(), x["pix"].cuda(), x["grid"])
    alone = [pipeline.rec_batch(model, proc, *args(x), max_new_tokens=T_NEW, schedule=sched, image_index=x["image_index"]) for x in batches]
    assert alone[0][3] != alone[1][3]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for x in batches:
        got += runner.submit(*args(x), max_new_tokens=T_NEW, schedule=sched, image_index=x["image_index"])
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2
    for (d0, c0, l0, v0), (d1, c1, l1, v1) in zip(alone, got):
        assert c0 == c1 and v0 == v1 and len(c0) == 7
        assert torch.equal(d0["pred_boxes"], d1["pred_boxes"]) and torch.equal(d0["pred_mask"], d1["pred_mask"])
        assert torch.equal(d0["pred_score"], d1["pred_score"])
    # ... and the expanded batch through rec_batch gives the same completions
    x = batches[0]
    plain = pipeline.rec_batch(model, proc, x["ids"].cuda().clone(), x["am"].cuda(), x["pix_x"].cuda(), x["grid_x"], max_new_tokens=T_NEW,
                               schedule=sched)
    assert plain[1] == alone[0][1] and plain[3] == alone[0][3]


def test_short_shared_prompt_after_a_long_plain_one(setup, runs):
    """A session first used by a LONGER plain prompt, then by the shared one: no stale key beyond `lens` is visible — the result is the
    fresh session's (both sessions hold 128 slots: the decode attention's split is the same)."""
    cfg, w, model, U, oc, c = setup
    gen = dict(max_new_tokens=T_NEW, schedule=sched_rec(U), do_sample=False)
    grid, pix, ids, am = U.synthetic_batch(cfg, c["grid_x"].tolist(), n_pre=15, n_post=60, ragged=True, seed=5)
    assert max(runs["lens"]) < int(am.sum(1).min()) and int(am.sum(1).max()) + T_NEW <= 128
    model.generate(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, lane=12, **gen)
    used = model.generate(lane=12, **gen, **shared_kw(c))
    fresh = model.generate(lane=11, **gen, **shared_kw(c))
    assert model.lm._sessions[(7, 12)].s_max == model.lm._sessions[(7, 11)].s_max == 128
    assert torch.equal(used.sequences, fresh.sequences)
    assert torch.equal(used.hidden_states.last_layer_rows(), fresh.hidden_states.last_layer_rows())
    assert torch.equal(used.hidden_states[0][-1], fresh.hidden_states[0][-1])
    assert torch.equal(used.sequences, runs["shared"].sequences)


def test_hooked_loop_bans_and_penalty_with_image_index(setup, runs):
    """The device-side bans, the repetition penalty and the hooked loop read input_ids and the score rows, not the prompt pass: with
    image_index the captured steps and the hooked loop (an identity processor) return the same tokens and score rows, and the rules bite."""
    cfg, w, model, U, oc, c = setup
    L = c["ids"].shape[1]
    free = runs["shared"].sequences[:, L:].cpu()
    ban = sorted(set(free[:, :3].flatten().tolist()) - {cfg.eos_token_id, cfg.pad_token_id})      # what the free run said first
    gen = dict(max_new_tokens=T_NEW, schedule=sched_rec(U), do_sample=False, repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=ban,
               output_scores=True)
    a = model.generate(**gen, **shared_kw(c))
    b = model.generate(**gen, logits_processor=[lambda input_ids, scores: scores], **shared_kw(c))
    assert torch.equal(a.sequences, b.sequences) and not torch.equal(a.sequences[:, L:].cpu(), free)
    assert not torch.isin(a.sequences[:, L:].cpu(), torch.tensor(ban)).any()
    assert len(a.scores) == len(b.scores) == T_NEW and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))


# ------------------------------------------------------------------------------------------------------------ quantised weights
@pytest.mark.parametrize("llm_weights", ["fp8", "fp8+act", "fp4"])
def test_quantised_llm_weights_shared_against_expanded(llm_weights):
    """The margin rule of the oracle test with the EXPANDED call's score rows as the reference: every token of the shared call is the
    expanded call's arg-max unless that call's own top-2 margin is below the operand noise floor (then within the floor)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    cfg = dataclasses.replace(cfg, tie_word_embeddings=False, num_attention_heads=4, num_key_value_heads=2, hidden_size=512)
    cfg = dataclasses.replace(cfg, vision_config=dataclasses.replace(cfg.vision_config, out_hidden_size=512))
    model = PaDTForConditionalGeneration(cfg, U.bf16_weights(cfg, seed=19, std=0.05), device="cuda", llm_weights=llm_weights)
    assert model.W.llm_weights == llm_weights.split("+")[0] and bool(model.W.fp8_prefill) == (llm_weights == "fp8+act")
    c = shared_case(cfg)
    L = c["ids"].shape[1]
    gen = dict(max_new_tokens=T_NEW, schedule=sched_rec(U), do_sample=False, output_scores=True)
    plain = model.generate(**gen, **expanded_kw(c))
    shared = model.generate(**gen, **shared_kw(c))
    toks = shared.sequences[:, L:].cpu()
    print(f"\n[{llm_weights}] shared == expanded: sequences {torch.equal(shared.sequences, plain.sequences)}, step rows "
          f"{torch.equal(shared.hidden_states.last_layer_rows(), plain.hidden_states.last_layer_rows())}")
    for t in range(T_NEW):
        lg = plain.scores[t].cpu()
        top2 = lg.topk(2, dim=-1).values
        chosen = lg.gather(1, toks[:, t:t + 1]).squeeze(1)
        floor = tol(model, 2e-2, 4e-3) * lg[torch.isfinite(lg)].abs().max().item()
        for b in range(7):
            margin = (top2[b, 0] - (top2[b, 1] if torch.isfinite(top2[b, 1]) else top2[b, 0] - 1)).item()
            if margin > floor:
                assert chosen[b] == top2[b, 0], f"step {t} sample {b}: shared token is not the expanded call's argmax (margin {margin:.3e})"
            else:
                assert (top2[b, 0] - chosen[b]).item() <= floor
    assert torch.equal(shared.past_image_embeds, plain.past_image_embeds)


# ------------------------------------------------------------------------------------------------------------ range guard
def test_bf16_rerun_of_a_flagged_batch_keeps_the_image_index():
    """operands="auto": a batch whose SwiGLU hidden exceeds fp16's range is re-run on the bf16 twin WITH its image_index — the result is
    the bf16 model's own shared run (the weight edit is test_range_guard_gpu.py's `llm_swiglu` case)."""
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
    c = shared_case(cfg)
    gen = dict(max_new_tokens=T_NEW, schedule=sched_rec(U))
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16")
    want = ref.generate(**gen, **shared_kw(c))
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(**gen, **shared_kw(c))
    assert auto.overflow_reruns == 1 and torch.equal(got.sequences, want.sequences)
    assert torch.equal(got.hidden_states.last_layer_rows(), want.hidden_states.last_layer_rows())
    assert torch.equal(got.hidden_states[0][-1], want.hidden_states[0][-1])
    assert got.past_image_embeds.shape[0] == sum(c["n_merged"][u] for u in c["image_index"])
