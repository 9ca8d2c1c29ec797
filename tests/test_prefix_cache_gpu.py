"""encode_prefix / generate(prefix=): an image's ViT output and the K / V rows of its prompt prefix kept across generate calls.

Kernel level: padt_kv_prefix_fanout is data movement — cached join rows land where padt_llm_qkv_post_shared would have fanned the same tokens out
(bit equality of whole poisoned buffers).  Build half: the handle holds, bit for bit, what a plain generate on the prefix rows leaves in its
session and outputs.  Consume half (the small synthetic model, prefix_cache_util.prefix_case: 6 queries over 3 cached prefixes): against the
fp32 oracle on the expanded inputs and against generate(image_index=) on the same model, with test_shared_prefix_gpu.py's bounds."""
import pytest
import torch

from prefix_cache_util import prefix_case
from test_shared_prefix_gpu import T_NEW, cache_rows, rel_err, sched_rec, tol

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------ the fan-out kernel
PREFIX_PAIRS = ((1, 50), (15, 33), (16, 32), (17, 31))            # two images per launch; the edges of the 16- and 32-slot fragments
# (head_dim, handle rows misaligned): the 16-byte path; its scalar twin on a 2-byte aligned base; a head_dim % 16 != 0 (row-major caches only:
# the packed forms need head_dim % 32 == 0)
SHAPES = [(128, False, 0), (128, False, 1), (128, True, 0), (128, True, 1), (72, False, 0)]


@pytest.mark.parametrize("head_dim,misaligned,cache_packed", SHAPES, ids=lambda v: str(int(v)))
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
def test_kv_prefix_fanout_is_the_shared_post_pass_minus_the_arithmetic(dt, head_dim, misaligned, cache_packed):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops
    Hq, Hkv, D = 4, 2, head_dim
    sec = (16, 24, 24) if D == 128 else (8, 14, 14)
    inv = (1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))).cuda()
    g = torch.Generator().manual_seed(4321 + D + cache_packed)
    poison = lambda *shape: torch.full(shape, 0x7B3D, dtype=torch.int16, device="cuda").view(dt)
    v16 = lambda t: t.view(torch.int16)
    case = 0
    for S in (64, 128):
        for P in PREFIX_PAIRS:
            # even cases: a session of 5 rows, image 0's member is row 0, image 1's are rows 1 and 3 — rows 2 and 4 keep their poison;
            # odd cases: the same batch at row0 = 2 of a session of 7 rows
            row0, n_rows = (0, 5) if case % 2 == 0 else (2, 7)
            case += 1
            members = [(0, row0 + 0), (1, row0 + 1), (1, row0 + 3)]              # (image, session row)
            n_own = 3
            assert max(P) + n_own <= S
            seg, n_join = [], 2
            for u, _ in members:                                  # key segments [prefix | own] with gaps nobody writes
                seg.append(n_join)
                n_join += P[u] + n_own + 3
            side = n_join                                         # a member whose session row is out of range: its join rows only
            n_join += P[1] + 1
            pre_off = [0, P[0], P[0] + P[1]]
            # token list of the reference: the two prefixes, then every member's own tokens
            dests = [[(r, j, seg[m] + j) for m, (u, r) in enumerate(members) if u == img] + ([(n_rows, j, side + j)] if img == 1 else [])
                     for img in (0, 1) for j in range(P[img])]
            n_pre = len(dests)
            dests += [[(r, P[u] + j, seg[m] + P[u] + j)] for m, (u, r) in enumerate(members) for j in range(n_own)]
            T = len(dests)
            qkv = (torch.randn(T, (Hq + 2 * Hkv) * D, generator=g) * 2).to(dt).cuda()
            pos = torch.randint(0, 600, (3, T), generator=g, dtype=torch.int32).cuda()

            def post(rows, dst, q, kc, vt, kj, vj):
                off = [0]
                for d in dst:
                    off.append(off[-1] + len(d))
                flat = [e for d in dst for e in d]
                ops.llm_qkv_post_shared(qkv[rows].contiguous(), pos[:, rows].contiguous(), inv, q, kc, vt, kj, vj, i32(off),
                                        i32([e[0] for e in flat]), i32([e[1] for e in flat]), i32([e[2] for e in flat]), Hq, Hkv, D, S, sec,
                                        cache_packed=bool(cache_packed))
            # ---- reference: ONE post-pass over prefix + own tokens
            q_ref, kj_ref, vj_ref = poison(T, Hq * D), poison(n_join, Hkv * D), poison(n_join, Hkv * D)
            kc_ref, vt_ref = poison(n_rows, Hkv, S, D), poison(n_rows, Hkv, D, S)
            post(slice(0, T), dests, q_ref, kc_ref, vt_ref, kj_ref, vj_ref)
            # ---- under test: the prefix tokens into handle-shaped rows (join-only destinations) ...
            k_pre, v_pre = poison(n_pre, Hkv * D), poison(n_pre, Hkv * D)
            scratch_c, scratch_v = poison(1, Hkv, S, D), poison(1, Hkv, D, S)
            post(slice(0, n_pre), [[(-1, 0, t)] for t in range(n_pre)], poison(n_pre, Hq * D), scratch_c, scratch_v, k_pre, v_pre)
            assert (v16(scratch_c) == 0x7B3D).all() and (v16(scratch_v) == 0x7B3D).all()
            if misaligned:                                        # the same rows on a base that is 2-byte aligned only
                shift = lambda t: torch.cat([poison(1), t.reshape(-1)])[1:].view(t.shape)
                k_pre, v_pre = shift(k_pre), shift(v_pre)
                assert k_pre.data_ptr() % 16 == 2
            # ... fresh poisoned buffers, the fan-out of the cached rows, the post-pass over the own tokens
            q, kj, vj = poison(T - n_pre, Hq * D), poison(n_join, Hkv * D), poison(n_join, Hkv * D)
            kc, vt = poison(n_rows, Hkv, S, D), poison(n_rows, Hkv, D, S)
            # members out of range: the session row (its join rows are written, as the reference's destinations say); the session row AND
            # the join rows (the segment would end past n_join): skipped; the image, on either side: skipped
            mem = members + [(1, n_rows), (1, n_rows + 3), (2, row0 + 4), (-1, row0 + 4)]
            join = seg + [side, n_join - 1, 0, 0]
            ops.kv_prefix_fanout(k_pre, v_pre, i32(pre_off), i32([m[0] for m in mem]), i32([m[1] for m in mem]), i32(join), max(P), kc, vt, kj, vj,
                                 Hkv, D, S, cache_packed=bool(cache_packed))
            post(slice(n_pre, T), dests[n_pre:], q, kc, vt, kj, vj)
            torch.cuda.synchronize()
            what = f"P={P} s_max={S} row0={row0}"
            assert torch.equal(v16(q), v16(q_ref[n_pre:])), what
            assert torch.equal(v16(kc), v16(kc_ref)), what        # whole buffers, poison included: nothing else was written
            assert torch.equal(v16(vt), v16(vt_ref)), what
            assert torch.equal(v16(kj), v16(kj_ref)), what
            assert torch.equal(v16(vj), v16(vj_ref)), what
            for r in sorted(set(range(n_rows)) - {r for _, r in members}):
                assert (v16(kc[r]) == 0x7B3D).all() and (v16(vt[r]) == 0x7B3D).all(), what


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
    return cfg, w, model, U, U.oracle_config(cfg), prefix_case(cfg)


def prefix_inputs(c):
    return c["pre_ids"].cuda(), c["pre_am"].cuda(), c["pix"].cuda(), c["grid"]


def prefix_kw(c, handle):
    return dict(input_ids=c["q_ids"].cuda(), attention_mask=c["q_am"].cuda(), prefix=handle, image_index=c["q_index"])


def index_kw(c):
    return dict(input_ids=c["q_ids"].cuda(), attention_mask=c["q_am"].cuda(), pixel_values=c["pix"].cuda(), image_grid_thw=c["grid"],
                image_index=c["q_index"])


def handle_tensors(h):
    return dict(low=h.low, high=h.high, cos=h.pe[0], sin=h.pe[1], proto=h.proto, hidden=h.hidden, k=h.k, v=h.v, pre_off=h.pre_off)


class no_vit:
    """model.visual replaced by a function that raises, for the duration of a block."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.kept = self.model.visual

        def visual(*a, **kw):
            raise AssertionError("the ViT ran in a generate(prefix=) call")
        self.model.visual = visual

    def __exit__(self, *exc):
        self.model.visual = self.kept


@pytest.fixture(scope="module")
def runs(setup):
    """The handle, and the prefix call and the image_index call on the same model, once per operand type (cache images copied: the calls use one
    session).  Nothing here is modified by a test."""
    cfg, w, model, U, oc, c = setup
    gen = dict(max_new_tokens=T_NEW, schedule=sched_rec(U), do_sample=False, output_hidden_states=True, return_dict_in_generate=True)
    handle = model.encode_prefix(*prefix_inputs(c))
    kept = {k: v.clone() for k, v in handle_tensors(handle).items()}
    lens = [int(x) for x in c["q_am"].sum(1)]
    shared = model.generate(**gen, **index_kw(c))
    shared_cache = cache_rows(shared.past_key_values, [l + T_NEW - 1 for l in lens])
    shared_rope = model.rope_deltas.clone()
    with no_vit(model):
        pref = model.generate(**gen, **prefix_kw(c, handle))
    pref_cache = cache_rows(pref.past_key_values, [l + T_NEW - 1 for l in lens])
    return dict(handle=handle, kept=kept, shared=shared, shared_cache=shared_cache, shared_rope=shared_rope, pref=pref, pref_cache=pref_cache,
                pref_rope=model.rope_deltas.clone(), lens=lens, gen=gen)


def test_the_handle_holds_what_a_plain_generate_on_the_prefix_rows_leaves(setup, runs):
    """Build half.  encode_prefix and generate(max_new_tokens=1) on the three prefix rows perform the same launches at the same row counts and
    differ in the post-pass's sink only: bit equality."""
    cfg, w, model, U, oc, c = setup
    h = runs["handle"]
    ids, am, pix, grid = prefix_inputs(c)
    plain = model.generate(input_ids=ids, attention_mask=am, pixel_values=pix, image_grid_thw=grid, max_new_tokens=1, do_sample=False)
    P, off = c["P"], [0, c["P"][0], c["P"][0] + c["P"][1], sum(c["P"])]
    ks, vs = cache_rows(plain.past_key_values, P)
    Hkv, hd = cfg.num_key_value_heads, cfg.head_dim
    assert h.dtype == model.dtype and h.k.dtype == h.v.dtype == h.hidden.dtype == model.dtype and h.n_images == 3 and h.lens == P
    assert h.k.shape == h.v.shape == (cfg.num_hidden_layers, sum(P), Hkv * hd)
    assert h.nbytes == sum(t.numel() * t.element_size() for k, t in handle_tensors(h).items() if k != "pre_off")
    assert h.nbytes >= 2 * cfg.num_hidden_layers * sum(P) * Hkv * hd * 2
    for i in range(cfg.num_hidden_layers):
        for u in range(3):
            k = h.image_k(u)[i].view(P[u], Hkv, hd)
            v = h.image_v(u)[i].view(P[u], Hkv, hd)
            assert torch.equal(k.permute(1, 0, 2), ks[i][u]), f"K rows of layer {i}, image {u}"
            assert torch.equal(v.permute(1, 2, 0), vs[i][u]), f"V rows of layer {i}, image {u}"
    assert torch.equal(h.proto, plain.past_image_embeds)
    assert torch.equal(h.high, plain.past_high_res_image_embeds)
    assert torch.equal(h.pe[0], plain.past_visual_pe[0]) and torch.equal(h.pe[1], plain.past_visual_pe[1])
    assert torch.equal(h.low, model.visual(pix, grid)[0])         # the merged rows: the call generate makes (they are no output of it)
    h0 = plain.hidden_states[0][-1]
    L = ids.shape[1]
    for u in range(3):
        assert torch.equal(h.hidden[off[u]: off[u + 1]], h0[u, L - P[u]:]), f"prefix hidden rows of image {u}"
    assert h.pre_off.tolist() == off and h.next_pos == [int(p.max()) + 1 for p in h.pos3]
    assert [p.shape for p in h.pos3] == [(3, n) for n in P]
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(h.inputs, (ids, am, pix, grid)))


def test_prefix_generate_against_the_oracle_on_expanded_inputs(setup, runs):
    """What test_shared_generate_against_the_oracle_on_expanded_inputs asserts, with its tol(...) numbers, for the prefix call against the
    oracle teacher-forced on the EXPANDED inputs."""
    cfg, w, model, U, oc, c = setup
    import padt_amd
    O = U.O
    B, T = 6, T_NEW
    ids, am, grid_x = c["q_ids"], c["q_am"], c["q_grid_x"]
    sched = sched_rec(U)
    out = runs["pref"]
    seq = out.sequences.cpu()
    L = ids.shape[1]
    toks = seq[:, L:]
    assert toks.shape[1] == T and (toks[:, -1] == cfg.eos_token_id).all()
    V = cfg.vocab_size
    n_m = [c["n_merged"][u] for u in c["q_index"]]
    off = [sum(n_m[:b]) for b in range(B)]
    for b in range(B):
        for t in range(T - 1):
            if sched[t] == "v":
                assert V + off[b] <= toks[b, t] < V + off[b] + n_m[b], (b, t, int(toks[b, t]))
            else:
                assert toks[b, t] < V
    ores = O.generate(w, oc, ids, am, c["q_pix_x"], grid_x, T, schedule=sched, collect_logits=True, force_tokens=toks)
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
    assert n_tie <= T * B // 4, "too many near-ties: test has no power"
    hid = out.hidden_states.last_layer_rows().cpu().float()
    for t in range(T):
        mx, rms = rel_err(hid[t], ores["hidden"][t][:, -1].float())
        assert rms < tol(model, 2e-2, 3e-3) and mx < tol(model, 8e-2, 1.2e-2), f"hidden step {t}: rel err max {mx:.3e} rms {rms:.3e}"
    h0 = out.hidden_states[0][-1]                                 # complete: the handle's prefix rows + the computed own rows
    assert h0.shape == (B, L, cfg.hidden_size)
    for b in range(B):
        l = runs["lens"][b]
        assert not h0[b, : L - l].any()
        mx, rms = rel_err(h0[b, L - l:], ores["hidden"][0][b, L - l:].float())
        assert rms < tol(model, 2e-2, 3e-3) and mx < tol(model, 8e-2, 1.2e-2), f"prompt rows of sample {b}: rel err max {mx:.3e} rms {rms:.3e}"
    assert torch.equal(runs["pref_rope"].long().cpu(), ores["state"].rope_deltas.long().reshape(B, 1))
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, max(n_m)), 2)
    proc.model_embed_token_size = V
    local = proc.assign_to_local_vrt_id(seq.clone(), grid_x)[:, L:]
    comps, feats, labels, vrts, _ = padt_amd.parseVRTintoCompletion(proc, local, out["hidden_states"], torch.Tensor([False] * B))
    assert [len(f) for f in feats] == [1] * B and all(f[0].shape == (4, cfg.hidden_size) for f in feats)
    for b in range(B):
        assert torch.equal(feats[b][0].cpu().float(), hid[4:8, b])
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
    print(f"\n[prefix e2e parity, {model.dtype}] box |d|max {db:.3e}  score |d|max {ds:.3e}  mask rel max {mx:.3e} rms {rms:.3e}  token noise {noise:.3e}  near-ties {n_tie}")
    assert db < tol(model, 3e-4, 3e-5), f"box coords differ by {db:.3e}"
    assert ds < tol(model, 5e-3, 8e-4) * (odec["pred_score"].abs().max().item() + 1), f"score logit differs by {ds:.3e}"
    assert rms < tol(model, 1.2e-2, 1.5e-3) and mx < tol(model, 9e-3, 1.1e-3), f"mask logits rel err max {mx:.3e} rms {rms:.3e}"


def compare_runs(model, a, b, cache_a, cache_b, label):
    """Part (2) of test_shared_generate_equals_the_expanded_call for two runs of one model whose prompt passes (and mergers) ran at different
    row counts — the tile GEMM's epilogue rounds by a row's place in the launch, so they are equal up to that rounding seen through the
    network: no further apart than either may be from the fp32 oracle (the oracle test's hidden-row bounds), per quantity.  A wrong fan-out
    destination, key segment or position puts another token's row there: a relative difference of order one.  Prints the measured maxima."""
    diffs = {}

    def d(name, x, y):
        assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape, x.dtype, y.dtype)
        diffs[name] = (x.float() - y.float()).abs().max().item() if x.numel() else 0.0
    d("sequences", a.sequences, b.sequences)
    d("past_image_embeds", a.past_image_embeds, b.past_image_embeds)
    pairs = [("hidden_states[0][-1]", a.hidden_states[0][-1], b.hidden_states[0][-1]),
             ("last_layer_rows", a.hidden_states.last_layer_rows(), b.hidden_states.last_layer_rows())]
    (ka, va), (kb, vb) = cache_a, cache_b
    for name, xa, xb in (("K", ka, kb), ("V^T", va, vb)):
        for i, (la, lb) in enumerate(zip(xa, xb)):
            pairs += [(f"{name} cache layer {i} row {r}", x, y) for r, (x, y) in enumerate(zip(la, lb))]
    for name, x, y in pairs:
        d(name, x, y)
    caches = {k: v for k, v in diffs.items() if "cache" in k}
    print(f"\n[{label}, {model.dtype}] max |difference| per quantity: " + ", ".join(f"{k} {v:.3e}" for k, v in diffs.items() if "cache" not in k)
          + f"; cache images (below each row's length): max {max(caches.values()):.3e}, non-zero in {sum(v != 0.0 for v in caches.values())} of {len(caches)}")
    lim_rms, lim_mx = tol(model, 2e-2, 3e-3), tol(model, 8e-2, 1.2e-2)
    for name, x, y in pairs:
        mx, rms = rel_err(x, y)
        assert rms < lim_rms and mx < lim_mx, f"{name}: {label} rel err max {mx:.3e} rms {rms:.3e}"
    return diffs


def test_prefix_generate_against_the_image_index_call(setup, runs):
    cfg, w, model, U, oc, c = setup
    a, b = runs["pref"], runs["shared"]
    L = c["q_ids"].shape[1]
    # row copies of the ViT's patch-level rows, and host integers: bit equality
    assert torch.equal(a.past_high_res_image_embeds, b.past_high_res_image_embeds)
    assert torch.equal(a.past_visual_pe[0], b.past_visual_pe[0]) and torch.equal(a.past_visual_pe[1], b.past_visual_pe[1])
    assert torch.equal(a.past_logit_mask, b.past_logit_mask)
    assert torch.equal(runs["pref_rope"], runs["shared_rope"])
    assert a.sequences.shape == b.sequences.shape == (6, L + T_NEW)
    assert a.past_image_embeds.shape == b.past_image_embeds.shape == (sum(c["n_merged"][u] for u in c["q_index"]), cfg.hidden_size)
    # the merger and the prototype projection ran at N images' rows when the handle was built, the prompt pass at the own tokens' row count
    diffs = compare_runs(model, a, b, runs["pref_cache"], runs["shared_cache"], "prefix vs image_index")
    mx, rms = rel_err(a.past_image_embeds, b.past_image_embeds)
    assert rms < tol(model, 2e-2, 3e-3) and mx < tol(model, 8e-2, 1.2e-2), f"prototype rows: rel err max {mx:.3e} rms {rms:.3e}"
    assert diffs["sequences"] == 0.0, "the existing runs report equal sequences on these inputs"


def test_a_handle_is_read_only_and_serves_any_number_of_calls(setup, runs):
    """The same handle again, after an unrelated plain generate on the same session lane: bit-equal outputs, the handle's tensors unchanged."""
    cfg, w, model, U, oc, c = setup
    grid, pix, ids, am = U.synthetic_batch(cfg, c["q_grid_x"].tolist(), n_pre=15, n_post=60, ragged=True, seed=5)
    model.generate(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, max_new_tokens=T_NEW,
                   schedule=sched_rec(U), do_sample=False)
    with no_vit(model):
        again = model.generate(**runs["gen"], **prefix_kw(c, runs["handle"]))
    first = runs["pref"]
    assert torch.equal(again.sequences, first.sequences)
    assert torch.equal(again.hidden_states.last_layer_rows(), first.hidden_states.last_layer_rows())
    assert torch.equal(again.hidden_states[0][-1], first.hidden_states[0][-1])
    assert torch.equal(again.past_image_embeds, first.past_image_embeds)
    assert torch.equal(again.past_high_res_image_embeds, first.past_high_res_image_embeds)
    ka, va = cache_rows(again.past_key_values, [l + T_NEW - 1 for l in runs["lens"]])
    kb, vb = runs["pref_cache"]
    assert all(torch.equal(x, y) for la, lb in zip(ka + va, kb + vb) for x, y in zip(la, lb))
    for name, t in handle_tensors(runs["handle"]).items():
        assert torch.equal(t, runs["kept"][name]), f"the handle's {name} changed"
    assert runs["handle"].twin is None


def test_merged_runner_with_prefix_equals_single_calls(setup):
    """PipelinedRunner(merge=2) with prefix= on both batches (each its own handle): one decode session, the second batch's cached rows land at
    row0 = 6 — results equal two plain rec_batch(prefix=) calls bit for bit."""
    cfg, w, model, U, oc, c = setup
    import padt_amd
    from padt_amd import pipeline
    sched = sched_rec(U)
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 40), 2)
    proc.model_embed_token_size = cfg.vocab_size
    batches = [c, prefix_case(cfg, seed=78)]
    handles = [model.encode_prefix(*prefix_inputs(x)) for x in batches]
    args = lambda x: (x["q_ids"].cuda().clone(), x["q_am"].cuda(), None, None)
    with no_vit(model):
        alone = [pipeline.rec_batch(model, proc, *args(x), max_new_tokens=T_NEW, schedule=sched, prefix=h, image_index=x["q_index"])
                 for x, h in zip(batches, handles)]
        assert alone[0][3] != alone[1][3]
        runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
        got = []
        for x, h in zip(batches, handles):
            got += runner.submit(*args(x), max_new_tokens=T_NEW, schedule=sched, prefix=h, image_index=x["q_index"])
        got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2
    for (d0, c0, l0, v0), (d1, c1, l1, v1) in zip(alone, got):
        assert c0 == c1 and v0 == v1 and len(c0) == 6
        assert torch.equal(d0["pred_boxes"], d1["pred_boxes"]) and torch.equal(d0["pred_mask"], d1["pred_mask"])
        assert torch.equal(d0["pred_score"], d1["pred_score"])
    # ... and rec_batch(image_index=) with the images gives the same completions
    x = batches[0]
    plain = pipeline.rec_batch(model, proc, x["q_ids"].cuda().clone(), x["q_am"].cuda(), x["pix"].cuda(), x["grid"], max_new_tokens=T_NEW,
                               schedule=sched, image_index=x["q_index"])
    assert plain[1] == alone[0][1] and plain[3] == alone[0][3]


def test_score_completions_with_a_prefix(setup, runs):
    """forced_tokens + output_token_logprobs through score_completions(prefix=) against score_completions(image_index=): equal sequences, the
    step rows within compare_runs' bounds, and every token log-prob within 2 x (the max-norm bound of the rows, relative to the largest finite
    logit): a log-softmax moves by at most twice what its row moves by."""
    cfg, w, model, U, oc, c = setup
    L = c["q_ids"].shape[1]
    free = runs["shared"].sequences[:, L:].cpu()
    comp = [free[b, : 3 + b].tolist() for b in range(6)]          # ragged completions, VRT tokens among them
    kw = dict(schedule=sched_rec(U)[:8], output_scores=True)
    lens = [l + 8 - 1 for l in runs["lens"]]
    a = model.score_completions(c["q_ids"].cuda(), c["q_am"].cuda(), None, None, comp, prefix=runs["handle"], image_index=c["q_index"], **kw)
    cache_a = cache_rows(a.past_key_values, lens)                 # copied now: the two calls use one session
    b = model.score_completions(c["q_ids"].cuda(), c["q_am"].cuda(), c["pix"].cuda(), c["grid"], comp, image_index=c["q_index"], **kw)
    assert torch.equal(a.sequences, b.sequences) and a.sequences.shape[1] == L + 8
    for r, cmp_ in enumerate(comp):
        assert a.sequences[r, L: L + len(cmp_)].tolist() == cmp_
    compare_runs(model, a, b, cache_a, cache_rows(b.past_key_values, lens), "score_completions: prefix vs image_index")
    top = max(s[torch.isfinite(s)].abs().max().item() for s in b.scores)
    dl = (a.completion_token_logprobs - b.completion_token_logprobs).abs().max().item()
    dc = (a.completion_logprobs - b.completion_logprobs).abs().max().item()
    print(f"[score_completions, {model.dtype}] max |d token log-prob| {dl:.3e}, max |d completion log-prob| {dc:.3e}, largest logit {top:.3e}")
    assert torch.equal(a.completion_token_logprobs != 0, b.completion_token_logprobs != 0)
    assert dl <= 2 * tol(model, 8e-2, 1.2e-2) * top


# ------------------------------------------------------------------------------------------------------------ range guard
def test_range_guard_with_a_prefix():
    """operands="auto", the weight edit of test_bf16_rerun_of_a_flagged_batch_keeps_the_image_index (the existing overflow-flag path): the
    build is flagged and answered by the bf16 twin, calls with that handle run on the twin — the bf16 model's own prefix run, bit for bit —
    and nothing is built a second time.  Then the other direction on unedited weights: the twin asked with an fp16 handle builds the
    handle's bf16 rows once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    clean = U.bf16_weights(cfg, seed=21, std=0.05)
    w = dict(clean)
    for name, idx, val in (("model.layers.0.self_attn.o_proj.weight", (7, slice(None)), 8192.0), ("model.layers.1.mlp.gate_proj.weight", (3, 7), 32.0),
                           ("model.layers.1.mlp.up_proj.weight", (3, 7), 32.0)):
        w[name] = w[name].clone()
        w[name][idx] = val
    c = prefix_case(cfg)
    gen = dict(max_new_tokens=T_NEW, schedule=sched_rec(U))

    def same(x, y):
        return (torch.equal(x.sequences, y.sequences) and torch.equal(x.hidden_states.last_layer_rows(), y.hidden_states.last_layer_rows())
                and torch.equal(x.hidden_states[0][-1], y.hidden_states[0][-1]) and torch.equal(x.past_image_embeds, y.past_image_embeds))
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16")
    want = ref.generate(**gen, **prefix_kw(c, ref.encode_prefix(*prefix_inputs(c))))
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    assert auto.dtype == F16
    with pytest.warns(RuntimeWarning, match="the prefix is built on the bf16"):
        h = auto.encode_prefix(*prefix_inputs(c))
    assert h.dtype == BF and auto.overflow_reruns == 1
    got = auto.generate(**gen, **prefix_kw(c, h))
    assert same(got, want) and auto.overflow_reruns == 1          # the call went to the twin directly: no second pass
    builds = []
    for m in (auto, auto.fallback_model()):
        m._build_prefix = lambda *a, **k: builds.append(1)
    again = auto.generate(**gen, **prefix_kw(c, h))
    assert same(again, want) and not builds and h.twin is None and auto.overflow_reruns == 1
    # an fp16 handle asked for by the twin (what the re-run of a flagged call does): its bf16 rows are built once, from the kept inputs
    ref2 = PaDTForConditionalGeneration(cfg, clean, device="cuda", operands="bf16")
    want2 = ref2.generate(**gen, **prefix_kw(c, ref2.encode_prefix(*prefix_inputs(c))))
    auto2 = PaDTForConditionalGeneration(cfg, clean, device="cuda", operands="auto")
    h16 = auto2.encode_prefix(*prefix_inputs(c))
    assert h16.dtype == F16 and h16.twin is None and auto2.overflow_reruns == 0
    twin = auto2.fallback_model()
    got2 = twin.generate(**gen, **prefix_kw(c, h16))
    built = h16.twin
    assert built is not None and built.dtype == BF and same(got2, want2)
    assert same(twin.generate(**gen, **prefix_kw(c, h16)), want2) and h16.twin is built
    with pytest.raises(ValueError, match="the prefix was built with torch.bfloat16 operands"):
        PaDTForConditionalGeneration(cfg, clean, device="cuda", operands="fp16").generate(**gen, **prefix_kw(c, built))
