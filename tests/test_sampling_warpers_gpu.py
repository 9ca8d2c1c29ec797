"""generate(min_p=, typical_p=, epsilon_cutoff=, eta_cutoff=) on the device: padt_warp_sample_rows_f32 against the fp64 reference chain of
tests/sampling_warpers_util.py (itself pinned to HF's classes by tests/test_sampling_warpers_cpu.py), its draw distribution, its values read
from device memory by a captured graph, and generate() end to end against HF's full warper list."""
import math

import pytest
import torch

import sampling_warpers_util as W

pytestmark = pytest.mark.gpu
INF = float("inf")
SENTINEL = 0x7FFFFFFF


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops
    return ops


def cfg_tensor(ops, seed=1, T=1.0, top_k=0, min_p=0.0, typical_p=1.0, eps=0.0, eta=0.0):
    return ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=seed, temperature=T, top_k=top_k, top_p=1.0, write_back=True, min_p=min_p,
                              typical_p=typical_p, epsilon_cutoff=eps, eta_cutoff=eta)


def poisoned(rows, pad=12):
    """(B, n) → device (B, n + pad) with +inf / NaN past n"""
    B, n = rows.shape
    x = torch.empty((B, n + pad), dtype=torch.float32)
    x[:, :n] = rows
    x[:, n::2] = INF
    x[:, n + 1::2] = float("nan")
    return x.cuda()


def launch(ops, x, n, cfg, t, B):
    pv = torch.full((B,), 3.0, device="cuda")
    pi = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    ops.warp_sample_rows(x, n, cfg, torch.tensor([t], dtype=torch.int32, device="cuda"), pv, pi, B)
    return pv.cpu(), pi.cpu().long()


# ------------------------------------------------------------------------------------------------------------ support, values, draws
# (n, setting, top_k of the sample_token pass that prepares the rows, scale of the rows).  Half of the cases (10 of 22) go through top_k = 40:
# the kernel then starts from 40 survivors in its LDS list.  With top_k = 0 every finite column is a candidate: at full width min_p runs
# over the row in place, and what it leaves is warped in the list (the peaked row: 794 of 104 000 survive min_p = 0.02) or by sweeps over
# the row itself (the flat row: 34 074 survive).
FULL = (dict(min_p=0.05), dict(typical_p=0.9), dict(eps=3e-4), dict(eta=3e-4))
CASES = ([(3000, s, 40 if i % 2 == 0 else 0, 1.0) for i, s in enumerate(W.SINGLE)]
         + [(n, W.COMBINED, 40 if i % 2 == 0 else 0, 1.0) for i, n in enumerate(W.WIDTHS)]
         + [(W.FULL_WIDTH, s, 0, 1.0) for s in FULL] + [(W.FULL_WIDTH, s, 40, 1.0) for s in FULL]
         + [(W.FULL_WIDTH, W.COMBINED, 0, 1.0), (W.FULL_WIDTH, W.COMBINED, 0, 0.5)])


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"n{n}-{W.setting_id(s)}-k{k}-x{x:g}" for n, s, k, x in CASES])
def test_support_values_and_draws(ops, case):
    n, setting, top_k, scale = CASES[case]
    T = 0.7 if top_k else 1.0                                       # rows as sample_token's write_back leaves them
    B, steps = 16, 24
    cap = W.AMBIGUOUS_MAX if n <= 3000 else W.AMBIGUOUS_MAX_FULL
    x = poisoned(W.make_rows(n, 1.0, seed=case) * scale)
    cfg = cfg_tensor(ops, seed=11 + case, T=T, top_k=top_k, **setting)
    pv = torch.zeros(B, device="cuda")
    pi = torch.zeros(B, dtype=torch.int32, device="cuda")
    ops.sample_token(x, n, cfg, torch.zeros(1, dtype=torch.int32, device="cuda"), pv, pi, B)
    pre_dev = x.clone()
    pre = pre_dev.cpu()
    assert int((pre[:, :n] > -INF).sum(1).max()) <= (max(top_k, 1) if 0 < top_k < n else n)
    ref = [W.ref_chain(pre[r, :n], **setting) for r in range(B)]
    if n == W.FULL_WIDTH and top_k == 0 and "min_p" in setting:    # the case is what its comment says: which side of the list's 4096 entries
        left = int(W.ref_chain(pre[0, :n], min_p=setting["min_p"])[0].sum())
        assert (left > 4096) == (scale < 1.0) and left > 1, left
    for r, (kept, amb) in enumerate(ref):                           # the cap holds on the reference before the device is looked at
        assert int(amb.sum()) <= cap, (r, int(amb.sum()))
    draws = []
    for t in range(steps):
        x.copy_(pre_dev)
        val, tok = launch(ops, x, n, cfg, t, B)
        out = x.cpu()
        assert torch.equal(out[:, n:].view(torch.int32), pre[:, n:].view(torch.int32)), "the padding past n was touched"
        for r, (kept, amb) in enumerate(ref):
            got = out[r, :n] > -INF
            if t == 0:
                W.check_support(got, kept, amb, cap, f"row {r}")
                assert torch.equal(out[r, :n][got].view(torch.int32), pre[r, :n][got].view(torch.int32)), "a kept value changed"
                assert not torch.isnan(out[r, :n]).any() and bool((out[r, :n][~got] == -INF).all())
            else:
                assert torch.equal(got, first[r]), "the support depends on the step"
            assert 0 <= int(tok[r]) < n and bool((kept | amb)[tok[r]]) and bool(got[tok[r]]), (t, r, int(tok[r]))
        if t == 0:
            first = [out[r, :n] > -INF for r in range(B)]
        draws.append(tok)
    x.copy_(pre_dev)
    assert torch.equal(launch(ops, x, n, cfg, 5, B)[1], draws[5]), "the same (seed, step, row) must give the same draw"
    if n > 1 and max(int(f.sum()) for f in first) > 1:
        assert len({tuple(d.tolist()) for d in draws}) > 1, "every step drew the same tokens"


def test_planted_rows(ops):
    """the cases random rows miss (sampling_warpers_util.planted_rows; the reference's answer there is checked on the CPU)"""
    rows, expect, settings = W.planted_rows()
    B, n = rows.shape
    x = poisoned(rows)
    before = x.clone()
    for r, setting in enumerate(settings):
        val, tok = launch(ops, x[r: r + 1], n, cfg_tensor(ops, seed=9, **setting), 3, 1)
        out = x[r].cpu()
        assert torch.equal(out[:n] > -INF, expect[r]), f"row {r} {setting}: kept {(out[:n] > -INF).nonzero().flatten().tolist()[:8]}"
        assert torch.equal(out[:n][expect[r]], rows[r][expect[r]]) and torch.equal(out[n:].view(torch.int32), before[r, n:].cpu().view(torch.int32))
        if not expect[r].any():
            assert int(tok[0]) == SENTINEL and float(val[0]) == -INF        # what sample_token writes for such a row: greedy_step emits pad
        else:
            assert bool(expect[r, tok[0]])


def test_draw_distribution(ops):
    """4096 draws (64 identical rows x 64 steps) from a row whose final support is five entries of probability .4 / .25 / .2 / .1 / .05: min_p = 0.1
    removes 60 entries of relative mass 1e-3 each first.  Every count within 5 binomial standard deviations.  Deterministic for the seed."""
    n, B, steps = 1500, 64, 64
    p = torch.tensor([0.4, 0.25, 0.2, 0.1, 0.05])
    cols = torch.tensor([3, 700, 1024, 1025, 1499])
    row = torch.full((n,), -INF)
    row[100:160] = math.log(1e-3)
    row[cols] = p.log()
    x = poisoned(row[None].repeat(B, 1))
    pre = x.clone()
    cfg = cfg_tensor(ops, seed=2024, min_p=0.1)
    counts = torch.zeros(5, dtype=torch.long)
    for t in range(steps):
        x.copy_(pre)
        _, tok = launch(ops, x, n, cfg, t, B)
        hit = tok[:, None] == cols[None, :]
        assert bool(hit.any(1).all()), "a draw outside the five survivors"
        counts += hit.sum(0)
    N = B * steps
    sd = (N * p * (1 - p)).sqrt()
    print(f"\n[draw distribution] counts {counts.tolist()} expected {(N * p).tolist()} sd {[round(float(s), 1) for s in sd]}")
    # observed on an MI355X: counts [1670, 999, 788, 426, 213] against 1638.4 / 1024 / 819.2 / 409.6 / 204.8 — at most 1.2 standard deviations off
    assert bool(((counts - N * p).abs() <= 5 * sd).all()), counts.tolist()


def test_a_captured_graph_reads_the_values_from_device_memory(ops):
    n, B = 3000, 4
    rows = W.make_rows(n, 0.7, seed=77, copies=B)
    x = poisoned(rows)
    pre = x.clone()
    cfg = cfg_tensor(ops, seed=5, min_p=0.05)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    pv = torch.zeros(B, device="cuda")
    pi = torch.zeros(B, dtype=torch.int32, device="cuda")

    def body():
        x.copy_(pre)
        ops.warp_sample_rows(x, n, cfg, step, pv, pi, B)
    body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    supports = {}
    for name, setting in (("min_p 0.05", dict(min_p=0.05)), ("min_p 0.5", dict(min_p=0.5)), ("typical 0.2", dict(typical_p=0.2)),
                          ("all off", dict())):
        cfg.copy_(cfg_tensor(ops, seed=5, **setting))                # the captured launch keeps reading the same 16 words
        g.replay()
        torch.cuda.synchronize()
        out = x.cpu()
        for r in range(B):
            kept, amb = W.ref_chain(rows[r], **setting)
            W.check_support(out[r, :n] > -INF, kept, amb, W.AMBIGUOUS_MAX, f"{name} row {r}")
            assert bool((out[r, :n] > -INF)[int(pi[r])])
        supports[name] = int((out[:, :n] > -INF).sum())
    assert supports["min_p 0.5"] < supports["min_p 0.05"] < supports["all off"] == int((rows > -INF).sum())
    assert supports["typical 0.2"] < supports["all off"]


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


WARP = dict(min_p=0.1, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=1e-2)
GEN = dict(do_sample=True, temperature=0.7, top_k=20, max_new_tokens=12, **WARP)


def hf_full_chain():
    from transformers.generation.logits_process import LogitsProcessorList, TemperatureLogitsWarper, TopKLogitsWarper
    head = LogitsProcessorList([TemperatureLogitsWarper(GEN["temperature"]), TopKLogitsWarper(top_k=GEN["top_k"], min_tokens_to_keep=1)])
    tail = W.hf_processors(min_p=WARP["min_p"], typical_p=WARP["typical_p"], eps=WARP["epsilon_cutoff"], eta=WARP["eta_cutoff"])
    return head, tail


def check_generate(model, kw, what):
    """every step's scores have the support of HF's full warper list applied to the step's logits, the token comes from it, and its log-prob is
    log_softmax(scores) there → the run"""
    out = model.generate(seed=321, output_scores=True, output_logits=True, output_token_logprobs=True, **GEN, **kw)
    L = kw["input_ids"].shape[1]
    tok = out.sequences[:, L:].cpu()
    B, T = tok.shape
    assert len(out.scores) == T == len(out.logits) and tuple(out.token_logprobs.shape) == (B, T)
    head, tail = hf_full_chain()
    ids = torch.zeros((B, 1), dtype=torch.long)
    eos = set(model.generation_config.eos_token_id)
    live = torch.ones(B, dtype=torch.bool)
    worst, narrowed = 0.0, 0
    for t in range(T):
        raw, sc = out.logits[t].cpu(), out.scores[t].cpu()
        mid = head(ids, raw.clone())                                  # after temperature / top-k: what the new kernel starts from
        hf = tail(ids, mid.clone()) > -INF
        ls = torch.log_softmax(sc.double(), -1)
        for b in range(B):
            kept, amb = W.ref_chain(mid[b], min_p=WARP["min_p"], typical_p=WARP["typical_p"], eps=WARP["epsilon_cutoff"], eta=WARP["eta_cutoff"])
            W.check_support(sc[b] > -INF, hf[b], amb, W.AMBIGUOUS_MAX, f"step {t} row {b}")
            narrowed += int((mid[b] > -INF).sum()) - int(hf[b].sum())
            got_lp = float(out.token_logprobs[b, t])
            if live[b]:
                assert bool((sc[b] > -INF)[tok[b, t]]), f"step {t} row {b}: token {int(tok[b, t])} outside the support"
                want = float(ls[b, tok[b, t]])
                assert abs(got_lp - want) <= 5e-6 + 2.0 ** -22 * abs(want), (t, b, got_lp, want)
                worst = max(worst, abs(got_lp - want))
            else:
                assert got_lp == 0.0
            if int(tok[b, t]) in eos:
                live[b] = False
    assert narrowed > 0, "the four warpers removed nothing in the whole run: the case has no power"
    print(f"\n[generate, {what}] columns removed after top-k over the run: {narrowed}; largest token log-prob difference {worst:.3e}")
    return out


def test_generate_scores_are_hfs_and_the_token_comes_from_them(setup):
    cfg, w, model, U, kw = setup
    out = check_generate(model, kw, str(model.dtype))
    # the hooked loop (a caller processor that changes nothing) runs the same selection, eagerly
    hooked = model.generate(seed=321, output_scores=True, logits_processor=[lambda i, s: s], **GEN, **kw)
    assert torch.equal(hooked.sequences, out.sequences) and all(torch.equal(a, b) for a, b in zip(hooked.scores, out.scores))
    # the same seed without a captured graph, and another seed
    assert torch.equal(model.generate(seed=321, use_graph=False, **GEN, **kw).sequences, out.sequences)
    assert not torch.equal(model.generate(seed=322, **GEN, **kw).sequences, out.sequences)


@pytest.mark.parametrize("how", [dict(precision="reference"), dict(llm_weights="fp8"), dict(llm_weights="fp4")], ids=["reference", "fp8", "fp4"])
def test_generate_in_the_other_modes_do_sample_works_in(how):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_token_logprobs_gpu as TL
    cfg, U, model = TL.small_model(**how)
    check_generate(model, TL.two_ragged(cfg, U), str(how))


def test_all_four_off_is_the_call_without_them(setup, monkeypatch):
    cfg, w, model, U, kw = setup
    from padt_amd import ops as O
    gen = dict(do_sample=True, temperature=0.7, top_k=20, seed=99, max_new_tokens=12)
    with_warpers = model.generate(**gen, **WARP, **kw)

    def refuse(*a, **k):
        raise AssertionError("padt_warp_sample_rows_f32 launched with every warper off")
    monkeypatch.setattr(O, "warp_sample_rows", refuse)
    plain = model.generate(**gen, **kw)
    off = model.generate(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, **gen, **kw)
    assert torch.equal(off.sequences, plain.sequences)
    assert torch.equal(model.generate(do_sample=False, max_new_tokens=12, **WARP, **kw).sequences,
                       model.generate(do_sample=False, max_new_tokens=12, **kw).sequences)          # ignored under greedy decoding, as in HF
    assert with_warpers.sequences.shape == plain.sequences.shape


def test_a_merged_decode_group_draws_what_each_batch_draws_alone(setup):
    cfg, w, model, U, _ = setup
    import padt_amd
    from padt_amd import pipeline
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 40), 2)
    proc.model_embed_token_size = cfg.vocab_size
    batches = []
    for s, g in enumerate([[[1, 8, 8], [1, 10, 12]], [[1, 6, 10], [1, 8, 8]]]):
        grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5 + 3 * s, n_post=7, seed=100 + s, ragged=True)
        batches.append((ids.cuda(), am.cuda(), pix.cuda(), grid))
    gen = dict(GEN, seed=4242, max_new_tokens=10, schedule=["t"] * 3 + ["v"] * 4 + ["t"] * 2 + ["e"])      # VRT columns are drawn from too
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], **gen) for b in batches]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b in batches:
        got += runner.submit(b[0].clone(), *b[1:], **gen)
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2
    for s, ((d0, c0, l0, v0), (d1, c1, l1, v1)) in enumerate(zip(alone, got)):
        assert c0 == c1 and v0 == v1, f"batch {s}: the merged group drew other tokens than the batch alone"
    # a batch with another min_p does not join the group
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = runner.submit(batches[0][0].clone(), *batches[0][1:], **gen)
    got += runner.submit(batches[1][0].clone(), *batches[1][1:], **dict(gen, min_p=0.2))
    got += runner.flush()
    assert runner.n_groups == 2 and len(got) == 2
    assert got[0][1] == alone[0][1] and got[0][3] == alone[0][3]


def test_the_range_guard_rerun_keeps_the_warpers():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd.modeling import PaDTForConditionalGeneration
    from test_range_guard_gpu import _weights
    cfg, w, U = _weights("llm_swiglu")                               # the layer-1 SwiGLU hidden exceeds fp16's range on every batch
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8], [1, 10, 12]], n_pre=5, n_post=8, ragged=True, seed=41)
    kw = dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    seen = {}
    for name, m in (("auto", auto), ("twin", auto.fallback_model())):
        def spy(opts, *a, _inner=m._launch, _name=name, **k):
            seen.setdefault(_name, []).append(opts)
            return _inner(opts, *a, **k)
        m._launch = spy
    gen = dict(GEN, seed=77, max_new_tokens=4)
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(output_scores=True, **gen, **kw)
    assert auto.overflow_reruns == 1 and len(seen["auto"]) == 1 and len(seen["twin"]) == 1
    assert seen["twin"][0] == seen["auto"][0] and seen["twin"][0].sampling[3:] == (77, 0.1, 0.9, 1e-3, 1e-2)
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16").generate(output_scores=True, **gen, **kw)
    assert torch.equal(got.sequences, ref.sequences) and all(torch.equal(a, b) for a, b in zip(got.scores, ref.scores))
