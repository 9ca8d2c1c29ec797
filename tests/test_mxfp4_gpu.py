"""MXFP4 LLM weights on the GPU (llm_weights="fp4"): the WQ = 3 instantiation of the skinny GEMM against the 16-bit packed kernel on the
dequantised matrix — bit for bit, which also decides whether the hardware e2m1 → 16-bit conversion is exact for every code and block
exponent the quantiser emits (fp16 subnormals included) — and the decode path end to end.

The kernel tests run for both operand types.  Tolerances against fp32 statements are the ones the fp8 weight path is held to: close_bf16 at
one rounding for 16-bit outputs, close_f32 at 3e-5 of the rms for the fp32 stream (test_kernels_gpu.py)."""
import dataclasses

import pytest
import torch

from edge_util import outside_unchanged
from test_kernels_gpu import close_bf16, close_f32

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
X16 = pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
SHAPES = [(1, 96, 256), (33, 96, 256), (40, 704, 512), (64, 2048, 2080), (8, 2560, 2048), (128, 512, 1024)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def rnd(dt, *shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


def weights(ops, dt, N, K, seed):
    """N(0, 0.05^2) rows, one x40, one x1e-3, one x1e-6 (the fp16 exponent clamp bites: fp16 subnormal fragments) and one all-zero block →
    (nibble image, exponents, 16-bit packed image of the dequantised matrix, dequantised matrix)."""
    w = rnd(dt, N, K, scale=0.05, seed=seed).float()
    w[3] *= 40.0
    w[5] *= 1e-3
    w[7] *= 1e-6
    w[9, 32:64] = 0.0
    codes, exps, deq = ops.quantize_mxfp4_rows(w.to(dt), dt)
    assert torch.equal(ops.dequantize_mxfp4(codes, exps), deq.double())
    if dt == F16:
        assert int(exps[7].max()) == 127 + ops.mxfp4_min_exponent(F16) and bool((deq[7] != 0).any())    # clamped, and not flushed to nothing
    img, ex = ops.pack_weight_fp4(codes, exps)
    return img, ex, ops.pack_weight(deq), deq


def packed(ops, x, M):
    M16 = (M + 15) // 16 * 16
    xp = torch.zeros(M16, x.shape[1], device="cuda", dtype=x.dtype)
    ops.pack_rows(x, xp, M, to_packed=True)
    return xp


def unpacked(ops, buf, M):
    un = torch.zeros(M, buf.shape[1], device="cuda", dtype=buf.dtype)
    ops.pack_rows(buf, un, M, to_packed=False)
    return un


@X16
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fp4_kernel_is_the_16bit_kernel_on_the_dequantised_matrix(ops, dt, M, N, K):
    """Every variant the decode step uses — norm + bias, EPI_RESID, EPI_SWIGLU with packed A / C, split-K, the fp32-stream form (with and
    without split-K) — equals the 16-bit packed kernel on pack_weight(w_deq) bit for bit, and meets the fp32 statement on w_deq."""
    img, ex, wp, deq = weights(ops, dt, N, K, seed=82)
    x, b, r = rnd(dt, M, K, seed=81), rnd(dt, N, seed=83), rnd(dt, M, N, seed=84)
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)
    lin = xf @ deq.float().T
    tag = f"{M}x{N}x{K} {dt}"
    # norm + bias
    got = ops.gemm_packed_fp4(x, img, ex, N, b, norm_eps=1e-6)
    assert got.dtype == dt and torch.equal(got, ops.gemm_packed(x, wp, N, b, norm_eps=1e-6)), f"norm+bias {tag}: fp4 != 16-bit kernel on w_deq"
    close_bf16(got, lin * rstd + b.float(), f"fp4 norm+bias {tag}")
    assert torch.equal(got, ops.gemm_packed(x, img, N, b, norm_eps=1e-6, exps=ex))            # the route through ops.gemm_packed
    # residual epilogue, in place
    out, want = r.clone(), r.clone()
    ops.gemm_packed_fp4(x, img, ex, N, out=out, epilogue=ops.EPI_RESID, residual=out)
    ops.gemm_packed(x, wp, N, out=want, epilogue=ops.EPI_RESID, residual=want)
    assert torch.equal(out, want), f"resid {tag}"
    close_bf16(out, lin + r.float(), f"fp4 resid {tag}")
    # split-K
    if N >= 256:
        ws = ops.new_splitk_workspace(N, 2, "cuda")
        got = ops.gemm_packed_fp4(x, img, ex, N, b, split_k=2, workspace=ws)
        assert torch.equal(got, ops.gemm_packed(x, wp, N, b, split_k=2, workspace=ws)), f"split-K {tag}"
        close_bf16(got, lin + b.float(), f"fp4 split-K {tag}")
        out, want = r.clone(), r.clone()
        ops.gemm_packed_fp4(x, img, ex, N, out=out, epilogue=ops.EPI_RESID, residual=out, split_k=2, workspace=ws)
        ops.gemm_packed(x, wp, N, out=want, epilogue=ops.EPI_RESID, residual=want, split_k=2, workspace=ws)
        assert torch.equal(out, want), f"resid split-K {tag}"
    # SwiGLU + norm over packed A / C
    xp = packed(ops, x, M)
    hp, hw = torch.zeros(xp.shape[0], N // 2, device="cuda", dtype=dt), torch.zeros(xp.shape[0], N // 2, device="cuda", dtype=dt)
    ops.gemm_packed_fp4(xp, img, ex, N, b, out=hp, epilogue=ops.EPI_SWIGLU, norm_eps=1e-6, a_packed=True, c_packed=True, rows=M)
    ops.gemm_packed(xp, wp, N, b, out=hw, epilogue=ops.EPI_SWIGLU, norm_eps=1e-6, a_packed=True, c_packed=True, rows=M)
    assert torch.equal(unpacked(ops, hp, M), unpacked(ops, hw, M)), f"SwiGLU {tag}"
    y = (lin * rstd + b.float()).view(M, N // 32, 2, 16)
    close_bf16(unpacked(ops, hp, M), (torch.nn.functional.silu(y[:, :, 0]) * y[:, :, 1]).reshape(M, N // 2), f"fp4 SwiGLU {tag}")
    # the fp32-stream form: x32 += a w^T in place, mirror = X(stream_scale * x32) packed
    s = ops.stream_scale(dt)
    x0 = r.float().contiguous()
    for split in ((1, 2) if N >= 256 else (1,)):
        ws = ops.new_splitk_workspace(N, split, "cuda") if split > 1 else None
        st, sw = x0.clone(), x0.clone()
        mir, mw = torch.zeros(xp.shape[0], N, device="cuda", dtype=dt), torch.zeros(xp.shape[0], N, device="cuda", dtype=dt)
        ops.gemm_packed_resid32_fp4(xp, img, ex, N, st, mir, split_k=split, workspace=ws, rows=M)
        ops.gemm_packed_resid32(xp, wp, N, sw, mw, split_k=split, workspace=ws, rows=M)
        assert torch.equal(st, sw) and torch.equal(unpacked(ops, mir, M), unpacked(ops, mw, M)), f"resid32 split {split} {tag}"
        close_f32(st, x0 + lin, f"fp4 resid32 split {split} {tag}", rel=3e-5)
        assert torch.equal(unpacked(ops, mir, M), (st * s).to(dt)), "packed mirror != X(stream_scale * stream)"
        sr = x0.clone()
        ops.gemm_packed_resid32(xp, img, N, sr, mir, exps=ex, split_k=split, workspace=ws, rows=M)    # the route through ops.gemm_packed_resid32
        assert torch.equal(sr, st)


@X16
def test_a_rows_bits_do_not_depend_on_the_row_count(ops, dt):
    """Row 0 is bit-identical at 1, 16, 64 and 128 rows (MT = 1, 1, 4, 8): in-flight batching must not change a sample's tokens."""
    N, K = 704, 2048
    img, ex, wp, deq = weights(ops, dt, N, K, seed=26)
    x, b = rnd(dt, 128, K, seed=25), rnd(dt, N, seed=27)
    ws = ops.new_splitk_workspace(N, 2, "cuda")
    first = None
    for M in (1, 16, 64, 128):
        xp = packed(ops, x[:M].contiguous(), M)
        h = torch.zeros(xp.shape[0], N // 2, device="cuda", dtype=dt)
        ops.gemm_packed_fp4(xp, img, ex, N, b, out=h, epilogue=ops.EPI_SWIGLU, norm_eps=1e-6, a_packed=True, c_packed=True, rows=M)
        st = torch.ones(M, N, device="cuda")
        ops.gemm_packed_resid32_fp4(xp, img, ex, N, st, torch.zeros(xp.shape[0], N, device="cuda", dtype=dt), split_k=2, workspace=ws, rows=M)
        rows = (ops.gemm_packed_fp4(x[:M], img, ex, N, b, norm_eps=1e-6)[0].clone(), unpacked(ops, h, M)[0].clone(), st[0].clone())
        if first is None:
            first = rows
        for a, c, what in zip(first, rows, ("norm+bias", "SwiGLU", "resid32 split-K")):
            assert torch.equal(a, c), f"{what}: row 0 at {M} rows differs from row 0 alone"


@X16
def test_strided_output_window_in_a_poisoned_neighbourhood(ops, dt):
    """The output is a strided window of a NaN-filled buffer, the activations, the nibble image and the exponents are each followed by poison
    (NaN; 0xFF bytes: the codes -6 | -6 under the E8M0 NaN exponent): nothing outside the window changes, no NaN gets in, and the result is
    the clean run's.  K = 2080: an odd number of K-steps, so the last pair's second half is the image's own zero padding."""
    M, N, K = 40, 704, 2080
    img, ex, wp, deq = weights(ops, dt, N, K, seed=52)
    x, b = rnd(dt, M, K, seed=51), rnd(dt, N, seed=53)
    clean = ops.gemm_packed_fp4(x, img, ex, N, b, norm_eps=1e-6)
    img_b = torch.full((img.numel() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    ex_b = torch.full((ex.numel() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    x_b = torch.full((M + 256, K), float("nan"), dtype=dt, device="cuda")
    img_b[: img.numel()] = img.view(-1)
    ex_b[: ex.numel()] = ex.view(-1)
    x_b[:M] = x
    r0, c0, ld = 256, 128, 128 + N + 144
    backing = torch.full((r0 + M + 256, ld), float("nan"), dtype=dt, device="cuda")
    out = backing[r0:r0 + M, c0:c0 + N]
    ops.gemm_packed_fp4(x_b[:M], img_b[: img.numel()].view(img.shape), ex_b[: ex.numel()].view(ex.shape), N, b, out=out, norm_eps=1e-6)
    assert torch.isfinite(out).all(), "poison reached the output"
    assert torch.equal(out, clean)
    outside_unchanged(backing, (r0, c0, M, N), float("nan"))
    # the fp32 stream in place in a window, split-K, packed A followed by NaN blocks
    xp = packed(ops, x, M)
    xp_b = torch.full((xp.shape[0] + 64, K), float("nan"), dtype=dt, device="cuda")
    xp_b[: xp.shape[0]] = xp
    x0 = rnd(torch.float32, M, N, seed=54)
    ws = ops.new_splitk_workspace(N, 2, "cuda")
    want, mir = x0.clone(), torch.zeros(xp.shape[0], N, device="cuda", dtype=dt)
    ops.gemm_packed_resid32_fp4(xp, img, ex, N, want, mir, split_k=2, workspace=ws, rows=M)
    back32 = torch.full((r0 + M + 256, ld), float("nan"), device="cuda")
    st = back32[r0:r0 + M, c0:c0 + N]
    st.copy_(x0)
    mir2 = torch.zeros_like(mir)
    ops.gemm_packed_resid32_fp4(xp_b[: xp.shape[0]], img_b[: img.numel()].view(img.shape), ex_b[: ex.numel()].view(ex.shape), N, st, mir2,
                                split_k=2, workspace=ws, rows=M)
    assert torch.equal(st, want) and torch.equal(unpacked(ops, mir2, M), unpacked(ops, mir, M))
    outside_unchanged(back32, (r0, c0, M, N), float("nan"))


def test_argument_validation(ops):
    from padt_amd import _lib
    x = rnd(BF, 8, 64)
    codes, exps, _ = ops.quantize_mxfp4_rows(rnd(BF, 32, 64), BF)
    img, ex = ops.pack_weight_fp4(codes, exps)
    with pytest.raises(_lib.PaDTHipError, match="padt_gemm_packed_fp4"):
        ops.gemm_packed_fp4(x, img, ex, 24)                                       # N % 16
    with pytest.raises(_lib.PaDTHipError, match="padt_gemm_packed_fp4"):
        ops.gemm_packed_fp4(x[:, :40], img, ex, 32)                               # K % 32
    odd = torch.zeros(ex.numel() + 16, dtype=torch.uint8, device="cuda")[1:1 + ex.numel()]
    with pytest.raises(_lib.PaDTHipError, match="padt_gemm_packed_fp4"):
        ops.gemm_packed_fp4(x, img, odd, 32)                                      # exponents not 16-byte aligned


# ---------------------------------------------------------------------------------------------------------------- end to end
_MODELS = {}
OPERANDS = pytest.mark.parametrize("operands", ["fp16", "bf16"])


def fp4_model(operands):
    """The 512-wide untied GQA model of test_fp8_llm_weights_against_oracle_on_dequantised_weights, built with llm_weights="fp4", and its
    generate() on that test's inputs — built once per operand type."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if operands in _MODELS:
        return _MODELS[operands]
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    cfg = dataclasses.replace(cfg, tie_word_embeddings=False, num_attention_heads=4, num_key_value_heads=2, hidden_size=512)
    cfg = dataclasses.replace(cfg, vision_config=dataclasses.replace(cfg.vision_config, out_hidden_size=512))
    w = U.bf16_weights(cfg, seed=19, std=0.05)
    model = PaDTForConditionalGeneration(cfg, w, device="cuda", llm_weights="fp4", operands=operands)
    W = model.W
    assert W.llm_weights == "fp4" and not W.fp8_prefill
    for nm in ("qkv", "o", "gu", "down"):                                         # the decode images are the fp4 ones; no 16-bit or fp8 image is kept
        assert f"llm.0.{nm}.w4" in W and f"llm.0.{nm}.we" in W and W[f"llm.0.{nm}.w4"].dtype == torch.uint8
        assert f"llm.0.{nm}.wp" not in W and f"llm.0.{nm}.wq" not in W and f"llm.0.{nm}.w8" not in W
        assert W[f"llm.0.{nm}.w"].dtype == model.dtype
    assert "llm.head.wp" in W and W["llm.head.wp"].dtype == model.dtype            # the head table stays 16-bit
    grids = [[1, 8, 8], [1, 10, 12]]
    grid, pix, ids, am = U.synthetic_batch(cfg, grids, n_pre=5, n_post=8, ragged=True, seed=77)
    T = 12
    sched = U.rec_schedule(T, vrt_at=range(4, 8))
    out = model.generate(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, max_new_tokens=T,
                         schedule=sched, output_hidden_states=True, return_dict_in_generate=True)
    _MODELS[operands] = dict(cfg=cfg, w=w, model=model, U=U, batch=(grid, pix, ids, am), T=T, sched=sched, out=out, operands=operands)
    return _MODELS[operands]


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item(), ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()


def test_fp4_llm_weights_against_oracle_on_dequantised_weights():
    """Ids by the margin rule (floor 2e-2 of the logit range) and hidden rows within the bounds of the "fp8" case of
    test_fp8_llm_weights_against_oracle_on_dequantised_weights — after dequantisation the arithmetic is the same 16-bit-operand arithmetic — against
    the fp32 oracle on parity_util.effective_llm_weights; the quantisation itself is visible against the un-quantised oracle.
    Runs on that test's operand type (the default, fp16), which is what its bounds were measured on."""
    f = fp4_model("fp16")
    model, U, (grid, pix, ids, am), T, sched, out = f["model"], f["U"], f["batch"], f["T"], f["sched"], f["out"]
    O = U.O
    wo = U.effective_llm_weights(model, f["w"])
    oc = U.oracle_config(f["cfg"])
    toks = out.sequences.cpu()[:, ids.shape[1]:]
    ores = O.generate(wo, oc, ids, am, pix, grid, T, schedule=sched, collect_logits=True, force_tokens=toks)
    n_tie = 0
    for t in range(T):
        lg = ores["logits"][t]
        top2 = lg.topk(2, dim=-1).values
        chosen = lg.gather(1, toks[:, t:t + 1]).squeeze(1)
        floor = 2e-2 * lg[torch.isfinite(lg)].abs().max().item()
        for b in range(2):
            second = top2[b, 1] if torch.isfinite(top2[b, 1]) else top2[b, 0] - 1
            if (top2[b, 0] - second).item() > floor:
                assert chosen[b] == top2[b, 0], f"step {t} sample {b}: not the oracle argmax"
            else:
                n_tie += 1
                assert (top2[b, 0] - chosen[b]).item() <= floor
    assert n_tie <= T
    hid = out.hidden_states.last_layer_rows().cpu().float()
    worst = 0.0
    for t in range(T):
        mx, rms = rel_err(hid[t], ores["hidden"][t][:, -1].float())
        worst = max(worst, rms)
        print(f"[fp4 e2e, 512-wide] hidden step {t}: rel err max {mx:.3e} rms {rms:.3e}")
        assert rms < 5e-3 and mx < 2e-2, f"hidden step {t}: rel err max {mx:.3e} rms {rms:.3e}"
    ores0 = O.generate(f["w"], oc, ids, am, pix, grid, 1, schedule=sched)
    _, rms0 = rel_err(hid[0], ores0["hidden"][0][:, -1].float())
    print(f"[fp4 e2e, 512-wide] hidden rel rms worst {worst:.3e}; against the un-quantised oracle at step 0: {rms0:.3e}")
    assert rms0 > 2e-2


@OPERANDS
def test_fp4_model_is_the_16bit_model_on_the_dequantised_weights(operands):
    """A model with 16-bit LLM weights built from the state dict effective_llm_weights returns gives the same sequences and hidden rows, bit for
    bit: prefill reads the same 16-bit image and the fp4 decode kernels are bit-identical to the 16-bit ones."""
    from padt_amd.modeling import PaDTForConditionalGeneration
    f = fp4_model(operands)
    model, U, (grid, pix, ids, am), T, sched, out = f["model"], f["U"], f["batch"], f["T"], f["sched"], f["out"]
    twin = PaDTForConditionalGeneration(f["cfg"], U.effective_llm_weights(model, f["w"]), device="cuda", llm_weights="bf16", operands=f["operands"])
    assert "llm.0.qkv.wp" in twin.W and "llm.0.qkv.w4" not in twin.W
    for nm in ("qkv", "o", "gu", "down"):
        assert torch.equal(twin.W[f"llm.1.{nm}.w"], model.W[f"llm.1.{nm}.w"])
    ref = twin.generate(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid, max_new_tokens=T,
                        schedule=sched, output_hidden_states=True, return_dict_in_generate=True)
    assert torch.equal(out.sequences, ref.sequences)
    assert out.hidden_states.n == ref.hidden_states.n == T
    assert torch.equal(out.hidden_states.buf, ref.hidden_states.buf)


@OPERANDS
def test_fp4_merged_decode_group_matches_sequential(operands):
    """PipelinedRunner(merge=2): two batches share one decode session over the fp4 images — identical to one rec_batch call per batch."""
    import padt_amd
    from padt_amd import pipeline
    f = fp4_model(operands)
    cfg, model, U = f["cfg"], f["model"], f["U"]
    T = 9
    sched = U.rec_schedule(T, vrt_at=range(3, 6))
    proc = padt_amd.VisonTextProcessingClass(U.FakeProcessor(cfg, 40), 2)
    proc.model_embed_token_size = cfg.vocab_size
    batches = []
    for s, g in enumerate([[[1, 8, 8], [1, 10, 12]], [[1, 6, 10], [1, 8, 8]], [[1, 10, 12], [1, 10, 12]]]):
        grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5 + s % 2, n_post=7, seed=100 + s, ragged=True)
        batches.append((ids.cuda(), am.cuda(), pix.cuda(), grid))
    ref = [pipeline.rec_batch(model, proc, b[0].clone(), b[1], b[2], b[3], max_new_tokens=T, schedule=sched) for b in batches]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b in batches:
        got += runner.submit(b[0].clone(), b[1], b[2], b[3], max_new_tokens=T, schedule=sched)
    got += runner.flush()
    assert len(got) == len(batches)
    for (d0, c0, l0, v0), (d1, c1, l1, v1) in zip(ref, got):
        assert c0 == c1 and v0 == v1
        assert torch.equal(d0["pred_boxes"], d1["pred_boxes"]) and torch.equal(d0["pred_mask"], d1["pred_mask"])
        assert torch.equal(d0["pred_score"], d1["pred_score"])
