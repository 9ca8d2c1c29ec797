#!/usr/bin/env python
"""bench.py — images/s of PaDT_Pro_3B REC inference on MI355X (BASELINE.json metric), one process per GPU.

  python bench.py [--gpus N --steps K --warmup W] [--full] (N>1: one rank per GPU under torch.distributed.run — given as typed, the script
                                                           launches itself under it as a child process; rank 0's JSON line is the only stdout line)

A "step" = one batch of `--batch` (default 8) synthetic 640x640-equivalent images (grid [1,46,46], 2116 patches,
529 VRTs, prompt L=577) through the whole hot path with inputs already resident in HBM:
  ViT → prototypes → packed prefill → 27 hipGraph decode steps over text‖VRT (scripted 28-token REC completion: one run
  of 5 VRTs, forced EOS) → parseVRTintoCompletion → PaDT decoder (boxes + 184x184 mask logits) [→ RCCL all-gather].
Weights: random-init PaDT_Pro_3B architecture (3.85 B parameters, bf16 values; ViT / LLM multiply them as fp16 MFMA operands —
`v_mfma_f32_16x16x32_f16`, the bf16 rate with 3 more mantissa bits; `--operands bf16` is the A/B variant).  Rank 0 prints ONE JSON line.
The timed loops rotate 4 distinct input batches (a repeated batch would sit in the 256 MB Infinity Cache).
A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line, nothing else; the side legs run with --full only
(one GPU; a --no-* flag skips a single leg).
Extra objects on that line (N=1): "roofline" (bf16 MFMA tile-GEMM family: in-kernel start / end stamps of every tile-GEMM call INSIDE the
running pipeline — HIP-event pairs around 290 launches per step cost 10 % throughput and count the dispatch gaps; frac_replay = the same
launches replayed alone between one event pair), "roofline_decode" (HBM bytes of a decode step / its in-situ and stand-alone
duration), "from_images" (the same pipeline fed from uint8 host images), "cpu_baseline" (the fp32 CPU oracle timed on this host, with the
parity read-out), "extra_workloads" (BASELINE configs[3] OVD and configs[4] 7B RIC fp8 per-GPU shapes, short runs), "steady_state" (64 steps of the
same runner), "unmerged_decode" (decode groups of one batch), "single_batch_latency", "to_rle" (the loop ending at COCO RLE records),
"operands_bf16" (the bf16 instantiation, same steps), "reference_precision" (precision="reference": every float output within 1e-3).
The synthetic workload (prompts, pixel rows, scripted schedules, tokenizer stand-in) ships with the package (padt_amd/synthetic.py), so every
leg except `cpu_baseline` runs from an installed package; the CPU baseline needs the source checkout (oracle/ + tests/parity_util.py are test
infrastructure, deliberately not shipped): without them that leg reports itself as skipped.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # multi-process GPU work: the host driver only supports dmabuf IPC (RCCL needs it)
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0      # MI355X dense bf16 (guides/MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0


def alg_tflop_per_image(cfg, L, T, n_obj, n_vrt, grid_hw):
    """ALGORITHMIC work per image, SURVEY.md §8d formulas (3B REC, L=577, T=28, 1 obj x 5 VRT → 6.32: ViT 2.82 + prefill 3.25 +
    decode 0.17 + PaDT decoder 0.07; only the last prompt position goes through the head)."""
    v = cfg.vision_config
    D, Lyr, Hq, Hkv, I, hd = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.intermediate_size, cfg.head_dim
    V = cfg.vocab_size
    P = grid_hw[0] * grid_hw[1]
    N = P // 4
    vh, vi = v.hidden_size, v.intermediate_size
    wp = v.window_size // v.patch_size                                    # patches per window side
    ws = [min(wp, grid_hw[0] - a) * min(wp, grid_hw[1] - b) for a in range(0, grid_hw[0], wp) for b in range(0, grid_hw[1], wp)]
    n_full = len(v.fullatt_block_indexes)
    vit = (2 * P * (v.depth * (3 * vh * vh + vh * vh + 3 * vh * vi) + v.in_channels * v.temporal_patch_size * v.patch_size ** 2 * vh)
           + (v.depth - n_full) * sum(4 * x * x * vh for x in ws) + n_full * 4 * P * P * vh + 2 * N * ((4 * vh) ** 2 + 4 * vh * D))
    per_tok = 2 * Lyr * (2 * D * Hq * hd + 2 * D * Hkv * hd + 3 * D * I)
    prefill = L * per_tok + Lyr * 4 * (L * (L + 1) // 2) * Hq * hd
    head = 2 * (V + N) * D
    decode = sum(per_tok + Lyr * 4 * (L + t) * Hq * hd + head for t in range(1, T))
    dh, di = cfg.vl_decoder["hidden_size"], cfg.vl_decoder["intermediate_size"]
    Q = 3 + n_vrt

    def block(M):
        return 2 * Q * (8 * dh * dh + 2 * dh * di) + 2 * M * 4 * dh * dh + 4 * (Q * Q + 2 * Q * M) * dh
    dec = n_obj * (block(N) + 2 * block(P) + 2 * P * dh * dh + 2 * 4 * P * (dh // 4) * (dh // 4))
    return (vit + prefill + head + decode + dec) / 1e12


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tnew", type=int, default=28)
    ap.add_argument("--model", default="3b", choices=["3b", "7b", "small"])
    ap.add_argument("--task", default="rec", choices=["rec", "ovd", "ric"], help="rec: BASELINE configs[1] (L=577, T=28, 1 object x 5 VRT); "
                    "ovd: BASELINE configs[3] shape per GPU (80-class prompt L=890, T=120, 7 objects x 5 VRT per image); "
                    "ric: BASELINE configs[4] shape (caption with interleaved VRT runs: T=150, 6 runs x 5 VRT)")
    ap.add_argument("--weights", default="bf16", choices=["bf16", "fp8", "fp8+act"], help="fp8: LLM projection weights as OCP e4m3 + power-of-two "
                    "row scales, streamed by the decode steps (BASELINE configs[4], 7B fp8 weight path); fp8+act: additionally the prompt pass as "
                    "fp8 x fp8 MFMA GEMMs over e4m3 activation rows")
    ap.add_argument("--operands", default="auto", choices=["auto", "fp16", "bf16"], help="16-bit MFMA operand type of ViT / LLM (fp32 accumulation, fp32 "
                    "residual streams either way): auto (the product default: fp16 operands — 8x closer to the fp32 reference at the same rate — under "
                    "the device-side range guard, a flagged batch is re-run on bf16), fp16 (same guard, a flagged batch raises) or bf16")
    ap.add_argument("--cap", type=int, default=0, help="object capacity of the per-batch result record (default: 2 x the scheduled objects)")
    ap.add_argument("--full", action="store_true", help="after the timed region, also run every side leg (one GPU): steady state, unmerged decode, "
                    "single-batch latency, rooflines, host-image and RLE legs, bf16 and reference-precision twins, CPU baseline with the parity "
                    "read-out, OVD / 7B RIC workloads; the --no-* flags below skip single legs.  Without it the line carries the headline only")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--merge", type=int, default=0, help="consecutive batches of 8 whose decode steps share one session (in-flight batching; "
                    "1 = every batch decodes alone); default 8 for REC (28 new tokens), 16 for the decode-heavy OVD / RIC shapes (120 / 150 new tokens: "
                    "128-row steps cost 24 %% less per image; same-call OVD 66.1 → 69.3 images/s)")
    ap.add_argument("--no-graph", action="store_true", help="launch decode steps kernel by kernel instead of replaying the captured hipGraph (counter passes)")
    ap.add_argument("--no-alt", action="store_true", help="skip the merge=1 comparison run")
    ap.add_argument("--lane-streams", action="store_true", help="one prefill stream per lane instead of a shared one")
    ap.add_argument("--vit-stream", type=int, default=0, help="1: the ViT of batch b + 1 on its own stream, concurrent with the LLM prefill of batch b")
    ap.add_argument("--timeline", action="store_true", help="print a stream timeline of pipelined steps to stderr")
    ap.add_argument("--timeline-steps", type=int, default=4)
    ap.add_argument("--breakdown", action="store_true", help="also time the phases of one step (printed to stderr)")
    ap.add_argument("--depth", type=int, default=2, help="batches in flight on separate HIP streams (1 = no overlap)")
    ap.add_argument("--no-from-images", dest="from_images", action="store_false", help="skip the leg that feeds the pipeline from uint8 host images")
    ap.add_argument("--no-extras", dest="extras", action="store_false", help="skip the OVD (configs[3]) and 7B RIC fp8 (configs[4]) short runs")
    ap.add_argument("--no-steady", dest="steady", action="store_false", help="skip the 64-step steady-state run of the same runner")
    ap.add_argument("--no-bf16-twin", dest="bf16_twin", action="store_false", help="skip the leg that times the bf16-operand instantiation of the same workload")
    ap.add_argument("--dump-exchange", default="", help="directory: every rank saves its local results and what the all-gathers delivered (tests)")
    ap.add_argument("--dump-outputs", default="", help="directory: rank 0 saves what the last timed step returned (boxes, scores, mask logits, ...) as "
                    "<name>.npy in float32 (float64 for integer fields), at most 64 MB in all, so that two builds can be compared output for output")
    a = ap.parse_args()
    if a.model != "3b" or a.task != "rec" or a.weights != "bf16":
        a.extras = False                                               # the extra keys belong to the headline line only
    if a.merge <= 0:
        a.merge = 8 if a.task == "rec" else 16
    return a


def build_model(args, device):
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    cfg = {"3b": padt_amd.padt_pro_3b, "7b": padt_amd.padt_pro_7b, "small": padt_amd.small_test_config}[args.model]()
    grid_hw = (10, 12) if args.model == "small" else (46, 46)
    model = PaDTForConditionalGeneration.from_synthetic(cfg, seed=0, device=device, llm_weights=args.weights, operands=args.operands)
    args.policy = args.operands                                        # what was asked for ("auto": fp16 under the range guard)
    args.operands = "fp16" if model.dtype == torch.float16 else "bf16"  # what the MFMA pipes multiply: reported as `dtype`
    return cfg, model, grid_hw


def workload(args):
    """→ (n_post text tokens after the image, T_new, objects per image, VRTs per object, schedule)."""
    from padt_amd.synthetic import multi_object_schedule, rec_schedule
    if args.task == "ovd":
        T = args.tnew if args.tnew != 28 else 120
        return 346, T, 7, 5, multi_object_schedule(T, n_obj=7, n_vrt=5)
    if args.task == "ric":
        T = args.tnew if args.tnew != 28 else 150
        return 33, T, 6, 5, multi_object_schedule(T, n_obj=6, n_vrt=5)
    T = args.tnew
    if T >= 17:
        return 33, T, 1, 5, rec_schedule(T, range(11, 16))
    return 33, T, 1, 2, rec_schedule(T, range(2, 4))


N_ROT = 4          # distinct input batches every timed loop cycles through


def make_inputs(cfg, args, grid_hw, device, seed, dtype=torch.float16):
    from padt_amd.synthetic import FakeProcessor, synthetic_batch
    import padt_amd
    n_post, T, n_obj, n_vrt, sched = workload(args)
    args.tnew = T
    grids = [[1, grid_hw[0], grid_hw[1]]] * args.batch
    rot = []
    for k in range(N_ROT):                                             # same shapes, different pixels and prompt ids
        grid, pix, ids, am = synthetic_batch(cfg, grids, n_pre=15, n_post=n_post, seed=seed + 7919 * k)
        rot.append((ids.to(device), am.to(device), pix.to(device).to(dtype)))
    n_m = grid_hw[0] * grid_hw[1] // 4
    proc = padt_amd.VisonTextProcessingClass(FakeProcessor(cfg, n_m), cfg.vision_config.spatial_merge_size)
    proc.model_embed_token_size = cfg.vocab_size
    if not args.cap:
        args.cap = 2 * n_obj * args.batch
    ids, am, pix = rot[0]
    return dict(grid=grid, pix=pix, ids=ids, am=am, proc=proc, rot=rot, rot_k=[0],
                sched=sched, n_obj=n_obj, n_vrt=n_vrt, L=ids.shape[1])


def next_batch(inp):
    """→ (ids (fresh copy: the callers' loop body updates them in place), attention mask, pixel_values) of the next of the N_ROT batches."""
    k = inp["rot_k"][0]
    inp["rot_k"][0] = (k + 1) % len(inp["rot"])
    ids, am, pix = inp["rot"][k]
    return ids.clone(), am, pix


def run_step(model, inp, args, world):
    from padt_amd import pipeline
    ids, am, pix = next_batch(inp)
    decoded, completions, labels, vrts = pipeline.rec_batch(
        model, inp["proc"], ids, am, pix, inp["grid"], max_new_tokens=args.tnew,
        schedule=inp["sched"], sync_every=args.tnew, use_graph=not args.no_graph)
    if world > 1:
        packed = pipeline.pack_results(decoded, cap=args.cap, mask_hw=4 * max(int(inp["grid"][:, 1].max()), int(inp["grid"][:, 2].max())),
                                       device=inp["pix"].device)
        pipeline.all_gather_results(packed)
    return decoded


# ------------------------------------------------------------------------------------------------ roofline legs
def _alg_dims(model, cfg):
    """Undo the zero padding of MLP intermediates: padded size → the model's own."""
    pads = ((model.W.vit_ipad, cfg.vision_config.intermediate_size), (model.W.llm_ipad, cfg.intermediate_size),
            (model.W.dec_ipad, cfg.vl_decoder["intermediate_size"]))

    def alg(n):
        for pad, true in pads:
            if n == pad:
                return true
            if n == 2 * pad:
                return 2 * true
        return n
    return alg


def insitu_leg(model, inp, args, cfg, run_steps, steps):
    """The two rooflines measured IN the running pipeline: `steps` more steps of exactly the timed loop (same runner, same streams, same
    batches in flight) with in-kernel start / end stamps of every tile-GEMM call (ops.GemmProfile: nothing is added to the queues) and a
    HIP-event pair around every chunk of decode-step graph replays on the decode stream.  → (roofline dict for the tile-GEMM family,
    roofline_decode dict)."""
    from padt_amd import ops
    alg = _alg_dims(model, cfg)
    gp, st = ops.GemmProfile(400 * (steps + 2), inp["pix"].device), ops.EventTimer()
    gp.start()
    ops.STEP_TIMER = st
    t0 = time.perf_counter()
    run_steps(steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ops.STEP_TIMER = None
    gp.stop()
    g, d = gp.results(), st.results()
    st.close()
    flops = sum(2.0 * M * alg(N) * alg(K) for _, (kind, M, N, K) in g)
    ms = sum(m for m, _ in g)
    by = {}
    for m, (kind, M, N, K) in g:
        e = by.setdefault((M, N, K, kind), [0, 0.0])
        e[0] += 1
        e[1] += m
    top = sorted(by.items(), key=lambda kv: -kv[1][1])[:6]
    ach = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    roof = {"bound": "mfma", "kernel": "gemm_tile256_kernel + gemm_tile_kernel (%s MFMA 16x16x32 — same rate and peak for fp16 and bf16 —; 256/192/128x256x64 phase-pipelined / 128x128x64 LDS-DMA tiles)" % args.operands,
            "achieved": round(ach, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4),
            "how": "in-kernel wall-clock stamps (first block start → last block end, 100 MHz s_memrealtime) of every tile-GEMM call (rows > 64) of %d pipelined "
                   "steps run right after the timed region with the same runner: algorithmic 2MNK of the un-padded shapes / sum of those durations; the decode "
                   "group of the other stream runs concurrently and takes CUs from the GEMMs (under rocprofv3 the streams are serialised)" % steps,
            "launches_per_step": round(len(g) / max(steps, 1), 1), "avg_launch_us": round(ms * 1e3 / max(len(g), 1), 2),
            "alg_tflop_per_step": round(flops / max(steps, 1) / 1e12, 3), "ms_per_step_in_gemm": round(ms / max(steps, 1), 3),
            "images_per_s_while_instrumented": round(args.batch * steps / wall, 2),
            "top_shapes": [{"M": k[0], "N": k[1], "K": k[2], "kind": k[3], "launches_per_step": round(v[0] / steps, 1),
                            "TFLOP/s": round(2.0 * k[0] * alg(k[1]) * alg(k[2]) * v[0] / (v[1] * 1e-3) / 1e12, 1)} for k, v in top]}
    # ---- decode steps: bytes one step must read (weights of 36 layers + head table + KV of every row) / in-situ duration
    W = model.W
    wbytes = 0
    for i in range(cfg.num_hidden_layers):
        for nm in ("qkv", "o", "gu", "down"):
            t_ = W.get(f"llm.{i}.{nm}.wq") if W.llm_weights == "fp8" else W[f"llm.{i}.{nm}.wp"]
            wbytes += t_.numel() * t_.element_size()
    head = W.get("llm.head.wp", W["llm.head"])
    n_steps = sum(n for _, (n, rows) in d)
    dms = sum(m for m, _ in d)
    rows = max((r for _, (n, r) in d), default=0)
    n_proto = rows * (inp["grid"][0, 1] * inp["grid"][0, 2] // 4).item()
    kv_tok = 2 * cfg.num_key_value_heads * cfg.head_dim * 2 * cfg.num_hidden_layers
    kv_bytes = rows * (inp["L"] + args.tnew / 2.0) * kv_tok
    step_bytes = wbytes + head.numel() * head.element_size() + n_proto * cfg.hidden_size * 2 + kv_bytes
    us = dms * 1e3 / max(n_steps, 1)
    gbs = step_bytes / (us * 1e-6) / 1e9 if us > 0 else 0.0
    dec = {"bound": "hbm", "kernel": "one decode step = one hipGraph replay: %d x [norm+qkv, rope+append+attention over fragment-packed KV caches (ONE launch: block per "
                                     "(kv head, sample), on-chip merge), o+resid, norm+gate/up+SwiGLU, down+resid] (gemm_skinny_kernel, decode_attn_rope_packed_kernel) "
                                     "+ vrt_head_kernel + greedy_step_kernel" % cfg.num_hidden_layers,
           "rows_per_step": rows, "bytes_per_step": int(step_bytes), "weight_bytes_per_step": int(wbytes), "kv_bytes_per_step": int(kv_bytes),
           "us_per_step": round(us, 1), "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
           "steps_timed": n_steps,
           "how": "HIP-event pair around every chunk of graph replays on the decode stream during the same instrumented steps (the prefill of the "
                  "next decode group runs concurrently on the other stream and takes CUs from the step)"}
    return roof, dec


def decode_alone_leg(model, inp, args, cfg, dec):
    """The same decode-step graph with NOTHING else on the GPU: one decode group is prefilled, then all its steps run back to back alone
    (the event bracket opens in stream order, i.e. after the group's last prefill)."""
    from padt_amd import ops
    gids = inp["proc"].assign_to_global_vrt_id(inp["ids"].clone(), inp["grid"])
    for warm in (True, False):                                         # first pass: session allocation + graph capture
        st = ops.EventTimer()
        torch.cuda.synchronize()
        ctx = None
        for k in range(args.merge):
            if k == args.merge - 1:
                torch.cuda.synchronize()                               # the prefills of the other batches are done
                ops.STEP_TIMER = st
            ctx = model.generate_launch(gids, inp["am"], inp["pix"], inp["grid"], args.tnew, False, tuple(inp["sched"]), args.tnew, True, 7,
                                        group=ctx, n_slots=args.merge)
        model.generate_collect(ctx, all_batches=True)
        torch.cuda.synchronize()
        ops.STEP_TIMER = None
        d = st.results()
        st.close()
    n = sum(k for _, (k, r) in d)
    us = sum(m for m, _ in d) * 1e3 / max(n, 1)
    dec["us_per_step_alone"] = round(us, 1)
    dec["achieved_alone"] = round(dec["bytes_per_step"] / (us * 1e-6) / 1e9, 1) if us > 0 else 0.0
    dec["frac_alone"] = round(dec["achieved_alone"] / HBM_PEAK_GBS, 4)
    return dec


def replay_leg(model, inp, args, cfg):
    """The tile-GEMM launches of one step replayed back to back on an otherwise idle GPU (warm, no other kernels in between): the
    family's rate without the pipeline around it → roofline.frac_replay."""
    from padt_amd import _lib, ops
    lib = _lib.load()
    ops.GEMM_LOG = []
    run_step(model, inp, args, 1)
    torch.cuda.synchronize()
    log, ops.GEMM_LOG = ops.GEMM_LOG, None
    alg = _alg_dims(model, cfg)

    def dims(c):
        if c[0] == "hp":
            return c[8], c[2].shape[0], c[2].shape[1] // 2
        if c[0] == "r32":
            return c[1].shape[0], c[2].shape[0], c[1].shape[1]
        return c[0].shape[0], c[1].shape[0], (c[7] if c[7] is not None else c[0].shape[1])
    tile = [c for c in log if dims(c)[0] > 64]
    flops = sum(2.0 * M * alg(N) * alg(K) for M, N, K in map(dims, tile))
    alg_bytes = 0.0
    for c in tile:
        M, N, K = dims(c)
        n_, k_ = alg(N), alg(K)
        if c[0] == "hp":
            alg_bytes += 4.0 * M * k_ + 2.0 * n_ * k_ + 4.0 * M * n_ * (2 if c[6] is not None else 1)
        elif c[0] == "r32":
            alg_bytes += 2.0 * (M * k_ + n_ * k_) + (8.0 + (2.0 if c[5] is not None else 0.0)) * M * n_
        else:
            n_out = n_ // (2 if c[4] == 3 else 1)
            alg_bytes += 2.0 * (M * k_ + n_ * k_) + (4.0 if c[6] else 2.0) * M * n_out + (2.0 * M * n_out if c[5] is not None else 0.0)

    def replay():
        for c in tile:
            if c[0] == "r32":
                ops.gemm_resid32(c[1], c[2], c[3], c[4], c[5])
            elif c[0] == "hp":
                ops.gemm_hp(c[1], c[2], c[3], out=c[4], epilogue=c[5], residual=c[6], out_mode=c[7], M=c[8])
            else:
                (a, w, bias, out, epi, res, f32, K, rs) = c
                ops.gemm(a, w, bias, out=out, epilogue=epi, residual=res, out_f32=f32, K=K, row_scale=rs)
    replay()
    torch.cuda.synchronize()
    t = ops.EventTimer()
    tot = 0.0
    reps = 3
    for _ in range(reps):
        ev = t.begin()
        replay()
        t.end(ev, None)
        tot += t.results()[0][0]
    t.close()
    ms = tot / reps
    ach = flops / (ms * 1e-3) / 1e12
    # HBM-side bytes per launch of the same launches from rocprofv3 PMC passes (FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE): collected
    # separately (tools/collect_profiles.sh), committed under profiles/, and only quoted for the workload / launch count they were measured on
    import glob
    pdir = os.path.join(ROOT, "profiles")
    traffic, traffic_src, traffic_note = None, None, "no committed PMC measurement for this workload"
    sha = csrc_sha16()
    for tp in sorted(glob.glob(os.path.join(pdir, "r*_pmc_traffic.json")), reverse=True):
        tj = json.load(open(tp))
        wl = tj.get("workload", {})
        if wl.get("model") == args.model and wl.get("batch") == args.batch and wl.get("tnew") == args.tnew and wl.get("task", "rec") == args.task \
                and tj.get("gemm_calls", tj.get("launches")) == len(tile):
            # quoted only while it describes the kernels that ran: the measurement is stamped with the hash of csrc/ it was taken on
            if tj.get("csrc_sha16") == sha and wl.get("operands", "bf16") == args.operands:
                traffic, traffic_src, traffic_note = tj["traffic_bytes_per_launch"], "profiles/" + os.path.basename(tp), "csrc/ unchanged since the PMC passes"
            else:
                traffic_note = "profiles/%s was measured on other kernel sources (csrc sha %s, now %s): not quoted" % (os.path.basename(tp), tj.get("csrc_sha16"), sha)
            break
    return {"achieved_replay": round(ach, 1), "frac_replay": round(ach / MFMA_BF16_PEAK_TFLOPS, 4), "ms_per_step_replayed": round(ms, 3),
            "launches_replayed": len(tile), "alg_bytes_per_launch": round(alg_bytes / max(len(tile), 1), 0), "traffic": traffic,
            "traffic_unit": "bytes per launch", "traffic_source": traffic_src, "traffic_note": traffic_note}


# ------------------------------------------------------------------------------------------------ CPU baseline leg
def hip_sample0(model, inp, args):
    """The HIP path's own answer for the first batch of the workload, sample 0 kept: completion tokens, boxes, score logits and mask logits (valid
    region) — what the oracle run of cpu_baseline_leg is compared with (the timed mode AND precision="reference" go through this)."""
    from padt_amd.processor import parseVRTintoCompletion
    L = inp["ids"].shape[1]
    gids = inp["proc"].assign_to_global_vrt_id(inp["ids"].clone(), inp["grid"])
    hout = model.generate(input_ids=gids, attention_mask=inp["am"], pixel_values=inp["pix"], image_grid_thw=inp["grid"], use_cache=True,
                          max_new_tokens=args.tnew, do_sample=False, output_hidden_states=True, return_dict_in_generate=True, schedule=inp["sched"])
    hseq = hout["sequences"].cpu()
    hloc = inp["proc"].assign_to_local_vrt_id(hseq.clone(), inp["grid"].cpu())
    _, hfeats, _, _, _ = parseVRTintoCompletion(inp["proc"], hloc[:, L:], hout["hidden_states"], torch.Tensor([False] * hseq.shape[0]))
    hdec = model.vl_decode(hfeats, hout.past_image_embeds, hout.past_high_res_image_embeds, inp["grid"], hout.past_visual_pe)
    sel = [i for i, si in enumerate(hdec["sample_idx"]) if int(si) == 0]
    hw = hdec["pred_mask_valid_hw"]
    masks = [hdec["pred_mask"][i, : int(hw[0][i]), : int(hw[1][i])].float().cpu() for i in sel] if hdec.get("pred_mask") is not None and len(hw) else []
    return {"tokens": hseq[:1, L:], "boxes": [hdec["pred_boxes"][i].float().cpu().tolist() for i in sel],
            "scores": [float(hdec["pred_score"][i].float().cpu().reshape(-1)[0]) for i in sel], "masks": masks}


REFERENCE_SAMPLE0 = None     # reference_precision_leg leaves its hip_sample0() here for cpu_baseline_leg's parity read-out of that mode


def parity_readout(hip, ores, odec, n_tok, side=(640, 640)):
    """tokens / box IoU / |d box| / |d score logit| / mask-logit distance (max |d| over the valid region ÷ the oracle's logit range) of one
    HIP answer (hip_sample0) against the oracle run of the same sample — north_star: ids bit-exact, boxes and mask logits within 1e-3."""
    from padt_amd.postprocess import box_iou_xywh, box_to_pixels
    hip_tok = hip["tokens"]
    n_steps = min(len(ores["logits"]), hip_tok.shape[1], n_tok)
    same = sum(int(torch.argmax(ores["logits"][t][0]).item() == int(hip_tok[0, t])) for t in range(n_steps))
    oboxes = odec["pred_boxes"].float().tolist()
    ious = [round(box_iou_xywh(box_to_pixels(hb, side[1], side[0]), box_to_pixels(ob, side[1], side[0])), 4) for hb, ob in zip(hip["boxes"], oboxes)]
    out = {"tokens_equal_oracle_argmax": "%d/%d" % (same, n_steps), "box_iou_vs_oracle": ious,
           "box_abs_diff_max": round(max((abs(a - b) for hb, ob in zip(hip["boxes"], oboxes) for a, b in zip(hb, ob)), default=0.0), 6)}
    osc = odec["pred_score"].float().reshape(-1).tolist()
    out["score_abs_max"] = round(max((abs(a - b) for a, b in zip(hip["scores"], osc)), default=0.0), 6)
    om, ohw = odec.get("pred_mask"), odec.get("pred_mask_valid_hw")
    if om is not None and hip["masks"]:
        rel = []
        for i, hm in enumerate(hip["masks"]):
            o = om[i, : int(ohw[0][i]), : int(ohw[1][i])].float()
            rel.append(((hm - o).abs().max() / (o.max() - o.min())).item() if hm.shape == o.shape else float("nan"))
        out["mask_logits_rel_max"] = float("%.3e" % max(rel))
    return out


def cpu_baseline_leg(cfg, args, inp, model):
    """The fp32 CPU oracle (kind "port": the reference is Python and cannot travel to the GPU box) actually RUN on a bounded sample of
    the same workload: ONE image of the batch, same prompt, same scripted schedule, same random-init architecture — generate()
    (ViT + prototypes + prefill + T-1 decode steps over the 152k + 529 table) + parse + vl_decode, timed end to end.  ≈25-40 s."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import padt_oracle as O
    import parity_util as U
    from padt_amd.weights import synthetic_state_dict
    oc = U.oracle_config(cfg)
    ncpu = os.cpu_count() or 1
    # FIXED thread count (round 5): 32 is the measured best of 32 … 192 on the GPU box's 256-core host for the oracle's many mid-sized ops
    # (tools/bench_oracle_threads.py, profiles/r04 log); a calibrated count made the baseline wander from round to round (32 vs 64)
    cores = min(32, ncpu)
    torch.set_num_threads(cores)
    # random-init weights of the architecture, generated on the GPU and copied (15 GB of fp32 on the host for 3B)
    sd = synthetic_state_dict(cfg, seed=0, device=inp["pix"].device, dtype=torch.bfloat16)
    w = {k: v.float().cpu() for k, v in sd.items()}
    del sd
    P = int(inp["grid"][0, 1] * inp["grid"][0, 2])
    ids, am = inp["ids"][:1].cpu(), inp["am"][:1].cpu()
    pix, grid = inp["pix"][:P].float().cpu(), inp["grid"][:1]
    T, sched = args.tnew, inp["sched"]
    # the HIP path's own tokens / boxes / score / mask logits for the same image (sample 0 of the batch: its global VRT ids are its local ones),
    # so that the timed oracle run doubles as the parity check of the metric's "box IoU vs ref": the oracle is TEACHER-FORCED on the HIP tokens
    # (same work per step as free running — it still computes every logit row; only the appended token is overridden)
    hip = hip_sample0(model, inp, args)
    hip_tok = hip["tokens"]
    with torch.no_grad():
        t0 = time.perf_counter()
        ores = O.generate(w, oc, ids, am, pix, grid, T, schedule=sched, force_tokens=hip_tok, collect_logits=True)
        t_gen = time.perf_counter() - t0
        st = ores["state"]
        runs, cur = [], []
        for t, m in enumerate(sched):                                  # VRT runs of the schedule = the objects the parser would find
            if m == "v":
                cur.append(t)
            elif cur:
                runs.append(cur)
                cur = []
        feats = [[torch.cat([ores["hidden"][t][0:1, -1] for t in r], 0) for r in runs]]
        t1 = time.perf_counter()
        odec = O.vl_decode(w, oc, feats, st.proto, st.high_res, grid, st.visual_pe)
        t_dec = time.perf_counter() - t1
    t_img = t_gen + t_dec
    # parity read-out of the same run: how many HIP tokens are the oracle's own (scheduled) arg-max, the IoU of the boxes (xywh pixel boxes as
    # utils.py:258-260 derives them, IoU as eval_refcoco.py:15-41), |d box|, |d score logit| and the mask-logit distance (the mask head is ON in
    # the timed workload: padt_decoder.py:241-274) — for the timed mode and, when that leg ran, for precision="reference" on the same sample
    parity = parity_readout(hip, ores, odec, hip_tok.shape[1])
    parity["mode"] = "timed mode: %s MFMA operands (operands=%r), fp32 residual streams, split-precision PaDT decoder" % (args.operands, getattr(args, "policy", args.operands))
    parity["note"] = "sample 0 of the batch, oracle teacher-forced on the HIP tokens (HIP path vs fp32 CPU oracle, random-init weights); mask_logits_rel_max = max |d| over the valid region / the oracle's logit range"
    if REFERENCE_SAMPLE0 is not None:
        rp = parity_readout(REFERENCE_SAMPLE0, ores, odec, hip_tok.shape[1])
        rp["tokens_equal_timed_mode"] = bool(torch.equal(REFERENCE_SAMPLE0["tokens"], hip_tok))
        rp["mode"] = "precision='reference' (the mode that keeps north_star's 1e-3 on every float output), same sample, same oracle run"
        parity["reference_precision"] = rp
    return {"value": round(1.0 / t_img, 5), "unit": "images/s", "cores": cores, "kind": "port", "parity": parity,
            "sample": "1 image of the workload (L=%d, T_new=%d, %d object(s) x %d VRT), fp32 CPU oracle run end to end: generate %.2f s "
                      "(ViT + prefill + %d decode steps) + vl_decode %.2f s = %.2f s/image on %d threads of %d host cores"
                      % (ids.shape[1], T, len(runs), len(runs[0]) if runs else 0, t_gen, T - 1, t_dec, t_img, cores, ncpu)}


def short_run(model, inp, args, steps):
    """images/s of `steps` batches through a fresh pipelined runner of the same shape as the headline's (priming pass untimed)."""
    from padt_amd import pipeline
    r = pipeline.PipelinedRunner(model, inp["proc"], depth=args.depth, merge=args.merge)

    def go(k):
        for _ in range(k):
            ids, am, pix = next_batch(inp)
            r.submit(ids, am, pix, inp["grid"], max_new_tokens=args.tnew, schedule=inp["sched"])
        r.flush()
    go(args.depth * args.merge)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    go(steps)
    torch.cuda.synchronize()
    e = time.perf_counter() - t0
    return {"value": round(args.batch * steps / e, 3), "unit": "images/s", "steps": steps, "ms_per_step": round(e / steps * 1e3, 3)}


def bf16_twin_leg(cfg, args, grid_hw, device):
    """The SAME workload on the bf16-operand instantiation of the library (what BASELINE.json's configs[1] literally names, and what an
    operands="auto" model re-runs a flagged batch on): its own weights / inputs / runner, the headline's --steps / --warmup, and the in-situ
    tile-GEMM fraction of that run — driver-timed next to the fp16 headline."""
    import copy
    from padt_amd import pipeline
    from padt_amd.modeling import PaDTForConditionalGeneration
    a = copy.copy(args)
    a.cap = 0
    m2 = PaDTForConditionalGeneration.from_synthetic(cfg, seed=0, device=device, llm_weights=a.weights, operands="bf16")
    inp2 = make_inputs(cfg, a, grid_hw, device, seed=1234, dtype=torch.bfloat16)
    r2 = pipeline.PipelinedRunner(m2, inp2["proc"], depth=a.depth, merge=a.merge)

    def rs(k):
        for _ in range(k):
            ids, am, pix = next_batch(inp2)
            r2.submit(ids, am, pix, inp2["grid"], max_new_tokens=a.tnew, schedule=inp2["sched"])
        r2.flush()
    rs(a.depth * a.merge)
    rs(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rs(a.steps)
    torch.cuda.synchronize()
    e = time.perf_counter() - t0
    out = {"value": round(a.batch * a.steps / e, 3), "unit": "images/s", "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(e / a.steps * 1e3, 3),
           "dtype": "bf16", "note": "operands='bf16': v_mfma_f32_16x16x32_bf16 over bf16 activations / KV caches / weight images, fp32 residual streams; same "
                                    "runner shape, steps and warmup as the headline"}
    a.operands = "bf16"
    roof, dec = insitu_leg(m2, inp2, a, cfg, rs, min(a.steps, 16))
    out["roofline_frac_in_situ"] = roof["frac"]
    out["roofline_achieved"] = roof["achieved"]
    out["decode_us_per_step_in_situ"] = dec["us_per_step"]
    del r2, m2, inp2
    torch.cuda.empty_cache()
    return out


def reference_precision_leg(cfg, args, grid_hw, device):
    """The SAME workload with precision="reference" (padt_amd/reference.py: ViT / LLM on (hi, lo) bf16 GEMM operands at twice the MFMA work,
    exact-fp32 attention on the f32-input MFMA incl. an fp32 KV cache, captured decode steps whose projections read each weight once, the SwiGLU as the
    gate/up GEMM's epilogue): the mode that meets the north star's 1e-3 on EVERY
    float output, mask logits included (tests/test_reference_mode_gpu.py: full-depth 3B boxes 1.8e-6 / mask logits 2.7e-5, tokens equal) — its
    price next to the headline, same runner shape (depth x merge) as the headline."""
    import copy
    from padt_amd import pipeline
    from padt_amd.modeling import PaDTForConditionalGeneration
    a = copy.copy(args)
    a.cap = 0
    m2 = PaDTForConditionalGeneration.from_synthetic(cfg, seed=0, device=device, llm_weights="bf16", operands="fp16", precision="reference")
    inp2 = make_inputs(cfg, a, grid_hw, device, seed=1234, dtype=torch.float16)
    r2 = pipeline.PipelinedRunner(m2, inp2["proc"], depth=a.depth, merge=a.merge)

    def rs(k):
        for _ in range(k):
            ids, am, pix = next_batch(inp2)
            r2.submit(ids, am, pix, inp2["grid"], max_new_tokens=a.tnew, schedule=inp2["sched"])
        r2.flush()
    rs(a.depth * a.merge)                                              # priming: every lane allocates its session and captures its decode graph
    torch.cuda.synchronize()
    steps = 2 * a.merge
    t0 = time.perf_counter()
    rs(steps)
    torch.cuda.synchronize()
    e = time.perf_counter() - t0
    global REFERENCE_SAMPLE0
    REFERENCE_SAMPLE0 = hip_sample0(m2, inp2, a)                       # same first batch as the headline's (seed 1234): cpu_baseline_leg compares it with the oracle
    del r2, m2, inp2
    torch.cuda.empty_cache()
    return {"value": round(a.batch * steps / e, 3), "unit": "images/s", "steps": steps, "ms_per_step": round(e / steps * 1e3, 3),
            "note": "precision='reference': split-precision (hi, lo) bf16 GEMM operands through ViT / merger / prototypes / LLM (2x the MFMA work), exact-fp32 "
                    "attention on the f32-input MFMA (v_mfma_f32_16x16x4_f32: ViT windows / full layers, causal GQA prompt pass, decode steps over an fp32 KV "
                    "cache), hipGraph-captured decode steps in groups of %d batches whose projections read every weight once (padt_gemm_split_rows), SwiGLU fused into the "
                    "gate/up GEMM epilogue (round 5: VALU attention, eager steps, groups of 2: 24.3 images/s); parity of "
                    "THIS run's first batch against the oracle: cpu_baseline.parity.reference_precision; full-depth suites: tests/test_reference_mode_gpu.py" % a.merge}


def extra_workloads(args, device, model3b, cfg3b, grid3b):
    """BASELINE configs[3] and [4] per-GPU shapes, driver-timed as extra keys of the one JSON line (short runs, no side legs).  The OVD run
    uses the headline's own PaDT_Pro_3B weights; the 7B model is built (random init, fp8 e4m3 decode weights) after the 3B one is released."""
    import copy
    out = {}
    for key, over in (("ovd_3b", dict(model="3b", task="ovd", weights="bf16", tnew=28)),
                      ("ric_7b_fp8", dict(model="7b", task="ric", weights="fp8", tnew=28)),             # fp8 weights, 16-bit activations: keeps the 1e-3 parity
                      ("ric_7b_fp8_act", dict(model="7b", task="ric", weights="fp8+act", tnew=28))):    # + e4m3 activation rows in the prompt pass: faster, costs precision
        a = copy.copy(args)
        for k, v in over.items():
            setattr(a, k, v)
        a.cap = 0
        a.operands = getattr(args, "policy", a.operands)               # the asked-for policy ("auto"), not the resolved operand type
        a.merge = 16                                                   # decode-heavy shapes: 128-row decode steps (see --merge)
        if key == "ovd_3b":
            cfg, model, grid_hw = cfg3b, model3b, grid3b
            model3b = None
        else:
            cfg, model, grid_hw = build_model(a, device)
        inp = make_inputs(cfg, a, grid_hw, device, seed=4321, dtype=model.dtype)
        steps = 48                                                     # three decode groups of 16 batches after the priming pass
        r = short_run(model, inp, a, steps)
        alg = alg_tflop_per_image(cfg, inp["L"], a.tnew, inp["n_obj"], inp["n_vrt"], grid_hw)
        r.update({"workload": "%s %s, batch=%d/GPU, L=%d, T_new=%d, %d obj x %d VRT per image, %s LLM weights%s" % (
            {"3b": "PaDT_Pro_3B", "7b": "PaDT_Pro_7B (untied head)"}[a.model], a.task.upper(), a.batch, inp["L"], a.tnew, inp["n_obj"], inp["n_vrt"], a.weights,
            {"fp8": " (fp8 e4m3 weight streaming in the decode steps; the prompt pass multiplies the exactly dequantised 16-bit image: 16-bit ACTIVATIONS "
                    "throughout — the variant that keeps the north star's parity: full 28-layer depth boxes 3.8e-4, tests/test_real_shape_gpu.py::test_7b_full_depth_single_image_against_oracle)",
             "fp8+act": " (fp8 x fp8 MFMA prompt pass over e4m3 ACTIVATION rows + fp8 weight streaming in the decode steps: e4m3 activations cost "
                        "precision — at full 28-layer depth boxes 2.4-3.0e-3 (IoU 0.99), mask logits 5e-2 of their range, hidden rows 0.30 rel rms "
                        "against the oracle quantising the same rows, tokens unchanged: tests/test_real_shape_gpu.py::test_7b_full_depth_single_image_against_oracle — "
                        "the 1e-3 parity bar is met by the 16-bit-activation paths only: same model with 16-bit activations 3.9e-4 / 4.2e-3)"}.get(a.weights, "")),
            "alg_tflop_per_image": round(alg, 3), "mfma_frac_e2e": round(r["value"] * alg / MFMA_BF16_PEAK_TFLOPS, 4)})
        out[key] = r
        del model, inp
        torch.cuda.empty_cache()
    return out


def from_images_leg(model, inp, args, grid_hw, steps):
    """The headline pipeline fed from HOST images: 8 uint8 640x640x3 images in pinned memory per batch → H2D → bicubic resize to 644x644
    (Pillow's resampler on the device, byte-exact) → normalize + patchify → the same runner.  f2 of SURVEY.md §8f timed in the loop."""
    from padt_amd import pipeline
    from padt_amd.preprocess import ImageFrontEnd
    fe = ImageFrontEnd(inp["pix"].device, dtype=model.dtype)
    g = torch.Generator().manual_seed(99)
    hh, ww = grid_hw[0] * 14 - 4, grid_hw[1] * 14 - 4                  # 640 x 640 for the 46 x 46 grid: smart_resize brings it to 644 x 644
    hosts = [[torch.randint(0, 256, (hh, ww, 3), dtype=torch.uint8, generator=g).pin_memory() for _ in range(args.batch)] for _ in range(N_ROT)]
    pix, grid = fe(hosts[0])
    assert pix.shape == inp["pix"].shape and grid.tolist() == inp["grid"].tolist(), (pix.shape, grid.tolist())
    r = pipeline.PipelinedRunner(model, inp["proc"], depth=args.depth, merge=args.merge)
    n_sub = [0]

    def go(k):
        for _ in range(k):
            pv, gr = fe(hosts[n_sub[0] % N_ROT])
            n_sub[0] += 1
            ids, am, _ = next_batch(inp)
            r.submit(ids, am, pv, gr, max_new_tokens=args.tnew, schedule=inp["sched"])
        r.flush()
    go(args.depth * args.merge)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    go(steps)
    torch.cuda.synchronize()
    e = time.perf_counter() - t0
    return {"value": round(args.batch * steps / e, 3), "unit": "images/s", "steps": steps, "ms_per_step": round(e / steps * 1e3, 3),
            "host_bytes_per_image": hh * ww * 3,
            "note": "timed region starts at uint8 HWC images in pinned host memory: H2D + GPU resize + normalize + patchify inside the loop"}


def to_rle_leg(model, inp, args, steps):
    """The headline pipeline with the timed region ending where the reference's eval loop ends (utils.py:252-266): score sigmoid, pixel
    boxes, mask up-sampling to the 640 x 640 image + sigmoid > 0.5 on the device (padt_mask_upsample_binarize), COCO RLE on the host —
    f1 of SURVEY.md §8f timed in the loop."""
    from padt_amd import pipeline, postprocess
    r = pipeline.PipelinedRunner(model, inp["proc"], depth=args.depth, merge=args.merge)
    sizes = [(640, 640)] * args.batch
    n_rec = [0]
    post_stream = torch.cuda.Stream(device=inp["pix"].device, priority=-1)    # the records' small kernels + copies: not behind the caller's stream

    def post(done):
        for decoded, completions, labels, vrts in done:
            with torch.cuda.stream(post_stream):                       # (the runner synchronised the lane's decode stream before returning `decoded`)
                n_rec[0] += len(postprocess.postprocess_results(decoded, labels, sizes, want_mask=False))   # the loop's end state is the RLE (utils.py:263-265)

    def go(k):
        for _ in range(k):
            ids, am, pix = next_batch(inp)
            post(r.submit(ids, am, pix, inp["grid"], max_new_tokens=args.tnew, schedule=inp["sched"]))
        post(r.flush())
    go(args.depth * args.merge)
    n_rec[0] = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    go(steps)
    torch.cuda.synchronize()
    e = time.perf_counter() - t0
    return {"value": round(args.batch * steps / e, 3), "unit": "images/s", "steps": steps, "ms_per_step": round(e / steps * 1e3, 3),
            "records": n_rec[0],
            "note": "timed region ends at the eval loop's records: xywh pixel boxes, scores, 640 x 640 masks binarised AND run-length encoded on the device "
                    "(padt_mask_upsample_binarize + padt_mask_rle: only the COCO counts strings cross PCIe)"}


DUMP_LIMIT_BYTES = 60 << 20      # 62.9 MB of array data: with the .npy headers the files stay under 64 MB


def dump_outputs(decoded, out_dir, limit=DUMP_LIMIT_BYTES):
    """What a caller of the timed path receives for one batch (vl_decode's dict) → out_dir/<name>.npy: floating fields as float32, integer
    and bool fields as float64 (exact).  Tuples of per-object tensors become <name>_<i>.npy.  Should the files exceed `limit` bytes, every
    array is cut to the same fixed, seeded sample of its flattened elements (sorted indices, numpy seed 0) so that they fit."""
    import numpy as np
    arrays = {}
    for k, v in decoded.items():
        items = [(k, v)] if not isinstance(v, (tuple, list)) or not v or not isinstance(v[0], torch.Tensor) else [(f"{k}_{i}", t) for i, t in enumerate(v)]
        for name, t in items:
            t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(t)
            fp = t.is_floating_point()
            arrays[name] = t.to(torch.float32 if fp else torch.float64).numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > limit:
        keep = limit / total
        for name, a in arrays.items():
            n = max(1, int(a.size * keep))
            if n < a.size:
                idx = np.sort(np.random.default_rng(0).choice(a.size, n, replace=False))
                arrays[name] = a.reshape(-1)[idx]
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


def csrc_sha16():
    """sha256 (first 16 hex digits) over the kernel sources: what a committed PMC measurement was taken on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "padt_amd", "csrc")
    for f in sorted(os.listdir(d)):
        h.update(f.encode())
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as typed: run `python -m torch.distributed.run --nproc-per-node N bench.py ...` (one rank per GPU;
        # 127.0.0.1 rendezvous — the container hostname may not resolve; torchrun's own chatter goes to stderr, rank 0's line to stdout)
        import socket
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.stdout.flush()
        import ctypes
        import signal
        import subprocess

        def die_with_parent():                                         # the launcher (and through it every rank) ends when this process is killed
            ctypes.CDLL(None, use_errno=True).prctl(1, signal.SIGTERM)    # PR_SET_PDEATHSIG
        sys.exit(subprocess.call(cmd, preexec_fn=die_with_parent))     # a child process, not exec: this one stays the launcher's parent
    if args.gpus != world:
        print(f"bench.py --gpus {args.gpus} under a launcher with WORLD_SIZE={world}: the two must agree", file=sys.stderr)
        sys.exit(2)
    # The contract is ONE JSON line on stdout.  Native libraries write banners to file descriptor 1 behind Python's back (RCCL's version
    # block, gloo's "connected to N peer ranks"): keep a private handle on the real stdout for the line and point fd 1 at stderr.
    sys.stdout.flush()
    line_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    # PADT_DIST_FORCE=1: run the data-parallel code path (process group, device-side pack, asynchronous all-gather per decode group) at
    # world size 1 too — on a one-GPU box that is the one way to put the exchange on RCCL itself (RCCL refuses two ranks per device)
    dist_on = world > 1 or os.environ.get("PADT_DIST_FORCE") == "1"
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        # PADT_DIST_BACKEND=gloo lets the multi-rank path be exercised on a single-GPU box (ranks share device 0); the
        # driver's runs use the default: nccl = RCCL over xGMI, one GPU per rank
        backend = os.environ.get("PADT_DIST_BACKEND", "nccl")
        local = local % torch.cuda.device_count()
        torch.cuda.set_device(local)                                   # one GPU per rank: every allocation / stream / graph below lives on cuda:<LOCAL_RANK>
        # ... and the host cores of that GPU's NUMA node (8 ranks x an enqueue thread of ~7 ms per batch + the parser): real multi-GPU runs only
        # (PADT_PIN=0 / 1 overrides); ranks that share one GPU under gloo keep the whole machine
        pin = os.environ.get("PADT_PIN", "1" if (world > 1 and backend == "nccl") else "0") == "1"
        from padt_amd.pipeline import pin_rank_to_local_cores
        affinity = pin_rank_to_local_cores(local, int(os.environ.get("LOCAL_WORLD_SIZE", world))) if pin else {"skipped": "not a multi-GPU RCCL run"}
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"), rank=rank, world_size=world)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    device = f"cuda:{local}" if dist_on else "cuda:0"
    cfg, model, grid_hw = build_model(args, device)
    inp = make_inputs(cfg, args, grid_hw, device, seed=1234 + rank, dtype=model.dtype)

    def barrier():
        torch.cuda.synchronize()
        if dist_on:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    from padt_amd import pipeline
    runner = (pipeline.PipelinedRunner(model, inp["proc"], depth=args.depth, merge=args.merge, shared_prefill_stream=not args.lane_streams,
                                       use_graph=not args.no_graph, vit_stream=bool(args.vit_stream))
              if (args.depth > 1 or args.merge > 1) else None)
    # data-parallel exchange (world > 1): device-side pack of every batch's record, ONE asynchronous all-gather per decode group
    exchange = None
    gathered = []
    if dist_on:
        mask_hw = 4 * max(int(inp["grid"][:, 1].max()), int(inp["grid"][:, 2].max()))
        exchange = pipeline.ResultExchange(args.cap, mask_hw, per_gather=args.merge, device=device)
    dump = [] if args.dump_exchange else None

    def deliver(decoded):
        if dump is not None:
            dump.append({k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in decoded.items() if k in ("pred_boxes", "pred_score", "pred_mask", "sample_idx")})
        if exchange is not None:
            got = exchange.add(decoded)                                # views of the exchange's double buffer: consume (here: copy for the dump) now
            gathered.extend([t.clone() for t in got] if dump is not None else got)

    def run_steps(k, runner=runner):
        """k steps = k batches through the whole path; with depth > 1 consecutive batches overlap on separate streams
        (every batch is complete — results on the host side of vl_decode, exchange issued — before this returns)."""
        last = None
        if k <= 0:
            return last
        if runner is None:
            for _ in range(k):
                last = run_step(model, inp, args, 1)
                deliver(last)
        else:
            for _ in range(k):
                ids_k, am_k, pix_k = next_batch(inp)
                for r in runner.submit(ids_k, am_k, pix_k, inp["grid"], max_new_tokens=args.tnew, schedule=inp["sched"]):
                    last = r[0]
                    deliver(last)
            for r in runner.flush():
                last = r[0]
                deliver(last)
        if exchange is not None:
            got = exchange.flush()                                     # the run's last (possibly partial) group: waited for inside the timed region
            gathered.extend([t.clone() for t in got] if dump is not None else got)
        return last

    if runner is not None:
        run_steps(args.depth * args.merge)      # one-time: every lane allocates its session and captures its decode graph
    run_steps(args.warmup)
    if dump is not None:
        dump.clear()
    gathered.clear()
    barrier()
    t0 = time.perf_counter()
    decoded = run_steps(args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    if dist_on:
        import torch.distributed as dist
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    assert decoded["pred_boxes"].shape == (args.batch * inp["n_obj"], 4) and torch.isfinite(decoded["pred_boxes"]).all()
    if args.dump_exchange:                                             # tests: what this rank computed and what it received from everybody
        os.makedirs(args.dump_exchange, exist_ok=True)
        torch.save({"local": dump, "gathered": [g.records.cpu() for g in gathered], "cap": args.cap, "batch": args.batch,      # plain tensors: torch.load(weights_only)
                    "continuation": [None if g.continuation is None else g.continuation.cpu() for g in gathered]},
                   os.path.join(args.dump_exchange, f"rank{rank}.pt"))

    if args.dump_outputs and rank == 0:                                # the timed path's last step, before any side leg runs
        dump_outputs(decoded, args.dump_outputs)

    full = args.full and not dist_on and rank == 0                     # side legs: --full, one GPU
    side = full and not args.no_alt
    # the same runner over 64 steps (8 decode groups): what the pipeline does once the fill / drain of the driver's 20-step window
    # (2.5 groups: the last group's decode runs with nothing to overlap) is amortised
    steady = None
    if full and runner is not None and args.steady:
        if args.steps >= 64:
            steady = {"value": round(args.batch * args.steps / elapsed, 3), "unit": "images/s", "steps": args.steps, "note": "the timed region itself"}
        else:
            barrier()
            ts = time.perf_counter()
            run_steps(64)
            barrier()
            es = time.perf_counter() - ts
            steady = {"value": round(args.batch * 64 / es, 3), "unit": "images/s", "steps": 64, "ms_per_step": round(es / 64 * 1e3, 3),
                      "note": "same runner, same inputs, 64 steps (8 decode groups) timed right after the headline's region"}
    # same workload with every batch decoding alone (merge = 1, two batches in flight), for comparison in the same run
    alt = None
    if side and runner is not None and args.merge > 1:
        r1 = pipeline.PipelinedRunner(model, inp["proc"], depth=2, merge=1)
        run_steps(3, r1)
        barrier()
        k1 = min(args.steps, 12)
        t1 = time.perf_counter()
        run_steps(k1, r1)
        barrier()
        e1 = time.perf_counter() - t1
        alt = {"value": round(args.batch * k1 / e1, 3), "unit": "images/s", "steps": k1, "ms_per_step": round(e1 / k1 * 1e3, 3),
               "note": "decode groups of ONE batch (8 rows per decode step), 2 batches in flight"}
        del r1
    # latency of ONE batch running alone (depth 1, merge 1: no other batch in flight), same workload
    lat = None
    if side:
        for _ in range(2):
            run_step(model, inp, args, 1)
        torch.cuda.synchronize()
        tl = time.perf_counter()
        kl = 4
        for _ in range(kl):
            run_step(model, inp, args, 1)
        torch.cuda.synchronize()
        el = (time.perf_counter() - tl) / kl
        lat = {"ms_per_batch": round(el * 1e3, 3), "images_per_s": round(args.batch / el, 3),
               "note": "one batch alone on the GPU (depth 1, merge 1): ViT + prefill + decode at 8 rows per step + parse + PaDT decoder back to back; "
                       "GPU-bound (host enqueue time of the whole batch ≈ 7 ms, tools/latency_breakdown.py)"}

    if args.timeline and runner is not None and rank == 0:
        # stream timeline of a few pipelined steps (events on the prefill / per-lane decode streams), ms from the first mark
        runner.trace = []
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        run_steps(args.timeline_steps)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) * 1e3
        base = runner.trace[0][2]
        marks = sorted(((base.elapsed_time(e), b, tag) for b, tag, e in runner.trace))
        b0 = runner.trace[0][0]
        print(f"[timeline] {args.timeline_steps} steps, wall {wall:.1f} ms", file=sys.stderr)
        for t, b, tag in marks:
            print(f"[timeline] {t:8.2f} ms  batch {b - b0}  {tag}", file=sys.stderr)
        runner.trace = None

    if rank == 0:
        n_img = args.batch * args.steps * world
        value = n_img / elapsed
        alg_tf = alg_tflop_per_image(cfg, inp["L"], args.tnew, inp["n_obj"], inp["n_vrt"], grid_hw)
        ops_txt = ("fp16 MFMA operands (v_mfma_f32_16x16x32_f16: the bf16 rate, 3 more mantissa bits; bf16 checkpoint values)" if args.operands == "fp16"
                   else "bf16 MFMA operands")
        fmt = ("%s, batch=%d/GPU 640x640 synthetic (grid %dx%d, L=%d, T_new=%d, %d obj x %d VRT per image, mask head on), " + ops_txt + ", fp32 accumulation, fp32 "
               "residual streams in ViT / LLM, split-precision (bf16 hi + lo) PaDT decoder" +
               {"fp8": ", fp8 e4m3 LLM weights streamed by the decode steps (prompt pass on the dequantised 16-bit image)",
                "fp8+act": ", fp8 e4m3 LLM weights: fp8 x fp8 MFMA prompt pass over e4m3 activation rows + fp8 weight streaming in the decode steps"}.get(args.weights, "") +
               ", random-init weights; batches of %d submitted one by one (4 distinct input batches in rotation), ViT/prefill/parse/PaDT decoder per batch, "
               "decode steps of %d consecutive batches share one weight pass (in-flight batching, per-sample results bit-identical to batch-at-a-time)")
        wl = fmt % ({"3b": "PaDT_Pro_3B", "7b": "PaDT_Pro_7B (untied head)", "small": "small_test_config (plumbing)"}[args.model] + " " + args.task.upper(),
                    args.batch, grid_hw[0], grid_hw[1], inp["L"], args.tnew, inp["n_obj"], inp["n_vrt"], args.batch, args.merge)
        line = {
            "metric": "images/sec PaDT_Pro_3B REC inference, 1/2/4/8 MI355X; box IoU vs ref",
            "value": round(value, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.operands, "data": "synthetic",
            "config": {"workload": wl,
                       "global_batch": args.batch * world, "parallelism": f"dp{world}", "batches_in_flight": args.depth * args.merge,
                       "decode_groups_in_flight": args.depth, "batches_per_decode_group": args.merge},
            "alg_tflop_per_image": round(alg_tf, 3),
            "alg_tflops_e2e": round(value * alg_tf, 1),
            "mfma_frac_e2e": round(value * alg_tf / MFMA_BF16_PEAK_TFLOPS / world, 4),
        }
        if exchange is not None:
            line["exchange"] = {"all_gathers": exchange.n_gathers, "batches_per_gather": args.merge, "bytes_per_rank_per_gather": exchange.words * 4 * args.merge,
                                "continuation_gathers": exchange.n_continuation_gathers,
                                "gather_wait_ms": {"total": round(exchange.wait_ms_total, 3), "max": round(exchange.wait_ms_max, 3),
                                                   "note": "host time this rank spent waiting for gathers to complete (ResultExchange._wait): what the slowest rank costs the others"},
                                "backend": os.environ.get("PADT_DIST_BACKEND", "nccl"),
                                "world_size": world, "device": device, "host_affinity": affinity, "ranks_seen_by_the_last_gather": int(gathered[-1].world) if gathered else None,
                                "rccl_version": (".".join(str(v) for v in torch.cuda.nccl.version()) if os.environ.get("PADT_DIST_BACKEND", "nccl") == "nccl" else None),
                                "note": "device-side pack (one kernel per batch) + one asynchronous all_gather_into_tensor per decode group"}
        line["range_guard"] = {"operands_policy": getattr(args, "policy", args.operands), "batches_rerun_on_bf16": int(getattr(model, "overflow_reruns", 0)),
                               "note": "fp16 operands under the device-side range guard: every batch's ViT rows, prototypes and prompt-pass / decode-step hidden rows are "
                                       "checked for inf / NaN inside the timed region (padt_check_finite); a flagged batch would be re-run on the bf16 instantiation"}
        if steady is not None:
            line["steady_state"] = steady
        if lat is not None:
            line["single_batch_latency"] = lat
        if alt is not None:
            line["unmerged_decode"] = alt
        def leg(key, fn):
            """Side legs never take the headline down: a failure is recorded under the key instead of raised."""
            try:
                line[key] = fn()
            except Exception as e:                                     # noqa: BLE001
                import traceback
                traceback.print_exc(file=sys.stderr)
                line[key] = {"error": f"{type(e).__name__}: {e}"[:300]}

        if full and not args.no_roofline and runner is not None:
            def roofs():
                roof, dec = insitu_leg(model, inp, args, cfg, run_steps, min(args.steps, 16))
                roof.update(replay_leg(model, inp, args, cfg))
                line["roofline_decode"] = decode_alone_leg(model, inp, args, cfg, dec)
                return roof
            leg("roofline", roofs)
        if full and args.bf16_twin and runner is not None and args.operands == "fp16" and args.extras:
            leg("operands_bf16", lambda: bf16_twin_leg(cfg, args, grid_hw, device))
        if full and args.extras and runner is not None and args.operands == "fp16":
            leg("reference_precision", lambda: reference_precision_leg(cfg, args, grid_hw, device))
        if full and args.from_images and runner is not None:
            leg("from_images", lambda: from_images_leg(model, inp, args, grid_hw, min(args.steps, 24)))
            leg("to_rle", lambda: to_rle_leg(model, inp, args, min(args.steps, 24)))
        if full and not args.no_cpu_baseline:
            leg("cpu_baseline", lambda: cpu_baseline_leg(cfg, args, inp, model))
        if isinstance(line.get("cpu_baseline"), dict) and "parity" in line["cpu_baseline"]:
            line["parity_vs_oracle"] = line["cpu_baseline"]["parity"]      # top level too: the metric's "box IoU vs ref" read-out of this run
        if full and args.extras:
            del runner
            m3, model = model, None
            leg("extra_workloads", lambda: extra_workloads(args, device, m3, cfg, grid_hw))
            del m3
        print(json.dumps(line), file=line_out, flush=True)
    if dist_on:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
