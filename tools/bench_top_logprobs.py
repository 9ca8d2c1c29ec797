"""Time the captured decode step with generate(top_logprobs=k) / generate(output_patch_logprobs=True), without them, and with output_scores=True
(what they replace).

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built like tools/bench_token_logprobs.py builds it
(seeded random 16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass), with `--patches` prototype rows per sample so
that the score rows have a realistic width (vocab + rows * patches columns) and every sample has patch columns of its own.  The step's
hipGraph is captured once per mode:

  plain      the step as generate() runs it by default: logit head with the fused arg-max, padt_greedy_step
  top5       top_logprobs=5: the head also writes the fp32 row, padt_topk_logprob_rows_f32 (two launches) reduces it to 5 ids + log-probs
  top32      top_logprobs=32
  patches    output_patch_logprobs=True: the same launches with k = 0 and the gather of the sample's own patch columns
  both       top_logprobs=5 and output_patch_logprobs=True
  scores     output_scores=True: the head writes every row's fp32 logits, padt_stash_step_f32 files them per step

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Per mode the median window is reported with the extremes and every
window's value.  For the flagged modes the launch pair is also timed alone (`pair_us`, back-to-back launches over the session's row buffer) with
the rate at which it reads the rows (`pair_read_GBps`: the rows are cache-resident there, so this is no HBM bandwidth); `extra_bytes_per_step` is
a count of what the mode moves, not a measurement.  Prints one JSON line per (rows, mode).

usage: python tools/bench_top_logprobs.py [--rows 8,64] [--modes plain,top5,top32,patches,both,scores] [--operands fp16|bf16] [--patches 256]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from padt_amd import config  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from padt_amd.llm import DecodeSession  # noqa: E402
from padt_amd.weights import _pad_to  # noqa: E402
from bench_decode_weights import build_weights  # noqa: E402

MODES = {"plain": (0, False), "top5": (5, False), "top32": (32, False), "patches": (0, True), "both": (5, True), "scores": (0, False)}


def set_mode(sess, mode, patches):
    sess.begin(GenOptions(keep_scores=mode == "scores", top_logprobs=MODES[mode][0], patch_logprobs=MODES[mode][1]), patches)


def time_rows(cfg, rows, op16, modes, args, device):
    W, wbytes = build_weights(cfg, "bf16", op16, device)
    window = max(args.steps, args.warmup)
    sess = DecodeSession(cfg, W, rows, _pad_to(args.context + window + 1, 64), rows * args.patches, window + 1, device)
    sess.proto.copy_(torch.randn(sess.proto.shape, generator=torch.Generator(device=device).manual_seed(2), device=device) * 0.02)
    sess.vrt_off.copy_(torch.arange(rows + 1, dtype=torch.int32, device=device) * args.patches)      # every sample owns `patches` columns
    first = torch.randint(0, cfg.vocab_size, (rows,), generator=torch.Generator(device=device).manual_seed(1), device=device)

    def reset():
        """`context` cached tokens per row, step counter at zero: every window replays the same steps (never past s_max / t_max)"""
        sess.step.zero_()
        sess.unfinished.fill_(1)
        sess.cur_tok.copy_(first)
        sess.slot.fill_(args.context)
        sess.lens.fill_(args.context)
        sess.pos3.fill_(args.context)

    tokens = {}
    for mode in modes:                                            # one eager step, the capture, then replays — per mode
        set_mode(sess, mode, args.patches)
        reset()
        sess.run_steps(max(args.warmup, 2))
        torch.cuda.synchronize()
        tokens[mode] = sess.tokens[:, : max(args.warmup, 2)].clone()
        if MODES[mode][0]:                                        # greedy: the best candidate of every step is the token the step selected
            assert torch.equal(sess.top_idx[:, : max(args.warmup, 2), 0].long(), tokens[mode]), f"mode {mode}: entry 0 is not the selected token"
    for mode in modes[1:]:                                        # the modes select the same tokens: only what is written next to them differs
        assert torch.equal(tokens[mode], tokens[modes[0]]), f"mode {mode} selected other tokens than {modes[0]}"
    us = {m: [] for m in modes}
    for _ in range(args.repeats):
        for mode in modes:
            set_mode(sess, mode, args.patches)
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            sess.run_steps(args.steps)
            e1.record()
            torch.cuda.synchronize()
            us[mode].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    width = cfg.vocab_size + sess.np_max
    row_bytes = rows * width * 4

    def pair_alone(mode, n=200):
        """The two launches of padt_topk_logprob_rows_f32 alone, back to back over the session's row buffer as the last step left it (the rows
        are then cache-resident, as they are in the step, where the head has just written them) → us per call: median of 5 windows of n calls"""
        from padt_amd import ops
        set_mode(sess, mode, args.patches)
        reset()
        t = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                ops.topk_logprob_rows(sess.logits, width, sess.unfinished, sess.step, sess.topk_ws, rows, top_idx=sess.top_idx, top_val=sess.top_val,
                                      vrt_off=sess.vrt_off if sess.mode.patches else None, vocab=cfg.vocab_size,
                                      patch_lp=sess.patch_lp if sess.mode.patches else None)
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / n)
        return statistics.median(t)
    out = []
    for mode in modes:
        med = statistics.median(us[mode])
        k, pt = MODES[mode]
        # bytes next to the plain step: the row written by the head and read once by the selection (scores: written, read and filed again)
        extra = 3 * row_bytes if mode == "scores" else (2 * row_bytes + rows * (8 * k + 4 * args.patches * pt) if (k or pt) else 0)
        out.append({"model": "PaDT_Pro_3B", "mode": mode, "rows": rows, "layers": cfg.num_hidden_layers, "operands": str(op16).split(".")[-1],
                    "context": args.context, "row_columns": width, "us_per_step": round(med, 1), "us_min": round(min(us[mode]), 1),
                    "us_max": round(max(us[mode]), 1), "windows": [round(u, 1) for u in us[mode]], "steps_per_window": args.steps,
                    "weight_bytes": int(wbytes), "extra_bytes_per_step": int(extra)})
        if k or pt:                                               # measured: the launch pair alone and the rate at which it reads the rows
            pu = pair_alone(mode)
            out[-1].update(pair_us=round(pu, 2), pair_read_GBps=round(row_bytes / pu / 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="8,64")
    ap.add_argument("--modes", default="plain,top5,top32,patches,both,scores")
    ap.add_argument("--operands", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--context", type=int, default=512, help="cached tokens per row when a window starts")
    ap.add_argument("--patches", type=int, default=256, help="prototype rows (patch columns) per sample")
    ap.add_argument("--steps", type=int, default=64, help="graph replays per timed window")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    modes = args.modes.split(",")
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode '{m}'")
    if not torch.cuda.is_available():
        raise SystemExit("bench_top_logprobs.py times kernels on an MI355X: no GPU found")
    device = torch.device("cuda:0")
    op16 = torch.float16 if args.operands == "fp16" else torch.bfloat16
    cfg = config.padt_pro_3b()
    for rows in (int(r) for r in args.rows.split(",")):
        for res in time_rows(cfg, rows, op16, modes, args, device):
            print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
