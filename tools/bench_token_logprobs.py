"""Time the captured decode step with and without generate(output_token_logprobs=True), and with output_scores=True (what the flag replaces).

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built like tools/bench_decode_weights.py builds it
(seeded random 16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass).  The step's hipGraph is captured once per mode:

  plain      the step as generate() runs it by default: logit head with the fused arg-max, padt_greedy_step
  logprobs   output_token_logprobs=True: the LSE head (per-block sum of exponentials next to the arg-max partials) + padt_greedy_step_lp
  scores     output_scores=True: the head also writes every row's fp32 logits, padt_stash_step_f32 files them per step

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Per mode the median window is reported with the extremes and every
window's value.  Prints one JSON line per (rows, mode).

usage: python tools/bench_token_logprobs.py [--rows 8,64] [--modes plain,logprobs,scores] [--operands fp16|bf16] [--steps 64] [--repeats 9]"""
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


def set_mode(sess, mode):
    sess.begin(GenOptions(keep_scores=mode == "scores", token_logprobs=mode == "logprobs"))


def time_rows(cfg, rows, op16, modes, args, device):
    W, wbytes = build_weights(cfg, "bf16", op16, device)
    window = max(args.steps, args.warmup)
    sess = DecodeSession(cfg, W, rows, _pad_to(args.context + window + 1, 64), 16, window + 1, device)
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
        set_mode(sess, mode)
        reset()
        sess.run_steps(max(args.warmup, 2))
        torch.cuda.synchronize()
        tokens[mode] = sess.tokens[:, : max(args.warmup, 2)].clone()
    for mode in modes[1:]:                                        # the modes select the same tokens: only what is written next to them differs
        assert torch.equal(tokens[mode], tokens[modes[0]]), f"mode {mode} selected other tokens than {modes[0]}"
    us = {m: [] for m in modes}
    for _ in range(args.repeats):
        for mode in modes:
            set_mode(sess, mode)
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            sess.run_steps(args.steps)
            e1.record()
            torch.cuda.synchronize()
            us[mode].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    width = cfg.vocab_size + sess.np_max
    extra = {"plain": 0, "logprobs": sess.nblk * rows * 4 + rows * 4, "scores": 3 * rows * width * 4}      # bytes written (+ re-read by the stash) next to the plain step
    out = []
    for mode in modes:
        med = statistics.median(us[mode])
        out.append({"model": "PaDT_Pro_3B", "mode": mode, "rows": rows, "layers": cfg.num_hidden_layers, "operands": str(op16).split(".")[-1],
                    "context": args.context, "us_per_step": round(med, 1), "us_min": round(min(us[mode]), 1), "us_max": round(max(us[mode]), 1),
                    "windows": [round(u, 1) for u in us[mode]], "steps_per_window": args.steps, "weight_bytes": int(wbytes),
                    "extra_bytes_per_step": int(extra[mode])})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="8,64")
    ap.add_argument("--modes", default="plain,logprobs,scores")
    ap.add_argument("--operands", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--context", type=int, default=512, help="cached tokens per row when a window starts")
    ap.add_argument("--steps", type=int, default=64, help="graph replays per timed window")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    modes = args.modes.split(",")
    for m in modes:
        if m not in ("plain", "logprobs", "scores"):
            raise SystemExit(f"unknown mode '{m}'")
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_logprobs.py times kernels on an MI355X: no GPU found")
    device = torch.device("cuda:0")
    op16 = torch.float16 if args.operands == "fp16" else torch.bfloat16
    cfg = config.padt_pro_3b()
    for rows in (int(r) for r in args.rows.split(",")):
        for res in time_rows(cfg, rows, op16, modes, args, device):
            print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
