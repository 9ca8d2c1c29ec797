"""Time the captured decode step with generate(frequency_penalty=, presence_penalty=, patch_suppression=) next to the step without them.

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built like tools/bench_stop_rules.py builds it
(seeded random 16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass; the first four rows own a 2 x 2 patch grid each).
The step's hipGraph is captured once per step mode:

  plain        the step as generate() runs it by default: padt_vrt_head with the fused arg-max, padt_greedy_step.  It uses nothing this
               feature added, so the script also runs in a tree without it (--modes plain): THAT run is the yardstick of the off path — the
               new build's `plain` is compared with the parent commit's `plain` of the same session, never with itself
  counts       padt_vrt_head_counts + padt_count_update with f = 0.5, p = 0.25 on every row, no suppression (every radius -1)
  suppression  ... f = p = 0, radius 1 and penalty 2.0 on every row
  both         ... all of it

The three `on` modes launch the SAME kernels with the SAME pointers (one step mode, one captured graph: the head reads the whole text count
table whatever f and p are); they are all timed to show what the contents cost.

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Per mode the median window is reported with the extremes and every
window's value.  Prints one JSON line per (rows, mode).

usage: python tools/bench_count_penalties.py [--rows 8,64] [--modes plain,counts,suppression,both] [--operands fp16|bf16] [--tag T]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from padt_amd import config, ops  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from padt_amd.llm import DecodeSession  # noqa: E402
from padt_amd.weights import _pad_to  # noqa: E402
from bench_decode_weights import build_weights  # noqa: E402

MODES = ("plain", "counts", "suppression", "both")


def set_mode(sess, mode):
    opts = GenOptions()
    if mode != "plain":
        opts = dataclasses.replace(opts, count_penalties=mode in ("counts", "both"), patch_suppression=mode in ("suppression", "both"))
    sess.begin(opts)
    if mode != "plain":                                               # what modeling._launch writes per batch
        n = min(4, sess.B)
        sess.vrt_off.copy_(torch.tensor([4 * min(b, n) for b in range(sess.B + 1)], dtype=torch.int32))
        sess.cgrid[:n].fill_(2)
        if mode in ("counts", "both"):
            sess.cpen[0].fill_(0.5)
            sess.cpen[1].fill_(0.25)
        if mode in ("suppression", "both"):
            sess.cpen[2].fill_(2.0)
            sess.cradius[:n].fill_(1)
    else:
        sess.vrt_off.zero_()


def time_rows(cfg, rows, op16, modes, args, device):
    W, wbytes = build_weights(cfg, "bf16", op16, device)
    window = max(args.steps, args.warmup)
    sess = DecodeSession(cfg, W, rows, _pad_to(args.context + window + 1, 64), 16, window + 1, device)
    gen = torch.Generator(device=device).manual_seed(1)
    first = torch.randint(0, cfg.vocab_size, (rows,), generator=gen, device=device)

    def reset():
        """`context` cached tokens per row, step counter at zero: every window replays the same steps (never past s_max / t_max)"""
        sess.step.zero_()
        sess.unfinished.fill_(1)
        sess.cur_tok.copy_(first)
        sess.slot.fill_(args.context)
        sess.lens.fill_(args.context)
        sess.pos3.fill_(args.context)

    n_chk = max(args.warmup, 2)
    tokens = {}
    for mode in ["plain"] + [m for m in modes if m != "plain"]:     # one eager step, the capture, then replays — per mode
        set_mode(sess, mode)
        reset()
        sess.run_steps(n_chk)
        torch.cuda.synchronize()
        tokens[mode] = sess.tokens[:, :n_chk].clone()
        if mode != "plain":
            counted = int(ops.count_values(sess.cnt_text).sum()) + int(ops.count_values(sess.cnt_patch).sum())
            live = int(sess.unfinished.sum())
            assert counted >= live * n_chk, f"mode {mode}: {counted} tokens counted for {live} live rows over {n_chk} steps"
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
    out = []
    for mode in modes:
        med = statistics.median(us[mode])
        out.append({"model": "PaDT_Pro_3B", "mode": mode, "rows": rows, "layers": cfg.num_hidden_layers, "operands": str(op16).split(".")[-1],
                    "context": args.context, "us_per_step": round(med, 1), "us_min": round(min(us[mode]), 1), "us_max": round(max(us[mode]), 1),
                    "windows": [round(u, 1) for u in us[mode]], "steps_per_window": args.steps, "weight_bytes": int(wbytes)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="8,64")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--operands", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--context", type=int, default=512, help="cached tokens per row when a window starts")
    ap.add_argument("--steps", type=int, default=64, help="graph replays per timed window")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--tag", default="", help="copied into every JSON line (which tree / which run)")
    args = ap.parse_args()
    modes = args.modes.split(",")
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode '{m}'")
    if not torch.cuda.is_available():
        raise SystemExit("bench_count_penalties.py times kernels on an MI355X: no GPU found")
    device = torch.device("cuda:0")
    op16 = torch.float16 if args.operands == "fp16" else torch.bfloat16
    cfg = config.padt_pro_3b()
    for rows in (int(r) for r in args.rows.split(",")):
        for res in time_rows(cfg, rows, op16, modes, args, device):
            print(json.dumps(dict(res, tag=args.tag) if args.tag else res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
