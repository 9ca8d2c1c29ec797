"""Time the captured decode step under do_sample=True with and without HF's warpers after top-p (generate(min_p=, typical_p=, epsilon_cutoff=,
eta_cutoff=)).

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built like tools/bench_decode_weights.py builds it
(seeded random 16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass).  The step's hipGraph is captured once per step
mode (generation.StepMode: one graph serves every warper value), and the warper values are written to the session's gen_cfg before each window:

  sample        do_sample=True, top_k=50: the step as generate() runs it without the new arguments — padt_sample_token draws
  scores        ... + output_scores=True: padt_sample_token writes the warped row back (as it does for every mode below) and the row is filed
                per step — what the write-back alone costs, plus one row copy
  min_p         ... + min_p=0.05: padt_sample_token writes the warped row back, padt_warp_sample_rows_f32 warps it further and draws
  typical_p     ... + typical_p=0.9
  epsilon       ... + epsilon_cutoff=3e-4
  eta           ... + eta_cutoff=3e-4
  all           ... + all four (0.02 / 0.95 / 1e-4 / 2e-3)
  sample_k0     do_sample=True, top_k=0: every unmasked column is a candidate
  min_p_k0      ... + min_p=0.05: the row is swept in place until min_p has thinned it
  all_k0        ... + all four

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Per mode the median window is reported with the extremes, every
window's value and the distance to the baseline of the same top_k (sample / sample_k0).  Prints one JSON line per (rows, mode).

usage: python tools/bench_sampling_warpers.py [--rows 8,64] [--modes sample,min_p,...] [--operands fp16|bf16] [--steps 64] [--repeats 9]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from padt_amd import config  # noqa: E402
from padt_amd.generation import GenOptions, Sampling  # noqa: E402
from padt_amd.llm import DecodeSession  # noqa: E402
from padt_amd.weights import _pad_to  # noqa: E402
from bench_decode_weights import build_weights  # noqa: E402

ALL = dict(min_p=0.02, typical_p=0.95, epsilon_cutoff=1e-4, eta_cutoff=2e-3)
MODES = {"sample": (50, {}), "scores": (50, {}), "min_p": (50, dict(min_p=0.05)), "typical_p": (50, dict(typical_p=0.9)), "epsilon": (50, dict(epsilon_cutoff=3e-4)),
         "eta": (50, dict(eta_cutoff=3e-4)), "all": (50, ALL), "sample_k0": (0, {}), "min_p_k0": (0, dict(min_p=0.05)), "all_k0": (0, ALL)}


def set_mode(sess, mode):
    top_k, warp = MODES[mode]
    sess.begin(GenOptions(sampling=Sampling(1.0, top_k, 1.0, 1234, **warp), keep_scores=mode == "scores"))


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

    kept = {}
    for mode in modes:                                            # one eager step, the capture, then replays — per mode
        set_mode(sess, mode)
        reset()
        sess.run_steps(max(args.warmup, 2))
        torch.cuda.synchronize()
        kept[mode] = None if sess.logits is None else float((sess.logits[:, : cfg.vocab_size + sess.np_max] > float("-inf")).sum(1).float().mean())
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
        base = "sample_k0" if mode.endswith("_k0") else "sample"
        res = {"model": "PaDT_Pro_3B", "mode": mode, "rows": rows, "layers": cfg.num_hidden_layers, "operands": str(op16).split(".")[-1],
               "context": args.context, "top_k": MODES[mode][0], "warpers": MODES[mode][1], "us_per_step": round(med, 1),
               "us_min": round(min(us[mode]), 1), "us_max": round(max(us[mode]), 1), "windows": [round(u, 1) for u in us[mode]],
               "steps_per_window": args.steps, "weight_bytes": int(wbytes), "row_columns": cfg.vocab_size + sess.np_max,
               # finite columns per row in the session's row buffer after the last warm-up step: the survivors when the mode writes the row back
               "finite_columns_last_step": kept[mode]}
        if base in us:
            res["over_" + base] = round(med - statistics.median(us[base]), 1)
        out.append(res)
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
    args = ap.parse_args()
    modes = args.modes.split(",")
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode '{m}'")
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling_warpers.py times kernels on an MI355X: no GPU found")
    device = torch.device("cuda:0")
    op16 = torch.float16 if args.operands == "fp16" else torch.bfloat16
    cfg = config.padt_pro_3b()
    for rows in (int(r) for r in args.rows.split(",")):
        for res in time_rows(cfg, rows, op16, modes, args, device):
            print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
