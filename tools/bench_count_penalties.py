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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataclasses  # noqa: E402

from padt_amd import ops  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

MODES = ("plain", "counts", "suppression", "both")


def time_rows(cfg, rows, op16, modes, args, device):
    bench = StepBench(cfg, rows, op16, args, device)
    sess, n = bench.sess, min(4, rows)                            # the first four rows own a 2 x 2 patch grid each

    def set_mode(mode):
        opts = GenOptions()
        if mode != "plain":
            opts = dataclasses.replace(opts, count_penalties=mode in ("counts", "both"), patch_suppression=mode in ("suppression", "both"))
        sess.begin(opts)
        if mode != "plain":                                       # one batch: f and p on every row, radius 1 and penalty 2.0 on the rows that own patches
            pen = mode in ("counts", "both")
            supp = [(1, 2.0)] * n + [None] * (rows - n) if mode in ("suppression", "both") else None
            bench.fake_batch(opts, vrt_off=[4 * min(b, n) for b in range(rows + 1)],
                             counts=dict(frequency_penalty=[0.5] * rows if pen else None, presence_penalty=[0.25] * rows if pen else None,
                                         patch_suppression=supp), count_grids=[(2, 2)] * n + [(0, 0)] * (rows - n))

    def check(mode, _):
        if mode != "plain":
            counted = int(ops.count_values(sess.cnt_text).sum()) + int(ops.count_values(sess.cnt_patch).sum())
            live = int(sess.unfinished.sum())
            assert counted >= live * bench.n_chk, f"mode {mode}: {counted} tokens counted for {live} live rows over {bench.n_chk} steps"

    bench.capture(["plain"] + [m for m in modes if m != "plain"], set_mode, check)
    us = bench.time(modes, set_mode)
    return [bench.record(mode, us[mode]) for mode in modes]


if __name__ == "__main__":
    main(parser(__doc__, MODES, tag=True), MODES, time_rows)
