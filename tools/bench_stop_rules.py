"""Time the captured decode step with generate(stop_sequences=, min_tokens=, max_tokens=) next to the step without them.

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built like tools/bench_score_bias.py builds it
(seeded random 16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass).  The step's hipGraph is captured once per mode:

  plain           the step as generate() runs it by default: padt_vrt_head with the fused arg-max, padt_greedy_step.  It uses nothing this
                  feature added, so the script also runs in a tree without it (--modes plain): THAT run is the yardstick of the off path — the
                  new build's `plain` is compared with the parent commit's `plain` of the same session, never with itself
  stop_sequences  padt_stop_ban (nothing to add: min 0) + padt_vrt_head_ban + padt_stop_match over a FULL table: 32 sequences of 32 ids, none
                  of which the run completes
  min_tokens      ... a minimum no row reaches inside the window: the EOS ids are banned at every step; no sequence
  max_tokens      ... per-row budgets no row reaches inside the window; no sequence, minimum 0

The three `on` modes launch the SAME kernels with the SAME pointers (one step mode, one captured graph: table, minima and budgets are device
arrays read whatever they hold); they are all timed to show what the contents cost.

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Per mode the median window is reported with the extremes and every
window's value.  Prints one JSON line per (rows, mode).

usage: python tools/bench_stop_rules.py [--rows 8,64] [--modes plain,stop_sequences,min_tokens,max_tokens] [--operands fp16|bf16] [--tag T]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataclasses  # noqa: E402

import torch  # noqa: E402

from padt_amd.generation import GenOptions  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

MODES = ("plain", "stop_sequences", "min_tokens", "max_tokens")


def time_rows(cfg, rows, op16, modes, args, device):
    bench = StepBench(cfg, rows, op16, args, device)
    sess, window = bench.sess, max(args.steps, args.warmup)

    def set_mode(mode):
        opts = GenOptions()
        if mode != "plain":
            seqs = tuple(tuple(1000 + 32 * i + k for k in range(32)) for i in range(32)) if mode == "stop_sequences" else None
            opts = dataclasses.replace(opts, stop_sequences=seqs, min_tokens=window + 1 if mode == "min_tokens" else None,
                                       row_limits=mode == "max_tokens")
        sess.begin(opts)
        if mode != "plain":                                       # a batch without budgets: no row ends inside a window, every step does a live row's work
            bench.fake_batch(opts, stop=dict(min_tokens=None, max_tokens=None))

    def check(mode, _):
        if mode != "plain":
            assert bool(sess.unfinished.all()) and not bool(sess.finish_reason.any()), f"mode {mode}: a row ended inside the window"

    tokens = bench.capture(["plain"] + [m for m in modes if m != "plain"], set_mode, check)
    eos = int(cfg.eos_token_id)
    for mode in modes:
        if mode in ("stop_sequences", "max_tokens"):                  # nothing is banned and nothing matches: the run is the plain one
            assert torch.equal(tokens[mode], tokens["plain"]), f"mode {mode} changed the run"
        if mode == "min_tokens":
            assert not bool((tokens[mode] == eos).any()), "an EOS below min_tokens"
    us = bench.time(modes, set_mode)
    return [bench.record(mode, us[mode]) for mode in modes]


if __name__ == "__main__":
    main(parser(__doc__, MODES, tag=True), MODES, time_rows)
