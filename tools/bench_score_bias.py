"""Time the captured decode step with generate(logit_bias=, patch_bias=, exponential_decay_length_penalty=) next to the step without them.

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built like tools/bench_forced_tokens.py builds it
(seeded random 16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass).  The step's hipGraph is captured once per mode:

  plain        the step as generate() runs it by default: padt_vrt_head with the fused arg-max, padt_greedy_step.  It uses nothing this
               feature added, so the script also runs in a tree without it (--modes plain): THAT run is the yardstick of the off path — the
               new build's `plain` is compared with the parent commit's `plain` of the same session, never with itself
  logit_bias   padt_vrt_head_bias: a bias over 64 text ids (the plain run's first tokens banned with -inf, so the run must change)
  patch_bias   ... generate(patch_bias=) on for a batch in which no row owns a patch: the patch columns of the vector stay zero
  decay        ... exponential_decay_length_penalty=(8, 1.05)
  all          ... the three together
  all_lp       ... with output_token_logprobs=True: the LSE instantiation of the same head + padt_greedy_step_lp

The four `on` modes launch the SAME kernel with the SAME pointers (one step mode, one captured graph: bias vector and decay table are dense
device arrays read whatever they hold), so they are expected to cost the same; they are all timed to show that.

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Per mode the median window is reported with the extremes and every
window's value.  Prints one JSON line per (rows, mode).

usage: python tools/bench_score_bias.py [--rows 8,64] [--modes plain,logit_bias,patch_bias,decay,all,all_lp] [--operands fp16|bf16] [--tag T]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataclasses  # noqa: E402

import torch  # noqa: E402

from padt_amd.generation import GenOptions  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

MODES = ("plain", "logit_bias", "patch_bias", "decay", "all", "all_lp")
DECAY = (8, 1.05)


def time_rows(cfg, rows, op16, modes, args, device):
    bench = StepBench(cfg, rows, op16, args, device)
    sess, banned = bench.sess, []

    def set_mode(mode):
        opts = GenOptions(token_logprobs=mode == "all_lp")
        if mode != "plain":
            lb = None
            if mode in ("logit_bias", "all", "all_lp"):
                lb = {int(t): float("-inf") for t in banned}
                lb.update({i: 0.25 * (i % 7) - 0.5 for i in range(100, 164) if i not in lb and i % 7 != 2})
                lb = tuple(sorted(lb.items()))
            opts = dataclasses.replace(opts, logit_bias=lb, decay=DECAY if mode in ("decay", "all", "all_lp") else None,
                                       patch_bias=mode in ("patch_bias", "all", "all_lp"))
        sess.begin(opts)
        if opts.patch_bias:                                       # one batch in which no row owns a patch: its segment of the vector is empty
            bench.fake_batch(opts, patch_bias=[None] * rows)

    def check(mode, tok):
        if mode == "plain":                                       # plain runs first: its first tokens get banned
            banned[:] = sorted(set(tok[:, 0].tolist()))

    tokens = bench.capture(["plain"] + [m for m in modes if m != "plain"], set_mode, check)
    for mode in modes:
        if mode in ("logit_bias", "all", "all_lp"):                  # the banned columns are gone from step 0
            assert not set(tokens[mode][:, 0].tolist()) & set(banned), f"mode {mode} emitted a banned token"
        if mode in ("patch_bias", "decay"):                           # no row owns a patch here and no row is near EOS: the run is the plain one
            assert torch.equal(tokens[mode][:, 0], tokens["plain"][:, 0]), f"mode {mode} changed the first token"
    us = bench.time(modes, set_mode)
    return [bench.record(mode, us[mode]) for mode in modes]


if __name__ == "__main__":
    main(parser(__doc__, MODES, tag=True), MODES, time_rows)
