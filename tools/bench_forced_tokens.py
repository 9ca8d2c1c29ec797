"""Time the captured decode step with generate(forced_tokens=...) in each of its kernel sequences, next to the steps it is derived from.

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built like tools/bench_token_logprobs.py builds it
(seeded random 16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass).  The step's hipGraph is captured once per mode:

  plain           the step as generate() runs it by default: logit head with the fused arg-max, padt_greedy_step
  logprobs        output_token_logprobs=True: the LSE head + padt_greedy_step_lp
  forced          forced_tokens without log-probs: the plain head + padt_forced_step
  forced_lp       forced_tokens + output_token_logprobs: the probe head (the LSE head plus one store) + padt_forced_step with the LSE fold
  forced_scores   ... + output_scores=True: under greedy decoding still the probe head, which now also writes every row's fp32 logits, and
                  padt_stash_step_f32 files them per step
  forced_rows     ... under do_sample=True (top_k 50): the ROW path — head with logits, padt_sample_token with write-back,
                  padt_forced_override, padt_token_logprob_rows_f32, padt_forced_step

  row_kernels     not a step: the three launches the GREEDY row path adds per step (a caller `logits_processor`: the hooked loop, which is
                  never captured) — padt_argmax_rows_f32 + padt_forced_override + padt_token_logprob_rows_f32 over the session's fp32 rows —
                  timed alone, `--steps` eager rounds per window.  The fused path's counterpart is forced_lp minus forced.

Every step of a forced mode is a forced step (a seeded table of text ids); the forced modes must emit exactly the table.  `plain` and `logprobs`
use nothing this feature added, so the script also runs in a tree without it (--modes plain,logprobs).

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Per mode the median window is reported with the extremes and every
window's value.  Prints one JSON line per (rows, mode).

usage: python tools/bench_forced_tokens.py [--rows 8,64] [--modes plain,logprobs,forced,forced_lp,forced_scores,forced_rows] [--operands fp16|bf16]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataclasses  # noqa: E402
import statistics  # noqa: E402

import torch  # noqa: E402

from padt_amd.generation import GenOptions, Sampling  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

MODES = ("plain", "logprobs", "forced", "forced_lp", "forced_scores", "forced_rows", "row_kernels")


def time_row_kernels(sess, cfg, rows, table, args):
    """µs per round of argmax_rows + forced_override + token_logprob_rows over the session's row buffer (random fp32 rows), per window"""
    from padt_amd import ops
    n = cfg.vocab_size + sess.np_max
    lg = torch.randn((rows, (n + 3) // 4 * 4), device=table.device, dtype=torch.float32) * 4
    lp = torch.zeros((rows, sess.t_max), device=table.device, dtype=torch.float32)
    unf = torch.ones(rows, device=table.device, dtype=torch.int32)
    step = torch.zeros(1, device=table.device, dtype=torch.int32)
    us = []
    for _ in range(args.repeats + 1):                             # the first window warms up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.steps):
            ops.argmax_rows(lg, n, sess.part_val, sess.part_idx, rows)
            ops.forced_override(sess.part_idx, table, step, unf, n, rows)
            ops.token_logprob_rows(lg, n, sess.part_idx, unf, step, lp, rows)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / args.steps)
    return us[1:]


def time_rows(cfg, rows, op16, modes, args, device):
    row_kernels, modes = "row_kernels" in modes, [m for m in modes if m != "row_kernels"]
    bench = StepBench(cfg, rows, op16, args, device)
    sess = bench.sess
    table = torch.randint(0, min(cfg.vocab_size, cfg.image_token_id), (rows, sess.t_max), generator=bench.gen, device=device).to(torch.int32)

    def set_mode(mode):
        opts = GenOptions(keep_scores=mode == "forced_scores", token_logprobs=mode in ("logprobs", "forced_lp", "forced_scores", "forced_rows"),
                          sampling=Sampling(1.0, 50, 1.0, 7) if mode == "forced_rows" else None)
        if mode.startswith("forced"):
            opts = dataclasses.replace(opts, forced=True)
        sess.begin(opts)
        if mode.startswith("forced"):                             # one batch whose table forces every step of every row
            bench.fake_batch(opts, forced=table)

    tokens = bench.capture(modes, set_mode)
    free = [m for m in modes if not m.startswith("forced")]
    for mode in free[1:]:                                         # the free modes select the same tokens ...
        assert torch.equal(tokens[mode], tokens[free[0]]), f"mode {mode} selected other tokens than {free[0]}"
    for mode in modes:                                            # ... and a forced mode emits its table
        if mode.startswith("forced"):
            assert torch.equal(tokens[mode], table[:, : bench.n_chk].long()), f"mode {mode} did not emit the forced tokens"
    us = bench.time(modes, set_mode)
    out = [bench.record(mode, us[mode]) for mode in modes]
    if row_kernels:
        u = time_row_kernels(sess, cfg, rows, table, args)
        out.append({"model": "PaDT_Pro_3B", "mode": "row_kernels", "rows": rows, "us_per_step": round(statistics.median(u), 1),
                    "us_min": round(min(u), 1), "us_max": round(max(u), 1), "windows": [round(x, 1) for x in u], "steps_per_window": args.steps})
    return out


if __name__ == "__main__":
    main(parser(__doc__, MODES, tag=True), MODES, time_rows)
