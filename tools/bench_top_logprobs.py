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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics  # noqa: E402

import torch  # noqa: E402

from padt_amd import ops  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

MODES = {"plain": (0, False), "top5": (5, False), "top32": (32, False), "patches": (0, True), "both": (5, True), "scores": (0, False)}


def time_rows(cfg, rows, op16, modes, args, device):
    bench = StepBench(cfg, rows, op16, args, device, np_max=rows * args.patches)
    sess = bench.sess
    bench.random_prototypes(torch.Generator(device=device).manual_seed(2))

    def set_mode(mode):
        opts = GenOptions(keep_scores=mode == "scores", top_logprobs=MODES[mode][0], patch_logprobs=MODES[mode][1])
        sess.begin(opts, args.patches)
        bench.fake_batch(opts, vrt_off=[b * args.patches for b in range(rows + 1)])      # every sample owns `patches` columns

    def check(mode, tok):
        if MODES[mode][0]:                                        # greedy: the best candidate of every step is the token the step selected
            assert torch.equal(sess.top_idx[:, : bench.n_chk, 0].long(), tok), f"mode {mode}: entry 0 is not the selected token"

    tokens = bench.capture(modes, set_mode, check)
    for mode in modes[1:]:                                        # the modes select the same tokens: only what is written next to them differs
        assert torch.equal(tokens[mode], tokens[modes[0]]), f"mode {mode} selected other tokens than {modes[0]}"
    us = bench.time(modes, set_mode)
    width = cfg.vocab_size + sess.np_max
    row_bytes = rows * width * 4

    def pair_alone(mode, n=200):
        """The two launches of padt_topk_logprob_rows_f32 alone, back to back over the session's row buffer as the last step left it (the rows
        are then cache-resident, as they are in the step, where the head has just written them) → us per call: median of 5 windows of n calls"""
        set_mode(mode)
        bench.rewind()
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
        k, pt = MODES[mode]
        # bytes next to the plain step: the row written by the head and read once by the selection (scores: written, read and filed again)
        extra = 3 * row_bytes if mode == "scores" else (2 * row_bytes + rows * (8 * k + 4 * args.patches * pt) if (k or pt) else 0)
        out.append(bench.record(mode, us[mode], row_columns=width, extra_bytes_per_step=int(extra)))
        if k or pt:                                               # measured: the launch pair alone and the rate at which it reads the rows
            pu = pair_alone(mode)
            out[-1].update(pair_us=round(pu, 2), pair_read_GBps=round(row_bytes / pu / 1e3, 1))
    return out


if __name__ == "__main__":
    ap = parser(__doc__, MODES)
    ap.add_argument("--patches", type=int, default=256, help="prototype rows (patch columns) per sample")
    main(ap, MODES, time_rows)
