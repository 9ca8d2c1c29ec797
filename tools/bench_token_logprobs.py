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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from padt_amd.generation import GenOptions  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

MODES = ("plain", "logprobs", "scores")


def time_rows(cfg, rows, op16, modes, args, device):
    bench = StepBench(cfg, rows, op16, args, device)
    sess = bench.sess

    def set_mode(mode):
        sess.begin(GenOptions(keep_scores=mode == "scores", token_logprobs=mode == "logprobs"))

    tokens = bench.capture(modes, set_mode)
    for mode in modes[1:]:                                        # the modes select the same tokens: only what is written next to them differs
        assert torch.equal(tokens[mode], tokens[modes[0]]), f"mode {mode} selected other tokens than {modes[0]}"
    us = bench.time(modes, set_mode)
    width = cfg.vocab_size + sess.np_max
    extra = {"plain": 0, "logprobs": sess.nblk * rows * 4 + rows * 4, "scores": 3 * rows * width * 4}      # bytes written (+ re-read by the stash) next to the plain step
    return [bench.record(mode, us[mode], extra_bytes_per_step=int(extra[mode])) for mode in modes]


if __name__ == "__main__":
    main(parser(__doc__, MODES), MODES, time_rows)
