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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics  # noqa: E402

from padt_amd.generation import GenOptions, Sampling  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

ALL = dict(min_p=0.02, typical_p=0.95, epsilon_cutoff=1e-4, eta_cutoff=2e-3)
MODES = {"sample": (50, {}), "scores": (50, {}), "min_p": (50, dict(min_p=0.05)), "typical_p": (50, dict(typical_p=0.9)), "epsilon": (50, dict(epsilon_cutoff=3e-4)),
         "eta": (50, dict(eta_cutoff=3e-4)), "all": (50, ALL), "sample_k0": (0, {}), "min_p_k0": (0, dict(min_p=0.05)), "all_k0": (0, ALL)}


def time_rows(cfg, rows, op16, modes, args, device):
    bench = StepBench(cfg, rows, op16, args, device)
    sess = bench.sess

    def set_mode(mode):
        top_k, warp = MODES[mode]
        sess.begin(GenOptions(sampling=Sampling(1.0, top_k, 1.0, 1234, **warp), keep_scores=mode == "scores"))

    kept = {}

    def finite_columns(mode, _):
        kept[mode] = None if sess.logits is None else float((sess.logits[:, : cfg.vocab_size + sess.np_max] > float("-inf")).sum(1).float().mean())

    bench.capture(modes, set_mode, check=finite_columns)
    us = bench.time(modes, set_mode)
    out = []
    for mode in modes:
        base = "sample_k0" if mode.endswith("_k0") else "sample"
        # finite_columns_last_step: per row in the session's row buffer after the last warm-up step — the survivors when the mode writes the row back
        res = bench.record(mode, us[mode], top_k=MODES[mode][0], warpers=MODES[mode][1], row_columns=cfg.vocab_size + sess.np_max,
                           finite_columns_last_step=kept[mode])
        if base in us:
            res["over_" + base] = round(statistics.median(us[mode]) - statistics.median(us[base]), 1)
        out.append(res)
    return out


if __name__ == "__main__":
    main(parser(__doc__, MODES), MODES, time_rows)
