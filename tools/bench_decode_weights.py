"""Time the captured decode step over 16-bit, fp8 and MXFP4 LLM weight images.

One case = one DecodeSession (padt_amd/llm.py) at the PaDT_Pro_3B or PaDT_Pro_7B LLM shape, full depth, `rows` samples with `--context`
cached tokens each: the step's hipGraph (embed, per layer [norm+qkv, rope+append+attention, o+resid, norm+gate/up+SwiGLU, down+resid], final
norm, logit head, token selection) is captured once and replayed.  Weights are seeded random matrices quantised by the library's own
quantisers (one layer's worth, copied into a separate allocation per layer, so every layer streams its own bytes from HBM); no ViT, no PaDT decoder and no
prompt pass are built.  Timing: `--warmup` replays, then `--repeats` windows of `--steps` replays between two device events; the median
window is reported with the extremes.  Prints one JSON line per case:

  weight_bytes     bytes of the four projection images of every layer (scales / block exponents included)
  bytes_per_step   weight_bytes + the 16-bit head table + the K and V rows the step reads
  TB_per_s         bytes_per_step / median step time

--rules adds the device-side bans of generate() to the step (ops.gen_rules in front of the head, the head reading the ban bitmap):
no_repeat_ngram_size=3, 8 two-token bad words and 16 suppressed ids over a random prompt history of `--context` ids per row.

usage: python tools/bench_decode_weights.py [--models 3b,7b] [--rows 8,64] [--weights bf16,fp8,fp4] [--operands fp16|bf16] [--rules]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from padt_amd import config, ops  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from step_bench import IMAGE_KEYS, StepBench, gpu_or_exit, parser  # noqa: E402


def time_case(cfg, mode, rows, op16, args, device):
    bench = StepBench(cfg, rows, op16, args, device, weights=mode)
    opts, prompt = GenOptions(), None
    if args.rules:
        ids = torch.randint(0, cfg.vocab_size, (40,), generator=bench.gen, device=device).tolist()
        opts = GenOptions(rules=ops.gen_rules_key(3, [ids[2 * i: 2 * i + 2] for i in range(8)], ids[16: 32], vocab_size=cfg.vocab_size))
        prompt = torch.randint(0, cfg.vocab_size, (rows, args.context), generator=bench.gen, device=device)

    def set_mode(_):
        bench.sess.begin(opts)
        if args.rules:                                            # the rows' prompt history: what the n-gram ban reads
            bench.fake_batch(opts, prompt_ids=prompt)

    bench.capture([mode], set_mode)                               # one eager step, the capture, then replays
    us = bench.time([mode], set_mode)[mode]
    head = bench.W["llm.head.wp"]
    kv = rows * (args.context + args.steps / 2.0) * 2 * cfg.num_key_value_heads * cfg.head_dim * 2 * cfg.num_hidden_layers
    step_bytes = bench.wbytes + head.numel() * head.element_size() + kv
    med = statistics.median(us)
    return {"weights": mode, "rules": bool(args.rules), "rows": rows, "layers": cfg.num_hidden_layers, "hidden": cfg.hidden_size, "operands": str(op16).split(".")[-1],
            "context": args.context, "us_per_step": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
            "windows": args.repeats, "steps_per_window": args.steps, "weight_bytes": int(bench.wbytes), "bytes_per_step": int(step_bytes),
            "TB_per_s": round(step_bytes / (med * 1e-6) / 1e12, 3), "weight_TB_per_s": round(bench.wbytes / (med * 1e-6) / 1e12, 3)}


def main():
    ap = parser(__doc__, steps=32, repeats=5)
    ap.add_argument("--models", default="3b,7b")
    ap.add_argument("--weights", default="bf16,fp8,fp4")
    ap.add_argument("--rules", action="store_true", help="n-gram, bad-word and suppress-token bans active in the step")
    args = ap.parse_args()
    device, op16 = gpu_or_exit(args)
    cfgs = {"3b": config.padt_pro_3b, "7b": config.padt_pro_7b}
    for m in args.models.split(","):
        cfg = cfgs[m]()
        for rows in (int(r) for r in args.rows.split(",")):
            for mode in args.weights.split(","):
                if mode not in IMAGE_KEYS:
                    raise SystemExit(f"unknown weights '{mode}'")
                res = {"model": "PaDT_Pro_" + m.upper(), **time_case(cfg, mode, rows, op16, args, device)}
                print(json.dumps(res), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
