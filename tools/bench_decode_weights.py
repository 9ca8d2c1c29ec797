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
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from padt_amd import config, ops  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from padt_amd.llm import DecodeSession  # noqa: E402
from padt_amd.weights import PreparedWeights, _pad_to  # noqa: E402

IMAGE_KEYS = {"bf16": (".wp",), "fp8": (".wq", ".ws"), "fp4": (".w4", ".we")}


def build_weights(cfg, mode, op16, device, seed=0):
    """The entries of PreparedWeights a decode step reads, for llm_weights = mode ("bf16" stands for the 16-bit image of the operand type)."""
    W = PreparedWeights()
    W.llm_weights, W.op16, W.fp8_prefill = mode, op16, False
    W.llm_ipad = _pad_to(cfg.intermediate_size, 64)
    D, hd = cfg.hidden_size, cfg.head_dim
    n_qkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd
    shapes = {"qkv": (n_qkv, D), "o": (D, cfg.num_attention_heads * hd), "gu": (2 * W.llm_ipad, D), "down": (D, W.llm_ipad)}
    g = torch.Generator(device=device).manual_seed(seed)
    layer = {}
    for nm, (n, k) in shapes.items():
        w = (torch.randn(n, k, generator=g, device=device) * 0.02).to(op16)
        if mode == "fp8":
            q, sc, _ = ops.quantize_fp8_rows(w, deq_dtype=op16)
            layer[nm] = {".wq": ops.pack_weight_fp8(q), ".ws": sc}
        elif mode == "fp4":
            c, e, _ = ops.quantize_mxfp4_rows(w, deq_dtype=op16)
            img, ex = ops.pack_weight_fp4(c, e)
            layer[nm] = {".w4": img, ".we": ex}
        else:
            layer[nm] = {".wp": ops.pack_weight(w)}
        del w
    wbytes = 0
    for i in range(cfg.num_hidden_layers):
        for nm, imgs in layer.items():
            for key, t in imgs.items():
                W[f"llm.{i}.{nm}{key}"] = t.clone()          # an allocation of its own per layer: nothing is served from a cache twice
                wbytes += t.numel() * t.element_size()
        W[f"llm.{i}.qkv.b"] = torch.zeros(n_qkv, device=device, dtype=op16)
    table = (torch.randn(cfg.vocab_size, D, generator=g, device=device) * 0.02).to(op16)
    W["llm.embed"] = W["llm.head"] = table
    W["llm.head.wp"] = ops.pack_weight(table)
    W["llm.norm"] = torch.ones(D, device=device, dtype=op16)
    return W, wbytes


def time_case(cfg, mode, rows, op16, args, device):
    W, wbytes = build_weights(cfg, mode, op16, device)
    window = max(args.steps, args.warmup)
    s_max = _pad_to(args.context + window + 1, 64)
    sess = DecodeSession(cfg, W, rows, s_max, 16, window + 1, device)
    g = torch.Generator(device=device).manual_seed(1)
    first = torch.randint(0, cfg.vocab_size, (rows,), generator=g, device=device)
    if args.rules:
        ids = torch.randint(0, cfg.vocab_size, (40,), generator=g, device=device).tolist()
        sess.begin(GenOptions(rules=ops.gen_rules_key(3, [ids[2 * i: 2 * i + 2] for i in range(8)], ids[16: 32], vocab_size=cfg.vocab_size)))
        sess.hist[:, : args.context] = torch.randint(0, cfg.vocab_size, (rows, args.context), generator=g, device=device).to(torch.int32)
        sess.hist_len.fill_(args.context)

    def reset():
        """`context` cached tokens per row, step counter at zero: every window replays the same steps (a window never runs past s_max / t_max)."""
        sess.step.zero_()
        sess.unfinished.fill_(1)
        sess.cur_tok.copy_(first)
        sess.slot.fill_(args.context)
        sess.lens.fill_(args.context)
        sess.pos3.fill_(args.context)

    reset()
    sess.run_steps(max(args.warmup, 2))                       # one eager step, the capture, then replays
    torch.cuda.synchronize()
    us = []
    for _ in range(args.repeats):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        sess.run_steps(args.steps)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / args.steps)
    head = W["llm.head.wp"]
    kv = rows * (args.context + args.steps / 2.0) * 2 * cfg.num_key_value_heads * cfg.head_dim * 2 * cfg.num_hidden_layers
    step_bytes = wbytes + head.numel() * head.element_size() + kv
    med = statistics.median(us)
    return {"weights": mode, "rules": bool(args.rules), "rows": rows, "layers": cfg.num_hidden_layers, "hidden": cfg.hidden_size, "operands": str(op16).split(".")[-1],
            "context": args.context, "us_per_step": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
            "windows": args.repeats, "steps_per_window": args.steps, "weight_bytes": int(wbytes), "bytes_per_step": int(step_bytes),
            "TB_per_s": round(step_bytes / (med * 1e-6) / 1e12, 3), "weight_TB_per_s": round(wbytes / (med * 1e-6) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="3b,7b")
    ap.add_argument("--rows", default="8,64")
    ap.add_argument("--weights", default="bf16,fp8,fp4")
    ap.add_argument("--operands", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--context", type=int, default=512, help="cached tokens per row when a window starts")
    ap.add_argument("--steps", type=int, default=32, help="graph replays per timed window")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rules", action="store_true", help="n-gram, bad-word and suppress-token bans active in the step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_weights.py times kernels on an MI355X: no GPU found")
    device = torch.device("cuda:0")
    op16 = torch.float16 if args.operands == "fp16" else torch.bfloat16
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
