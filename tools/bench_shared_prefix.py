"""Time generate(image_index=) against the expanded call: several queries per image in one batch.

PaDT_Pro_3B, synthetic weights, bench.py's REC geometry (grid [1,46,46] = 529 image tokens, 15 text ids before the image, 33 after it,
T = 28 with one object of 5 VRTs), batch 8 with 8 / 4 / 2 / 1 distinct images.  The queries on one image share the text before it and the
image tokens; the 33 ids after it are the query's own.  Per case, in ONE process and alternating shared / expanded: one warm-up call of
each, then `--calls` timed calls of each (host clock around a device synchronise: the whole call — ViT, prompt pass, decode steps, output
assembly).  Prints one JSON line per case with the median and the min-max of both, the prompt-pass row counts, and whether the two calls
returned the same sequences.

usage: python tools/bench_shared_prefix.py [--distinct 8,4,2,1] [--calls 7] [--model 3b|small] [--operands auto|fp16|bf16]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import padt_amd  # noqa: E402
from padt_amd.modeling import PaDTForConditionalGeneration  # noqa: E402
from padt_amd.synthetic import rec_schedule  # noqa: E402


def make_case(cfg, grid_hw, batch, n_images, seed, n_pre=15, n_post=33):
    """→ (shared kwargs, expanded kwargs) of one batch: sample b asks about image b % n_images."""
    g = torch.Generator().manual_seed(seed)
    hi = min(cfg.vocab_size, cfg.image_token_id) - 1
    P = grid_hw[0] * grid_hw[1]
    n_m = P // cfg.merge_unit
    index = [b % n_images for b in range(batch)]
    pix = torch.randn(n_images * P, cfg.patch_dim, generator=g).to(torch.bfloat16)
    pre = [torch.randint(0, hi, (n_pre - 1,), generator=g).tolist() for _ in range(n_images)]
    rows = [pre[u] + [cfg.vision_start_token_id] + [cfg.image_token_id] * n_m + torch.randint(0, hi, (n_post,), generator=g).tolist() for u in index]
    ids = torch.tensor(rows)
    grid = torch.tensor([[1, grid_hw[0], grid_hw[1]]] * n_images)
    idx_t = torch.tensor(index)
    common = dict(input_ids=ids.cuda(), attention_mask=torch.ones_like(ids).cuda())
    shared = dict(common, pixel_values=pix.cuda(), image_grid_thw=grid, image_index=index)
    expanded = dict(common, pixel_values=pix.view(n_images, P, -1)[idx_t].reshape(batch * P, -1).cuda(), image_grid_thw=grid[idx_t])
    return shared, expanded


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--distinct", default="8,4,2,1", help="distinct images per batch, one case each")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=7, help="timed calls of each variant per case (at least 5)")
    ap.add_argument("--tnew", type=int, default=28)
    ap.add_argument("--model", default="3b", choices=["3b", "small"])
    ap.add_argument("--operands", default="auto", choices=["auto", "fp16", "bf16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shared_prefix.py times generate() on an MI355X: no GPU found")
    if args.calls < 5:
        raise SystemExit("--calls must be at least 5")
    cfg = {"3b": padt_amd.padt_pro_3b, "small": padt_amd.small_test_config}[args.model]()
    grid_hw = (10, 12) if args.model == "small" else (46, 46)
    model = PaDTForConditionalGeneration.from_synthetic(cfg, seed=0, device="cuda", operands=args.operands)
    T = args.tnew
    gen = dict(max_new_tokens=T, schedule=rec_schedule(T, range(11, 16)), do_sample=False, sync_every=T)

    def call(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(**gen, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for n_images in (int(x) for x in args.distinct.split(",")):
        shared, expanded = make_case(cfg, grid_hw, args.batch, n_images, seed=1000 + n_images)
        _, o_s = call(shared)                                     # warm-up: plans, sessions, the captured step
        _, o_x = call(expanded)
        same = bool(torch.equal(o_s.sequences, o_x.sequences))
        ms = {"shared": [], "expanded": []}
        for _ in range(args.calls):
            ms["shared"].append(call(shared)[0])
            ms["expanded"].append(call(expanded)[0])
        plan = padt_amd.llm.plan_prompt_shared(cfg, shared["input_ids"], shared["attention_mask"], shared["image_grid_thw"],
                                               shared["image_index"], "cpu")
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"model": args.model, "operands": "fp16" if model.dtype == torch.float16 else "bf16", "batch": args.batch,
                          "distinct_images": n_images, "L": int(shared["input_ids"].shape[1]), "T": T, "calls": args.calls,
                          "prompt_rows_shared": int(plan.shared.ids.numel()), "prompt_rows_expanded": int(plan.ids.numel()),
                          "shared_ms_median": round(med["shared"], 2), "shared_ms_min": round(min(ms["shared"]), 2),
                          "shared_ms_max": round(max(ms["shared"]), 2), "expanded_ms_median": round(med["expanded"], 2),
                          "expanded_ms_min": round(min(ms["expanded"]), 2), "expanded_ms_max": round(max(ms["expanded"]), 2),
                          "speedup": round(med["expanded"] / med["shared"], 3), "same_sequences": same}), flush=True)


if __name__ == "__main__":
    main()
