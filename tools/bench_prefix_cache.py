"""Time generate(prefix=) against generate(image_index=) and the expanded call, the cost of encode_prefix, and the fan-out kernel alone.

PaDT_Pro_3B, synthetic weights, bench.py's REC geometry as tools/bench_shared_prefix.py uses it (grid [1,46,46] = 529 image tokens, 15 text
ids before the image, 33 after it, T = 28 with one object of 5 VRTs), batch 8 with 8 / 4 / 2 / 1 distinct images.  The cached prefix of an
image is the text before it and its image tokens (544 rows); the 33 ids after it are the query's own.  Per case, in ONE process and
alternating prefix / image_index / expanded: one warm-up call of each, then `--calls` timed calls of each (host clock around a device
synchronise: the whole call), and `--calls` timed encode_prefix calls.  Prints one JSON line per case.

Then the kernel alone (`padt_kv_prefix_fanout`, one layer of the last case's handle into a session of `--batch` rows: cache images and join
rows) against a device-to-device copy of the byte count it WRITES, in the same process, by device events over `--reps` launches each.  That
copy is its yardstick; the ratio is reported, not judged.

usage: python tools/bench_prefix_cache.py [--distinct 8,4,2,1] [--calls 7] [--model 3b|small] [--operands auto|fp16|bf16]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import padt_amd  # noqa: E402
from padt_amd import ops  # noqa: E402
from padt_amd.modeling import PaDTForConditionalGeneration  # noqa: E402
from padt_amd.synthetic import rec_schedule  # noqa: E402
from bench_shared_prefix import make_case  # noqa: E402


def prefix_rows(cfg, shared, n_images):
    """The prefix of image u: the row of its first query up to and including the last image token."""
    ids = shared["input_ids"].cpu()
    rows = []
    for u in range(n_images):
        r = ids[shared["image_index"].index(u)].tolist()
        rows.append(r[: len(r) - r[::-1].index(cfg.image_token_id)])
    t = torch.tensor(rows)
    return t.cuda(), torch.ones_like(t).cuda()


def kernel_alone(model, handle, batch, n_images, reps):
    cfg = model.config
    Hkv, hd = cfg.num_key_value_heads, cfg.head_dim
    P = handle.lens[0]
    s_max = (P + 64 + 63) // 64 * 64
    packed = hd == 128
    dt = handle.dtype
    kc = torch.zeros((batch, Hkv, s_max, hd), device="cuda", dtype=dt)
    vt = torch.zeros((batch, Hkv, hd, s_max), device="cuda", dtype=dt)
    kj, vj = (torch.zeros((batch * (P + 33), Hkv * hd), device="cuda", dtype=dt) for _ in range(2))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    mem = (i32([b % n_images for b in range(batch)]), i32(list(range(batch))), i32([b * (P + 33) for b in range(batch)]))
    written = 4 * batch * P * Hkv * hd * kc.element_size()        # K and V, each to a cache image and to join rows
    src = torch.zeros(written, device="cuda", dtype=torch.uint8)
    dst = torch.empty_like(src)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps
    us_k = timed(lambda: ops.kv_prefix_fanout(handle.k[0], handle.v[0], handle.pre_off, *mem, P, kc, vt, kj, vj, Hkv, hd, s_max, cache_packed=packed))
    us_c = timed(lambda: dst.copy_(src))
    print(json.dumps({"kernel": "padt_kv_prefix_fanout", "members": batch, "images": n_images, "P": P, "kv_heads": Hkv, "head_dim": hd,
                      "cache_packed": packed, "bytes_written": written, "bytes_read": 2 * n_images * P * Hkv * hd * kc.element_size(),
                      "fanout_us": round(us_k, 2), "d2d_copy_same_bytes_us": round(us_c, 2), "fanout_over_copy": round(us_k / us_c, 3),
                      "written_GBps": round(written / us_k / 1e3, 1), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--distinct", default="8,4,2,1", help="distinct images per batch, one case each")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=7, help="timed calls of each variant per case (at least 5)")
    ap.add_argument("--reps", type=int, default=200, help="launches per timing of the kernel alone")
    ap.add_argument("--tnew", type=int, default=28)
    ap.add_argument("--model", default="3b", choices=["3b", "small"])
    ap.add_argument("--operands", default="auto", choices=["auto", "fp16", "bf16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix_cache.py times generate() on an MI355X: no GPU found")
    if args.calls < 5:
        raise SystemExit("--calls must be at least 5")
    cfg = {"3b": padt_amd.padt_pro_3b, "small": padt_amd.small_test_config}[args.model]()
    grid_hw = (10, 12) if args.model == "small" else (46, 46)
    model = PaDTForConditionalGeneration.from_synthetic(cfg, seed=0, device="cuda", operands=args.operands)
    T = args.tnew
    gen = dict(max_new_tokens=T, schedule=rec_schedule(T, range(11, 16)), do_sample=False, sync_every=T)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    handle = n_images = None
    for n_images in (int(x) for x in args.distinct.split(",")):
        shared, expanded = make_case(cfg, grid_hw, args.batch, n_images, seed=1000 + n_images)
        pre_ids, pre_am = prefix_rows(cfg, shared, n_images)
        build = lambda: model.encode_prefix(pre_ids, pre_am, shared["pixel_values"], shared["image_grid_thw"])
        _, handle = clock(build)                                  # warm-up: plans
        cached = dict(input_ids=shared["input_ids"], attention_mask=shared["attention_mask"], prefix=handle, image_index=shared["image_index"])
        variants = {"prefix": cached, "image_index": shared, "expanded": expanded}
        outs = {k: clock(lambda kw=kw: model.generate(**gen, **kw))[1] for k, kw in variants.items()}      # warm-up: sessions, the captured step
        ms = {k: [] for k in variants}
        for _ in range(args.calls):
            for k, kw in variants.items():
                ms[k].append(clock(lambda kw=kw: model.generate(**gen, **kw))[0])
        enc = [clock(build)[0] for _ in range(args.calls)]
        plan = padt_amd.llm.plan_prompt_prefix(cfg, cached["input_ids"], cached["attention_mask"], handle, cached["image_index"], "cpu")
        plan_s = padt_amd.llm.plan_prompt_shared(cfg, shared["input_ids"], shared["attention_mask"], shared["image_grid_thw"],
                                                 shared["image_index"], "cpu")
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = {"model": args.model, "operands": "fp16" if model.dtype == torch.float16 else "bf16", "handle_operands": str(handle.dtype),
               "batch": args.batch, "distinct_images": n_images, "L": int(shared["input_ids"].shape[1]), "P": handle.lens[0], "T": T,
               "calls": args.calls, "prompt_rows_prefix": int(plan.shared.ids.numel()), "prompt_rows_image_index": int(plan_s.shared.ids.numel()),
               "prompt_rows_expanded": int(plan.ids.numel()), "handle_MB": round(handle.nbytes / 2 ** 20, 1)}
        for k, v in ms.items():
            rec.update({f"{k}_ms_median": round(med[k], 2), f"{k}_ms_min": round(min(v), 2), f"{k}_ms_max": round(max(v), 2)})
        rec.update({"encode_prefix_ms_median": round(statistics.median(enc), 2), "encode_prefix_ms_min": round(min(enc), 2),
                    "encode_prefix_ms_max": round(max(enc), 2), "speedup_vs_image_index": round(med["image_index"] / med["prefix"], 3),
                    "speedup_vs_expanded": round(med["expanded"] / med["prefix"], 3),
                    "same_sequences_as_image_index": bool(torch.equal(outs["prefix"].sequences, outs["image_index"].sequences)),
                    "same_sequences_as_expanded": bool(torch.equal(outs["prefix"].sequences, outs["expanded"].sequences))})
        print(json.dumps(rec), flush=True)
    kernel_alone(model, handle, args.batch, n_images, args.reps)


if __name__ == "__main__":
    main()
