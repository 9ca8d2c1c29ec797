"""Time the captured decode step of generate(beam_width=K) next to the greedy step at the same row count, and padt_beam_reorder_kv alone.

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built by tools/step_bench.py (seeded random
16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass); rows = queries x `--width` beams.  The step's hipGraph is
captured once per mode:

  plain      the step as generate() runs it by default: padt_vrt_head with the fused arg-max, padt_greedy_step.  It uses nothing this feature
             added, so the script also runs in a tree without it (--modes plain): THAT run is the yardstick of the off path — the new build's
             `plain` is compared with the parent commit's `plain` of the same session, never with itself
  beam_step  the beam step without the cache move: the head writes the fp32 row, padt_topk_logprob_rows_f32 (k = 2 x width),
             padt_beam_step; padt_beam_reorder_kv is not launched, so the rows' caches do NOT follow the beams — a timing mode only.
             The switch is this tool's own (CacheMove below): it stands in front of ops.beam_reorder_kv, counts what reaches it, and the
             script asserts after every capture that the session went through it (no launch in this mode, launches in the others)
  beam       the step as generate(beam_width=) runs it: ... and padt_beam_reorder_kv over all layers
  beam_lp    ... with output_token_logprobs=True: the LSE head and padt_beam_cand_lp (the reported log-probs are the greedy step's fold)

Early stopping is "never" and the call longer than a window, so no query is done inside one (asserted).  `beam` reports how many of a
window's (step, query) pairs moved their caches.

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Prints one JSON line per (rows, mode).

Every mode has a graph table of its own (the session's `graphs` is pointed at it), so two launch lists under one step mode never meet.

Then the kernel alone: a 3-cycle among every query's first three beams (3 of 4 rows are written at width 4), `--generated` tokens behind
`--context`, the grid sized for the largest of them (a session's grid is sized for its t_max: see profiles/beam_search.md),
by device events over `--reps` launches, against a device-to-device copy of the byte count it WRITES, in the same process.  That copy is its
yardstick; the ratio is reported, not judged.

usage: python tools/bench_beam_search.py [--rows 32,64] [--width 4] [--modes plain,beam_step,beam,beam_lp] [--generated 16,64,128] [--tag T]"""
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from padt_amd import ops  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

MODES = ("plain", "beam_step", "beam", "beam_lp")


class CacheMove:
    """The tool's switch in front of ops.beam_reorder_kv: on — the kernel, off — nothing; either way it counts the calls that reached it,
    so that a session that stopped looking the function up through `ops` is noticed instead of timed."""

    def __init__(self):
        self.kernel, self.on, self.calls = ops.beam_reorder_kv, True, 0
        ops.beam_reorder_kv = self

    def __call__(self, *a, **k):
        self.calls += 1
        if self.on:
            self.kernel(*a, **k)

    def remove(self):
        ops.beam_reorder_kv = self.kernel


def time_rows(cfg, rows, op16, modes, args, device):
    K = args.width
    if rows % K:
        raise SystemExit(f"--rows {rows} is not a multiple of --width {K}")
    bench = StepBench(cfg, rows, op16, args, device)
    sess = bench.sess
    move = CacheMove() if hasattr(ops, "beam_reorder_kv") else None      # a tree without the feature: plain only
    moved, graphs = {}, {}

    def set_mode(mode):
        opts = GenOptions(eos_ids=(int(cfg.eos_token_id),))
        sess.graphs = graphs.setdefault(mode, {})             # beam_step and beam are one step mode: every mode keeps its own captures
        if mode != "plain":
            opts = dataclasses.replace(opts, beam=(K, 1, 1.0, "never"), token_logprobs=mode == "beam_lp")
            move.on, move.calls = mode != "beam_step", 0
        sess.begin(opts)
        if mode != "plain":
            bench.fake_batch(opts)

    def check(mode, _):
        if mode != "plain":
            assert bool(sess.unfinished.all()), f"mode {mode}: a query was done inside the window"
            assert move.calls > 0, f"mode {mode}: the session did not reach the cache-move switch"      # the eager step and the capture pass
            par = sess.beam.beam_parent[: bench.n_chk].view(bench.n_chk, rows // K, K).cpu()
            ident = (par == torch.arange(K)).all(-1)
            moved[mode] = round(1.0 - float(ident.float().mean()), 3)

    try:
        bench.capture(modes, set_mode, check)
        us = bench.time(modes, set_mode)
    finally:
        if move is not None:
            move.remove()
    return [bench.record(mode, us[mode], **({"width": K, "queries": rows // K, "moved_fraction_first_steps": moved.get(mode)} if mode != "plain" else {}))
            for mode in modes]


def kernel_alone(cfg, rows, K, op16, context, generated, reps, tag):
    Hkv, hd, nl = cfg.num_key_value_heads, cfg.head_dim, cfg.num_hidden_layers
    s_max = (context + max(generated) + 63) // 64 * 64
    kc = [torch.zeros((rows, Hkv, s_max, hd), device="cuda", dtype=op16) for _ in range(nl)]
    vt = [torch.zeros((rows, Hkv, hd, s_max), device="cuda", dtype=op16) for _ in range(nl)]
    table = ops.beam_kv_table(kc, vt)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    cyc = [1, 2, 0] + list(range(3, K)) if K >= 3 else [1, 0][:K]
    perm, p0 = i32(cyc * (rows // K)), i32([context] * rows)

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
    for n in generated:
        slot = i32([context + n] * rows)
        tiles = lambda w: (context + n - 1) // w - context // w + 1
        n_moved = sum(1 for c, p in enumerate(cyc) if c != p) * (rows // K)
        written = n_moved * nl * Hkv * hd * 2 * (16 * tiles(16) + 32 * tiles(32))
        src = torch.zeros(written, device="cuda", dtype=torch.uint8)
        dst = torch.empty_like(src)
        us_k = timed(lambda: ops.beam_reorder_kv(table, perm, p0, slot, rows // K, K, Hkv, hd, s_max, max(generated)))
        us_c = timed(lambda: dst.copy_(src))
        rec = {"kernel": "padt_beam_reorder_kv", "rows": rows, "width": K, "layers": nl, "kv_heads": Hkv, "head_dim": hd, "context": context,
               "generated": n, "rows_written": n_moved, "bytes_written": written, "bytes_read": rows * written // max(n_moved, 1),
               "reorder_us": round(us_k, 2), "d2d_copy_same_bytes_us": round(us_c, 2), "reorder_over_copy": round(us_k / us_c, 3),
               "written_GBps": round(written / us_k / 1e3, 1), "reps": reps}
        print(json.dumps(dict(rec, tag=tag) if tag else rec), flush=True)


if __name__ == "__main__":
    ap = parser(__doc__, MODES, tag=True)
    ap.set_defaults(rows="32,64")
    ap.add_argument("--width", type=int, default=4, help="beams per query")
    ap.add_argument("--generated", default="16,64,128", help="generated tokens per row for the timings of the reorder kernel alone ('' skips them)")
    ap.add_argument("--reps", type=int, default=200, help="launches per timing of the kernel alone")
    main(ap, MODES, time_rows)
    args = ap.parse_args()
    if args.generated and "beam" in args.modes.split(","):
        from padt_amd import config
        for r in (int(x) for x in args.rows.split(",")):
            kernel_alone(config.padt_pro_3b(), r, args.width, torch.float16 if args.operands == "fp16" else torch.bfloat16, args.context,
                         [int(x) for x in args.generated.split(",")], args.reps, args.tag)
