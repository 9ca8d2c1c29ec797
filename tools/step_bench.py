"""What the step benchmarks (tools/bench_*.py over a DecodeSession's captured decode step) share: the seeded weight images, the session, the
window rewind, capture and timed windows per step mode, the JSON record and the command line.  A script keeps its docstring, its MODES, a
`set_mode` that states the mode through the session's own methods (DecodeSession.begin / add_batch, never by writing its buffers) and its
own assertions."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from padt_amd import config, ops  # noqa: E402
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


class StepBench:
    """One DecodeSession of `rows` rows at cfg's LLM shape, full depth, over seeded random weight images, sized for windows of
    max(--steps, --warmup) steps behind `--context` cached tokens per row; no ViT, no prompt pass."""

    def __init__(self, cfg, rows, op16, args, device, np_max=16, weights="bf16"):
        self.cfg, self.rows, self.op16, self.args = cfg, rows, op16, args
        self.W, self.wbytes = build_weights(cfg, weights, op16, device)
        window = max(args.steps, args.warmup)
        self.sess = DecodeSession(cfg, self.W, rows, _pad_to(args.context + window + 1, 64), np_max, window + 1, device)
        self.gen = torch.Generator(device=device).manual_seed(1)      # a script's further seeded draws continue it
        self.first = torch.randint(0, cfg.vocab_size, (rows,), generator=self.gen, device=device)
        self.n_chk = max(args.warmup, 2)

    def random_prototypes(self, generator):
        """Seeded prototype rows — what the ViT and the prototype projection leave in a generate(), model output like the weights —
        for the scripts whose rows own patch columns"""
        p = self.sess.proto
        p.copy_(torch.randn(p.shape, generator=generator, device=p.device) * 0.02)

    def fake_batch(self, opts, vrt_off=None, **state):
        """One batch over all the session's rows, as generate() would add it after `--context` prompt tokens (vrt_off: the rows' patch
        offsets, default no row owns a patch; state: add_batch's other per-batch values)."""
        c = self.args.context
        self.sess.add_batch(opts, 0, 0, [0] * (self.rows + 1) if vrt_off is None else vrt_off, [c] * self.rows, [c] * self.rows, **state)

    def rewind(self):
        """`context` cached tokens per row, step counter at zero: every window replays the same steps (never past s_max / t_max).  This is
        the benchmark's own state, not generate()'s — there a row with `context` prompt tokens sees context + 1 keys (DecodeSession.add_batch)
        and starts from its prompt's last hidden row; here every row re-reads the same cached slots from a seeded token, window after
        window — so it is written here, once, and nowhere else."""
        s, c = self.sess, self.args.context
        s.step.zero_()
        s.unfinished.fill_(1)
        s.cur_tok.copy_(self.first)
        s.slot.fill_(c)
        s.lens.fill_(c)
        s.pos3.fill_(c)

    def capture(self, modes, set_mode, check=None):
        """Per mode: one eager step, the capture, then replays → {mode: the tokens of the first n_chk steps}.  check(mode, tokens) runs while
        the session still holds what the mode left."""
        tokens = {}
        for mode in modes:
            set_mode(mode)
            self.rewind()
            self.sess.run_steps(self.n_chk)
            torch.cuda.synchronize()
            tokens[mode] = self.sess.tokens[:, : self.n_chk].clone()
            if check is not None:
                check(mode, tokens[mode])
        return tokens

    def time(self, modes, set_mode):
        """--repeats rounds; a round times one window of --steps replays between two device events for EVERY mode in turn (the modes
        alternate, so drift of the machine hits them alike) → {mode: us per step of every window}"""
        us = {m: [] for m in modes}
        for _ in range(self.args.repeats):
            for mode in modes:
                set_mode(mode)
                self.rewind()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                self.sess.run_steps(self.args.steps)
                e1.record()
                torch.cuda.synchronize()
                us[mode].append(e0.elapsed_time(e1) * 1e3 / self.args.steps)
        return us

    def record(self, mode, us, **extra):
        """The JSON record of one (rows, mode): the median window with the extremes and every window's value"""
        return {"model": "PaDT_Pro_3B", "mode": mode, "rows": self.rows, "layers": self.cfg.num_hidden_layers, "operands": str(self.op16).split(".")[-1],
                "context": self.args.context, "us_per_step": round(statistics.median(us), 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                "windows": [round(u, 1) for u in us], "steps_per_window": self.args.steps, "weight_bytes": int(self.wbytes), **extra}


def parser(doc, modes=None, steps=64, repeats=9, tag=False):
    """The scripts' common command line; a script adds its own arguments to what this returns"""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="8,64")
    if modes is not None:
        ap.add_argument("--modes", default=",".join(modes))
    ap.add_argument("--operands", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--context", type=int, default=512, help="cached tokens per row when a window starts")
    ap.add_argument("--steps", type=int, default=steps, help="graph replays per timed window")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=repeats)
    if tag:
        ap.add_argument("--tag", default="", help="copied into every JSON line (which tree / which run)")
    return ap


def gpu_or_exit(args):
    """→ (device, 16-bit operand type), or the exit of a machine without a GPU"""
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(sys.argv[0])} times kernels on an MI355X: no GPU found")
    return torch.device("cuda:0"), torch.float16 if args.operands == "fp16" else torch.bfloat16


def main(ap, known_modes, time_rows):
    """Parse, check the modes, and print one JSON line per (rows, mode) of time_rows(cfg, rows, op16, modes, args, device) at the 3B shape"""
    args = ap.parse_args()
    modes = args.modes.split(",")
    for m in modes:
        if m not in known_modes:
            raise SystemExit(f"unknown mode '{m}'")
    device, op16 = gpu_or_exit(args)
    cfg = config.padt_pro_3b()
    tag = getattr(args, "tag", "")
    for rows in (int(r) for r in args.rows.split(",")):
        for res in time_rows(cfg, rows, op16, modes, args, device):
            print(json.dumps(dict(res, tag=tag) if tag else res), flush=True)
        torch.cuda.empty_cache()
