"""Time the captured decode step with generate(token_automaton=...) next to the steps it is derived from.

One DecodeSession (padt_amd/llm.py) per row count at the PaDT_Pro_3B LLM shape, full depth, built like tools/bench_forced_tokens.py builds it
(seeded random 16-bit weight images, `--context` cached tokens per row, no ViT / prompt pass); every row owns `--patches` prototype rows, so
the VRT class has columns to allow.  The step's hipGraph is captured once per mode:

  plain             the step as generate() runs it by default: logit head with the fused arg-max, padt_greedy_step
  ngram3            no_repeat_ngram_size=3 over a `--context`-token prompt: padt_gen_rules + the head reading its bitmap
  bans              the four bans (n-gram 3, eight 2-token bad words, sixteen suppressed ids): the same two kernels, a fuller table
  automaton         token_automaton = a COCO-80-sized trie (80 seeded labels of 2-4 text ids, five VRTs each, repeat=True):
                    padt_token_automaton + the head reading its bitmap
  automaton_bans    the trie plus the four bans: padt_gen_rules, padt_token_automaton (which ORs the rules' bitmap in), the head

The options carry no EOS id, so no row finishes inside a window: every step pays for every row.  The automaton modes must emit sequences
the Python walker accepts.  `plain`, `ngram3` and `bans` use nothing this feature added, so the script also runs in a tree without it
(--modes plain,ngram3,bans).

Timing: `--warmup` replays per mode, then `--repeats` rounds; a round times one window of `--steps` replays between two device events for EVERY
mode in turn (the modes alternate, so drift of the machine hits them alike).  Per mode the median window is reported with the extremes and every
window's value.  Prints one JSON line per (rows, mode).

usage: python tools/bench_token_automaton.py [--rows 8,64] [--modes plain,ngram3,bans,automaton,automaton_bans] [--operands fp16|bf16]"""
import argparse
import dataclasses
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from padt_amd import config, ops  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from padt_amd.llm import DecodeSession  # noqa: E402
from padt_amd.weights import _pad_to  # noqa: E402
from bench_decode_weights import build_weights  # noqa: E402

MODES = ("plain", "ngram3", "bans", "automaton", "automaton_bans")


def coco_sized_trie(cfg, n_labels=80, n_vrt=5, seed=80):
    """80 labels of 2-4 distinct text ids each (no label a prefix of another), five of the row's own patches after each, then EOS or the next label"""
    from padt_amd.generation import TokenAutomaton
    rng = random.Random(seed)
    hi = min(cfg.vocab_size, cfg.image_token_id)
    firsts = rng.sample(range(hi), n_labels // 2)                   # two labels per first token: the trie branches at depth 1 too
    labels = []
    for f in firsts:
        for second in rng.sample(range(hi), 2):
            labels.append([f, second] + rng.sample(range(hi), rng.randrange(0, 3)))
    return TokenAutomaton.from_sequences([lb + [TokenAutomaton.VRT] * n_vrt for lb in labels], repeat=True)


def time_rows(cfg, rows, op16, modes, args, device):
    W, wbytes = build_weights(cfg, "bf16", op16, device)
    window = max(args.steps, args.warmup)
    sess = DecodeSession(cfg, W, rows, _pad_to(args.context + window + 1, 64), rows * args.patches, window + 1, device)
    gen = torch.Generator(device=device).manual_seed(1)
    first = torch.randint(0, cfg.vocab_size, (rows,), generator=gen, device=device)
    ids = torch.randint(0, cfg.vocab_size, (40,), generator=gen, device=device).tolist()
    prompt = torch.randint(0, cfg.vocab_size, (rows, args.context), generator=gen, device=device).to(torch.int32)
    sess.proto.copy_((torch.randn(sess.proto.shape, generator=gen, device=device) * 0.02).to(op16))
    vrt_off = (torch.arange(rows + 1, device=device) * args.patches).to(torch.int32)
    rules = {"ngram3": ops.gen_rules_key(3, vocab_size=cfg.vocab_size),
             "bans": ops.gen_rules_key(3, [ids[2 * i: 2 * i + 2] for i in range(8)], ids[16: 32], vocab_size=cfg.vocab_size)}
    rules["automaton_bans"] = rules["bans"]
    trie = coco_sized_trie(cfg) if any(m.startswith("automaton") for m in modes) else None

    def set_mode(mode):
        opts = GenOptions(rules=rules.get(mode))
        if mode.startswith("automaton"):
            sess.begin(dataclasses.replace(opts, automaton=trie.key), automaton=trie)
        else:
            sess.begin(opts)
        if opts.rules is not None:
            sess.hist[:, : args.context] = prompt
            sess.hist_len.fill_(args.context)

    def reset():
        """`context` cached tokens per row, step counter at zero: every window replays the same steps (never past s_max / t_max)"""
        sess.step.zero_()
        sess.unfinished.fill_(1)
        sess.cur_tok.copy_(first)
        sess.slot.fill_(args.context)
        sess.lens.fill_(args.context)
        sess.pos3.fill_(args.context)
        sess.vrt_off.copy_(vrt_off)

    n_chk = max(args.warmup, 2)
    for mode in modes:                                            # one eager step, the capture, then replays — per mode
        set_mode(mode)
        reset()
        sess.run_steps(n_chk)
        torch.cuda.synchronize()
        if mode.startswith("automaton"):                          # what was emitted is on the automaton, row by row
            tok = sess.tokens[:, :n_chk].tolist()
            for b, row in enumerate(tok):
                assert trie.accepts(row, cfg.vocab_size, (b * args.patches, (b + 1) * args.patches), ()), f"mode {mode}: row {b} left the automaton: {row}"
    us = {m: [] for m in modes}
    for _ in range(args.repeats):
        for mode in modes:
            set_mode(mode)
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            sess.run_steps(args.steps)
            e1.record()
            torch.cuda.synchronize()
            us[mode].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    out = []
    for mode in modes:
        med = statistics.median(us[mode])
        out.append({"model": "PaDT_Pro_3B", "mode": mode, "rows": rows, "layers": cfg.num_hidden_layers, "operands": str(op16).split(".")[-1],
                    "context": args.context, "patches_per_row": args.patches, "us_per_step": round(med, 1), "us_min": round(min(us[mode]), 1),
                    "us_max": round(max(us[mode]), 1), "windows": [round(u, 1) for u in us[mode]], "steps_per_window": args.steps,
                    "weight_bytes": int(wbytes)})
        if trie is not None and mode.startswith("automaton"):
            out[-1].update(states=len(trie.edges), edges=sum(len(e) for e in trie.edges))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="8,64")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--operands", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--context", type=int, default=512, help="cached tokens per row when a window starts (and the n-gram ban's prompt length)")
    ap.add_argument("--patches", type=int, default=8, help="prototype rows (VRT columns) per session row")
    ap.add_argument("--steps", type=int, default=64, help="graph replays per timed window")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--tag", default="", help="copied into every JSON line (which tree / which run)")
    args = ap.parse_args()
    modes = args.modes.split(",")
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode '{m}'")
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_automaton.py times kernels on an MI355X: no GPU found")
    device = torch.device("cuda:0")
    op16 = torch.float16 if args.operands == "fp16" else torch.bfloat16
    cfg = config.padt_pro_3b()
    for rows in (int(r) for r in args.rows.split(",")):
        for res in time_rows(cfg, rows, op16, modes, args, device):
            print(json.dumps(dict(res, tag=args.tag) if args.tag else res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
