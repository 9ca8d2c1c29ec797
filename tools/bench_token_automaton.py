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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataclasses  # noqa: E402
import random  # noqa: E402

import torch  # noqa: E402

from padt_amd import ops  # noqa: E402
from padt_amd.generation import GenOptions  # noqa: E402
from step_bench import StepBench, main, parser  # noqa: E402

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
    bench = StepBench(cfg, rows, op16, args, device, np_max=rows * args.patches)
    sess, gen = bench.sess, bench.gen
    ids = torch.randint(0, cfg.vocab_size, (40,), generator=gen, device=device).tolist()
    prompt = torch.randint(0, cfg.vocab_size, (rows, args.context), generator=gen, device=device).to(torch.int32)
    bench.random_prototypes(gen)
    vrt_off = [b * args.patches for b in range(rows + 1)]        # every row owns `patches` prototype rows, in every mode
    rules = {"ngram3": ops.gen_rules_key(3, vocab_size=cfg.vocab_size),
             "bans": ops.gen_rules_key(3, [ids[2 * i: 2 * i + 2] for i in range(8)], ids[16: 32], vocab_size=cfg.vocab_size)}
    rules["automaton_bans"] = rules["bans"]
    trie = coco_sized_trie(cfg) if any(m.startswith("automaton") for m in modes) else None

    def set_mode(mode):
        opts = GenOptions(rules=rules.get(mode))
        if mode.startswith("automaton"):
            opts = dataclasses.replace(opts, automaton=trie.key)
            sess.begin(opts, automaton=trie)
        else:
            sess.begin(opts)
        bench.fake_batch(opts, vrt_off=vrt_off, prompt_ids=prompt if opts.rules is not None else None)

    def check(mode, tok):
        if mode.startswith("automaton"):                          # what was emitted is on the automaton, row by row
            for b, row in enumerate(tok.tolist()):
                assert trie.accepts(row, cfg.vocab_size, (b * args.patches, (b + 1) * args.patches), ()), f"mode {mode}: row {b} left the automaton: {row}"

    bench.capture(modes, set_mode, check)
    us = bench.time(modes, set_mode)
    out = []
    for mode in modes:
        out.append(bench.record(mode, us[mode], patches_per_row=args.patches))
        if trie is not None and mode.startswith("automaton"):
            out[-1].update(states=len(trie.edges), edges=sum(len(e) for e in trie.edges))
    return out


if __name__ == "__main__":
    ap = parser(__doc__, MODES, tag=True)
    ap.add_argument("--patches", type=int, default=8, help="prototype rows (VRT columns) per session row")
    main(ap, MODES, time_rows)
