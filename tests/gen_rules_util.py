"""Shared by test_gen_rules_cpu.py / test_gen_rules_gpu.py: the reference of the device-side bans — the installed HF logits-processor
classes applied to a zero row (the ban set is where they return -inf) — a host model of padt_gen_rules over the packed rule table, and the
seeded random rule sets of the kernel tests."""
import random

import torch

KINDS = ("ngram", "bad_words", "suppress", "begin")


def hf_processors(rules, eos_ids, begin_index, device="cpu", kinds=KINDS):
    """rules: dict(no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens) → HF's processors for them, in the order
    GenerationMixin._get_logits_processor builds them; begin_index = the prompt length (padt.py:570-580)."""
    from transformers.generation import logits_process as lp
    out = []
    if "ngram" in kinds and rules.get("no_repeat_ngram_size"):
        out.append(lp.NoRepeatNGramLogitsProcessor(rules["no_repeat_ngram_size"]))
    if "bad_words" in kinds and rules.get("bad_words_ids"):
        out.append(lp.NoBadWordsLogitsProcessor(rules["bad_words_ids"], list(eos_ids)))
    if "suppress" in kinds and rules.get("suppress_tokens"):
        out.append(lp.SuppressTokensLogitsProcessor(rules["suppress_tokens"], device=device))
    if "begin" in kinds and rules.get("begin_suppress_tokens"):
        out.append(lp.SuppressTokensAtBeginLogitsProcessor(rules["begin_suppress_tokens"], begin_index, device=device))
    return out


def hf_ban(rules, eos_ids, history, begin_index, width, kinds=KINDS):
    """history: one row's ids (prompt + generated so far) → bool (width,): the columns HF's processors set to -inf on a zero row."""
    ids = torch.tensor([list(history)], dtype=torch.long)
    sc = torch.zeros((1, width))
    for p in hf_processors(rules, eos_ids, begin_index, kinds=kinds):
        sc = p(ids, sc)
    assert bool(((sc == 0) | (sc == float("-inf"))).all())
    return sc[0] == float("-inf")


def table_ban(table, history, t, width):
    """Host model of padt_gen_rules: the packed table (ops.gen_rules_tensor) on one row's history at step t → bool (width,)."""
    r = table.tolist()
    n, ns, nb, nw = r[:4]
    h, cur = list(history), len(history)
    out = torch.zeros(width, dtype=torch.bool)

    def ban(i):
        if 0 <= i < width:
            out[i] = True
    for i in r[4: 4 + ns]:
        ban(i)
    if t == 0:
        for i in r[4 + ns: 4 + ns + nb]:
            ban(i)
    for o in r[4 + ns + nb: 4 + ns + nb + nw]:
        m = r[o]
        wd = r[o + 1: o + 1 + m]
        if cur >= m and h[cur - (m - 1):] == wd[:-1]:
            ban(wd[-1])
    if n > 0 and cur + 1 >= n:
        last = h[cur - (n - 1):] if n > 1 else []
        for i in range(0, cur - n + 1):
            if h[i: i + n - 1] == last:
                ban(h[i + n - 1])
    return out


def bitmap_to_bool(words, width):
    """int32 (rows, n_words) bitmap → (bool (rows, width), bool: no bit at or past `width` is set)."""
    w = words.cpu().to(torch.int64) & 0xFFFFFFFF
    bits = ((w[:, :, None] >> torch.arange(32)) & 1).bool().reshape(w.shape[0], -1)
    return bits[:, :width], not bool(bits[:, width:].any())


# ---- the seeded random cases of the kernel tests: 5 rows over a table of 96 text rows + ragged prototypes (width 113: no multiple of 32)
V = 96
PROTO_COUNTS = (3, 5, 2, 4, 3)
WIDTH = V + sum(PROTO_COUNTS)
TEXT = (3, 17, 31, 64, 95)             # the 5 text ids of the histories (31 / 64: both sides of a bitmap word boundary; 95: the last text row)
VRT = (V + 1, WIDTH - 1)               # ... and 2 VRT ids (the last column of the table among them)
EOS = (17,)
HIST_LENS = (1, 7, 40)
STEPS = (0, 1, 2, 9)
N_CASES = 60


def random_case(seed):
    """→ (rules dict, hist_len per row, t, tokens per row (t ids), prompts per row)."""
    g = random.Random(seed)
    alpha = TEXT + VRT
    t = STEPS[seed % 4]
    rules = dict(no_repeat_ngram_size=g.choice((0, 1, 2, 2, 3, 4)),
                 bad_words_ids=[[g.choice(TEXT) for _ in range(g.choice((1, 2, 2, 3)))] for _ in range(g.choice((0, 2, 4, 6)))],
                 suppress_tokens=g.sample(range(V), g.choice((0, 1, 3))),
                 begin_suppress_tokens=g.sample(range(V), g.choice((1, 2, 5))) if t == 0 else g.sample(range(V), g.choice((0, 2))))
    lens = [g.choice(HIST_LENS) for _ in PROTO_COUNTS]
    prompts = [[g.choice(alpha) for _ in range(l)] for l in lens]
    tokens = [[g.choice(alpha) for _ in range(t)] for _ in PROTO_COUNTS]
    return rules, lens, t, tokens, prompts
