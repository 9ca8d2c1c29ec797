"""Shared by test_token_automaton_cpu.py / test_token_automaton_gpu.py: the shapes of the kernel-level cases (a 1003-column text table, three
rows with patch ranges [0, 5), [5, 5) and [5, 42)), seeded random automata and token histories, the specification `TokenAutomaton.allowed()`
as a ban row and as the function HF's PrefixConstrainedLogitsProcessor takes."""
import random

import torch

from padt_amd.generation import TokenAutomaton as TA

V = 1003                                    # text columns: not a multiple of 32
VRT_OFF = [0, 5, 5, 42]                     # row 0: patches [0, 5) — ends inside a word; row 1: none; row 2: [5, 42) — starts and ends inside words
N_COLS = V + VRT_OFF[-1]                    # 1045 = 32 * 32 + 21
WORDS = (N_COLS + 31) // 32
EOS_LISTS = ([77], [77, 1002, 0, 500])      # 1 and 4 ids; the first and the last text column among them
N_STATES = 40
BIG_STATE, VRT_ONLY_STATE = 3, 5            # a state with more than 300 explicit edges, a state whose only edge is VRT
HISTORY_LENGTHS = (0, 1, 2, 70)


def random_automaton(seed, eos=()):
    """About 40 states + one terminal state, every state with explicit ids and / or classes; explicit ids include EOS ids now and then (the
    explicit-over-class rule and the carve-out meet)."""
    rng = random.Random(seed)
    term = N_STATES
    table = []
    for s in range(N_STATES):
        edges = {}
        if s == VRT_ONLY_STATE:
            edges[TA.VRT] = rng.randrange(N_STATES)
        else:
            n_explicit = 320 if s == BIG_STATE else rng.choice((0, 1, 2, 3, 6))
            ids = rng.sample(range(V), n_explicit)
            if eos and rng.random() < 0.4:
                ids.append(rng.choice(list(eos)))
            if s % 7 == 1:
                ids += [0, 31, 32, V - 1]                                       # word edges and the last text column
            for i in ids:
                edges[i] = rng.randrange(N_STATES)
            for cls in (TA.VRT, TA.TEXT, TA.EOS):
                if rng.random() < 0.45:
                    edges[cls] = term if cls == TA.EOS else rng.randrange(N_STATES)
            if not edges:
                edges[TA.TEXT] = rng.randrange(N_STATES)
        table.append(list(edges.items()))
    table.append([])
    return TA(table, start=rng.randrange(N_STATES))


def random_history(seed, A, length, vrt_range, eos):
    """`length` tokens: mostly allowed ones (EOS avoided while something else is allowed, so the walk goes on), now and then any column."""
    rng = random.Random(seed)
    toks, state = [], A.start
    for _ in range(length):
        ok = A.allowed_in(state, V, vrt_range, eos)
        live = [c for c in ok if c not in eos] or ok
        tok = rng.choice(live) if rng.random() < 0.93 else rng.randrange(N_COLS)
        toks.append(tok)
        state = A.step(state, tok, V, vrt_range, eos)
    return toks


def ban_row(A, tokens, vrt_range, eos, width=N_COLS, n_text=V):
    """the specification as the kernel's output: bool (width,), True = banned"""
    row = torch.ones(width, dtype=torch.bool)
    row[torch.tensor(A.allowed(tokens, n_text, vrt_range, eos), dtype=torch.long)] = False
    return row


def bitmap_to_bool(ban, width):
    """int32 (B, words) bitmap → (bool (B, width), True when every bit past `width` is clear)"""
    w = ban.detach().cpu().to(torch.int64) & 0xFFFFFFFF
    bits = ((w[:, :, None] >> torch.arange(32)) & 1).bool().reshape(w.shape[0], -1)
    return bits[:, :width], not bool(bits[:, width:].any())


def prefix_fn(A, prompt_len, n_text, vrt_ranges, eos):
    """`allowed()` as HF's prefix_allowed_tokens_fn(batch_id, input_ids): the generated part is what follows the prompt"""
    def fn(batch_id, input_ids):
        return A.allowed([int(t) for t in input_ids[prompt_len:].tolist()], n_text, vrt_ranges[batch_id], eos)
    return fn


def label_automaton(labels, n_vrt=3, repeat=True):
    """the OVD shape: one of the labels, then n_vrt of the row's own patches, then EOS or (repeat) another label"""
    return TA.from_sequences([list(lb) + [TA.VRT] * n_vrt for lb in labels], repeat=repeat)
