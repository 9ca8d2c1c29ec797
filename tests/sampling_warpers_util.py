"""Shared by tests/test_sampling_warpers_cpu.py and tests/test_sampling_warpers_gpu.py: an fp64 reference of HF's warpers after top-p
(MinP → Typical → Epsilon → Eta, generation/logits_process.py, min_tokens_to_keep = 1), HF's own classes in the same order, and the rows and
settings both files test on."""
import math

import torch

BAND = 1e-5                      # the band tests/test_token_selection_gpu.py::ref_warp uses for the nucleus
AMBIGUOUS_MAX = 4                # entries a test may excuse per row at n <= 3000 ...
AMBIGUOUS_MAX_FULL = 16          # ... and at full width
OFF = dict(min_p=0.0, typical_p=1.0, eps=0.0, eta=0.0)
SINGLE = [dict(min_p=0.05), dict(min_p=0.5), dict(typical_p=0.9), dict(typical_p=0.2), dict(eps=3e-4), dict(eps=0.05), dict(eta=3e-4),
          dict(eta=0.05)]
COMBINED = dict(min_p=0.02, typical_p=0.95, eps=1e-4, eta=2e-3)
WIDTHS = (1, 1023, 1025, 3000)
FULL_WIDTH = 156000


def setting_id(s):
    return "-".join(f"{k}{v:g}" for k, v in s.items())


def make_rows(n, T, seed=0, copies=16):
    """`copies` rolled copies of one seeded randn · 2 row with a third of its columns at -inf, divided by T: fp32 (copies, n)."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    base = torch.randn(n, generator=g) * 2
    base[torch.randperm(n, generator=g)[: n // 3]] = float("-inf")
    return torch.stack([torch.roll(base, 7 * r) for r in range(copies)]) / T


def _log_softmax(x, kept):
    xs = torch.where(kept, x, torch.full_like(x, float("-inf")))
    return xs - torch.logsumexp(xs, 0)


def _threshold(x, kept, amb, lp, log_thr):
    """drop log p < log_thr unless the entry has the row's top score; entries within BAND of the threshold are ambiguous"""
    top = x == x[kept].max()
    amb |= kept & ~top & ((lp - log_thr).abs() < BAND)
    return kept & ~((lp < log_thr) & ~top)


def ref_chain(row, min_p=0.0, typical_p=1.0, eps=0.0, eta=0.0):
    """HF's MinP → Typical → Epsilon → Eta on one fp32 row (-inf = removed by an earlier warper), every softmax, entropy and cumsum in fp64
    → (kept, ambiguous).  `ambiguous` marks the entries whose decision lies within BAND of its threshold: |log p - log thr| for min_p /
    epsilon / eta; |key - cut key| for typical where the key is not the cut key, and the ranks whose cumulative mass before or at them is
    within BAND of typical_p."""
    x = row.double()
    kept = x > float("-inf")
    amb = torch.zeros_like(kept)
    if not kept.any():
        return kept, amb
    if 0.0 < min_p <= 1.0:
        lp = _log_softmax(x, kept)
        kept = _threshold(x, kept, amb, lp, math.log(min_p) + lp[kept].max())
    if 0.0 < typical_p < 1.0:
        lp = _log_softmax(x, kept)
        idx = kept.nonzero().flatten()
        p = lp[idx].exp()
        H = -(p * lp[idx]).sum()
        key = (-lp[idx] - H).abs()
        order = torch.sort(key, stable=True).indices
        cum = torch.cumsum(p[order], 0)
        last = min(int((cum < typical_p).sum()), idx.numel() - 1)
        cut = key[order[last]]
        amb[idx[(key != cut) & ((key - cut).abs() < BAND)]] = True
        near = ((cum - typical_p).abs() < BAND) | ((cum - p[order] - typical_p).abs() < BAND)
        amb[idx[order[near]]] = True
        kept = kept.clone()
        kept[idx[key > cut]] = False
    if 0.0 < eps < 1.0:
        lp = _log_softmax(x, kept)
        kept = _threshold(x, kept, amb, lp, math.log(eps))
    if 0.0 < eta < 1.0:
        lp = _log_softmax(x, kept)
        H = -(lp[kept].exp() * lp[kept]).sum()
        kept = _threshold(x, kept, amb, lp, math.log(min(eta, math.sqrt(eta) * math.exp(-float(H)))))
    return kept, amb


def hf_processors(min_p=0.0, typical_p=1.0, eps=0.0, eta=0.0):
    """The warpers HF's _get_logits_processor appends after top-p for these values, in its order."""
    from transformers.generation.logits_process import (EpsilonLogitsWarper, EtaLogitsWarper, LogitsProcessorList, MinPLogitsWarper,
                                                        TypicalLogitsWarper)
    out = LogitsProcessorList()
    if 0.0 < min_p <= 1.0:
        out.append(MinPLogitsWarper(min_p=min_p, min_tokens_to_keep=1))
    if 0.0 < typical_p < 1.0:
        out.append(TypicalLogitsWarper(mass=typical_p, min_tokens_to_keep=1))
    if 0.0 < eps < 1.0:
        out.append(EpsilonLogitsWarper(epsilon=eps, min_tokens_to_keep=1))
    if 0.0 < eta < 1.0:
        out.append(EtaLogitsWarper(epsilon=eta, min_tokens_to_keep=1, device="cpu"))
    return out


def hf_support(rows, **setting):
    """finite support of HF's classes applied to fp32 rows (B, n)"""
    scores = rows.clone()
    ids = torch.zeros((rows.shape[0], 1), dtype=torch.long)
    for proc in hf_processors(**setting):
        scores = proc(ids, scores)
    return scores > float("-inf")


def check_support(got, kept, amb, cap, what=""):
    """`got` (bool) equals the reference's support outside its ambiguous entries, of which there are at most `cap` — asserted first"""
    assert int(amb.sum()) <= cap, f"{what}: {int(amb.sum())} ambiguous entries in the reference (cap {cap})"
    bad = (got != kept) & ~amb
    assert not bad.any(), f"{what}: support differs at columns {bad.nonzero().flatten().tolist()[:8]} ({int(bad.sum())} in all)"


def planted_rows():
    """The cases random rows miss → (rows (8, 6100) fp32, the expected support, one setting per row)."""
    ninf = float("-inf")
    n, B = 6100, 8
    rows = torch.full((B, n), ninf)
    expect = torch.zeros((B, n), dtype=torch.bool)
    g = torch.Generator().manual_seed(3)
    # 0: a typical-p cut inside a run of equal keys, few survivors: p = (.4, .15 x 4) — the four equal entries have the smaller key and the
    #    cumulative mass reaches 0.4 at the third of them: all four stay, the 0.4 entry goes
    c = torch.randperm(n, generator=g)[:5]
    rows[0, c] = torch.tensor([0.4, 0.15, 0.15, 0.15, 0.15]).log()
    expect[0, c[1:]] = True
    # 1: the same with 6001 survivors: one entry of mass 0.4 and 6000 equal ones sharing 0.6 — the mass crosses 0.30005 in the middle of the
    #    equal ones: all of them stay, and the entry that goes is the row's top score
    c = torch.randperm(n, generator=g)[:6001]
    rows[1, c[1:]] = 0.0
    rows[1, c[0]] = math.log(0.4 / (0.6 / 6000))
    expect[1, c[1:]] = True
    # 2, 3: entries tied with the top score (p = 0.22 each) under epsilon_cutoff 0.9 / min_p 1.0: the tied tops stay, an entry 1e-4 below goes
    c = torch.randperm(n, generator=g)[:6]
    for r in (2, 3):
        rows[r, c] = torch.tensor([1.0, 1.0, 0.5, 1.0, -3.0, 0.9999])
        expect[r, c[[0, 1, 3]]] = True
    # 4: eta_cutoff 0.9 on the same values: eta = sqrt(.9) exp(-H) = 0.19 keeps the four entries of p = 0.22
    rows[4, c] = rows[2, c]
    expect[4, c[[0, 1, 3, 5]]] = True
    # 5: one survivor; 6: none; 7: one entry that dominates 5000 finite ones (their p is 0 in fp32)
    rows[5, 4321] = -7.5
    expect[5, 4321] = True
    rows[7, :5000] = -200.0
    rows[7, 77] = 3.0
    expect[7, 77] = True
    settings = [dict(typical_p=0.4), dict(typical_p=0.30005), dict(eps=0.9), dict(min_p=1.0), dict(eta=0.9), COMBINED, COMBINED,
                dict(min_p=0.5, typical_p=0.5, eps=0.5, eta=0.5)]
    return rows, expect, settings
