"""generate()'s options in combination, host side: the covering array (pair coverage, the cap, determinism, the cover for the merged
groups), the rows' keywords and step modes, and the reference chain — HF's own classes in HF's order, the decay wrapped — against
generation.score_bias_row bit for bit.  No GPU."""
import itertools
from types import SimpleNamespace

import torch

import gen_rules_util as G
import generate_combinations_util as C
from padt_amd.generation import StepMode, check_logit_bias, decay_table, score_bias_row

INF = float("inf")


# ------------------------------------------------------------------------------------------------------------ the array
def test_the_array_covers_every_pair_within_the_cap_and_is_deterministic():
    rows = C.build_array()
    assert len(rows) <= C.MAX_ROWS, f"{len(rows)} rows"
    assert rows == C.build_array(), "two calls of the builder differ"
    sizes = [len(levels) for _, levels in C.FACTORS]
    assert sizes == [3, 2, 2, 2, 2, 2, 2, 2, 4, 2, 2] and all(len(r) == len(sizes) for r in rows)
    assert all(0 <= r[f] < sizes[f] for r in rows for f in range(len(sizes)))
    want = {(i, a, j, b) for i, j in itertools.combinations(range(len(sizes)), 2) for a in range(sizes[i]) for b in range(sizes[j])}
    assert C.all_pairs() == want and len(want) == sum(x * y for x, y in itertools.combinations(sizes, 2))
    got = set()
    for r in rows:
        got |= {(i, r[i], j, r[j]) for i, j in itertools.combinations(range(len(sizes)), 2)}
    assert got == want, f"uncovered pairs: {sorted(want - got)[:5]}"
    assert len(set(rows)) == len(rows) and len({C.row_id(i, r) for i, r in enumerate(rows)}) == len(rows)
    print(f"\n[array] {len(rows)} rows: " + ", ".join(C.row_id(i, r) for i, r in enumerate(rows)))


def test_the_seeded_combinations_are_rows_of_the_array():
    rows = C.build_array()
    for seed in C.SEEDS:
        want = {C.NAMES.index(n): C.FACTORS[C.NAMES.index(n)][1].index(lvl) for n, lvl in seed.items()}
        assert any(all(r[f] == lvl for f, lvl in want.items()) for r in rows), seed


def test_the_cover_for_the_merged_groups_takes_every_factor_off_its_default():
    """... at every non-default level, and one of its rows has the automaton, the patch bias and the patch log-probs on together"""
    rows = C.build_array()
    cover = C.cover_rows(rows)
    assert cover == C.cover_rows(rows) and len(set(cover)) == len(cover) <= 4
    for f, (name, levels) in enumerate(C.FACTORS):
        for lvl in range(1, len(levels)):
            assert any(rows[k][f] == lvl for k in cover), (name, levels[lvl])
    trio = [k for k in cover if C.is_patch_trio(rows[k])]
    assert trio and all(rows[k].automaton and rows[k].patch_bias and rows[k].outputs == 2 for k in trio)
    assert any(not rows[k].schedule for k in trio), "under the schedule no VRT state of the automaton has a candidate"
    for k in cover:                                              # greedy: no row of the cover is redundant
        rest = set().union(*(C.cover_items(rows[j]) for j in cover if j != k))
        assert C.cover_items(rows[k]) - rest


def test_the_named_constants_are_the_feature_suites_own():
    import test_token_automaton_gpu as TAG
    import test_token_logprobs_gpu as TL
    import test_score_bias_gpu as SB
    assert C.LABELS is TAG.LABELS and C.SCHED is TL.SCHED and C.T_NEW == TL.T_NEW == len(C.SCHED)
    assert {k: TL.MODES["sampling"][k] for k in C.SAMPLING} == C.SAMPLING
    assert set(C.SCHED) == {"t", "v", "e"}                        # text-only steps, VRT-only steps, a forced EOS
    assert SB.T_NEW == C.T_NEW


# ------------------------------------------------------------------------------------------------------------ rows → keywords, step modes
V, EOS, EOS2, PAD = 1600, 7, 30, 9                                # (1500 carries a bias: the vocabulary reaches past it)
CFG = SimpleNamespace(vocab_size=V, eos_token_id=EOS, pad_token_id=PAD, image_token_id=1590)
GRIDS = [[1, 4, 6], [1, 4, 8]]                                   # 6 and 8 patches: columns V .. V + 5 and V + 6 .. V + 13
KW = dict(image_grid_thw=torch.tensor(GRIDS))
N_COLS = V + 6 + 8
L = 5


def levels():
    plain = torch.tensor([[11, 12, 13, 14, 15, 16], [17, 18, 19, 20, 25, 26]])
    return C.make_levels(CFG, GRIDS, plain.tolist(), [EOS, EOS2], (1, 1.5))


def test_levels_are_what_the_table_says():
    lv = levels()
    lb = lv.logit_bias
    assert any(v > 0 for v in lb.values()) and any(-INF < v < 0 for v in lb.values()) and list(lb.values()).count(-INF) == 1 and EOS in lb
    assert lb[24] == -INF and check_logit_bias(lb, 2048) is not None
    assert lv.bans == dict(no_repeat_ngram_size=2, suppress_tokens=[22, 14], bad_words_ids=[[12, 13]], begin_suppress_tokens=[11, 31])
    assert lv.patch_bias[0] is None and tuple(lv.patch_bias[1].shape) == (2, 4) and bool(torch.isfinite(lv.patch_bias[1]).any())
    assert bool((lv.patch_bias[1] == -INF).any())
    rows = lv.forced
    assert [t for t, x in enumerate(rows[0]) if x >= 0] == [0, 1, 2] and [t for t, x in enumerate(rows[1]) if x >= 0] == [1]
    assert rows[0][2] == 24 and lb[rows[0][2]] == -INF          # one forced id is a column the bias sets to -inf
    allowed = lv.automaton.allowed([21, 23], V, (0, 6), [EOS, EOS2])
    assert allowed == [24], "24 is the only edge after (21, 23)"


def test_rows_resolve_to_keywords_and_step_modes():
    lv = levels()
    rows = C.build_array()
    for r in rows:
        case = C.bind(r, lv)
        dev, ref = C.device_kwargs(case), C.reference_kwargs(case, CFG, KW, L)
        built_in = ("no_repeat_ngram_size", "suppress_tokens", "bad_words_ids", "begin_suppress_tokens", "token_automaton", "logit_bias", "patch_bias",
                    "exponential_decay_length_penalty")
        assert not set(built_in) & set(ref) and ref["repetition_penalty"] == 1.0 and ref["output_scores"] is True and len(ref["logits_processor"]) >= 1
        for k in ("do_sample", "seed", "temperature", "top_k", "top_p", "min_p", "typical_p", "forced_tokens", "schedule", "eos_token_id",
                  "max_new_tokens", "output_token_logprobs", "top_logprobs", "output_patch_logprobs"):
            assert dev.get(k) == ref.get(k), k
        assert (dev["repetition_penalty"] == 1.3) == bool(r.repetition_penalty) and dev["use_graph"] == (not r.execution)
        assert ("token_automaton" in dev) == bool(r.automaton) and ("schedule" in dev) == bool(r.schedule)
        assert dev["output_scores"] == (r.outputs != 3) and bool(dev.get("output_token_logprobs")) == (r.outputs >= 1)
        m, h = C.expected_mode(case), C.expected_mode(case, reference=True)
        assert not m.processors and h.processors and not (h.rules or h.automaton or h.bias) and h.keep_scores
        assert m.bias == bool(r.logit_bias or r.patch_bias or r.decay) and m.rules == bool(r.bans) and m.automaton == bool(r.automaton)
        assert (m.sampling, m.warpers, m.forced, m.token_logprobs, m.top_k, m.patches) == (h.sampling, h.warpers, h.forced, h.token_logprobs, h.top_k, h.patches)
        n_procs = bool(r.logit_bias) + bool(r.patch_bias) + bool(r.repetition_penalty) + 4 * bool(r.bans) + bool(r.automaton) + bool(r.decay)
        assert len(C.reference_processors(case, CFG, KW, L)) == n_procs
    assert C.expected_mode(C.bind(C.Row(*[0] * len(C.FACTORS)), lv)) == StepMode(keep_scores=True)
    assert len({C.expected_mode(C.bind(r, lv)) for r in rows}) >= 10, "the array reaches at least ten step modes"


# ------------------------------------------------------------------------------------------------------------ the reference chain
def chain(case, ids, rows):
    out = rows
    for p in C.reference_processors(case, CFG, KW, L):
        out = p(ids, out)
    return out


def bias_matrix(lv, with_patches=True):
    """the rows' bias vectors: the logit_bias entries on the text columns, the map on the sample's own patch columns"""
    b = torch.zeros(2, N_COLS)
    for k, v in lv.logit_bias.items():
        b[:, k] = v
    if with_patches:
        b[1, V + 6: V + 14] = lv.patch_bias[1].reshape(-1)
    return b


def test_the_chain_is_the_specification_bit_for_bit():
    """bias (text and patch), penalty, the four bans and the decay on; random fp32 rows with -inf entries, an EOS column among them; one
    step before `start`, `start` itself and two steps after it"""
    lv = levels()
    start = lv.decay[0]
    on = C.Row(**dict({n: 0 for n in C.NAMES}, repetition_penalty=1, bans=1, logit_bias=1, patch_bias=1, decay=1))
    case = C.bind(on, lv)
    table = decay_table(lv.decay, C.T_NEW)
    g = torch.Generator().manual_seed(5)
    edited = 0
    for t in (start - 1, start, start + 1, start + 2):
        assert t >= 0
        logits = torch.randn(2, N_COLS, generator=g) * 5
        masked = torch.rand(2, N_COLS, generator=g) < 0.2
        masked[:, [EOS, EOS2]] = False
        masked[0, EOS2] = True                                    # an EOS column that is -inf before any processor: HF's class alone gives NaN
        logits[masked] = -INF
        ids = torch.randint(0, N_COLS, (2, L + t), generator=g)
        ids[0, -1], ids[1, -1] = 12, 21                          # the two-token bad word (12, 13) and a repeated bigram are armed
        ids[1, 1], ids[1, 2] = 21, 40
        seen = torch.zeros(2, N_COLS, dtype=torch.bool).scatter_(1, ids, True)
        banned = torch.stack([G.hf_ban(lv.bans, [EOS, EOS2], ids[b].tolist(), L, N_COLS) for b in range(2)])
        assert bool(banned[0, 13]) and bool(banned[1, 40]) and bool(banned[:, 22].all()) and bool(banned[:, 11].all()) == (t == 0)
        want = score_bias_row(logits, bias=bias_matrix(lv), penalty=C.PENALTY, seen=seen, banned=banned, eos_ids=(EOS, EOS2), a_t=table[t])
        got = chain(case, ids, logits.clone())
        assert got.dtype == torch.float32 and not bool(torch.isnan(got).any()), t
        assert torch.equal(got, want) and torch.equal(got == -INF, want == -INF), t
        assert got[0, EOS2] == -INF and bool((got[masked] == -INF).all()) and bool((got[:, 24] == -INF).all())
        off = score_bias_row(logits, bias=bias_matrix(lv), penalty=C.PENALTY, seen=seen, banned=banned, eos_ids=(EOS, EOS2), a_t=0.0)
        assert torch.equal(got, off) == (t <= start), t
        edited += int(not torch.equal(got, off))
    assert edited == 2


def test_the_wrapper_is_the_only_edit():
    """without a -inf EOS column on entry the wrapped decay IS HF's class; with one, HF's class gives NaN there and the wrapper -inf"""
    from transformers.generation.logits_process import ExponentialDecayLengthPenalty
    hf = ExponentialDecayLengthPenalty((1, 2.0), [EOS, EOS2], L)
    g = torch.Generator().manual_seed(9)
    rows = torch.randn(3, N_COLS, generator=g) * 4
    rows[torch.rand(3, N_COLS, generator=g) < 0.3] = -INF
    rows[:, [EOS, EOS2]] = torch.randn(3, 2, generator=g)
    ids = torch.zeros(3, L + 3, dtype=torch.long)
    assert torch.equal(C.keep_minus_inf(hf)(ids, rows.clone()), hf(ids, rows.clone()))
    rows[1, EOS] = -INF
    plain, wrapped = hf(ids, rows.clone()), C.keep_minus_inf(hf)(ids, rows.clone())
    assert bool(torch.isnan(plain[1, EOS])) and int(torch.isnan(plain).sum()) == 1
    assert wrapped[1, EOS] == -INF and not bool(torch.isnan(wrapped).any())
    keep = torch.ones_like(rows, dtype=torch.bool)
    keep[1, EOS] = False
    assert torch.equal(wrapped[keep], plain[keep])
    # on_host: the same numbers from rows and ids of any dtype the loop holds
    assert torch.equal(C.on_host(hf)(ids.to(torch.int32).long(), rows.clone())[keep], plain[keep])


def test_the_chain_with_the_automaton_bans_everything_but_allowed():
    lv = levels()
    on = C.Row(**dict({n: 0 for n in C.NAMES}, automaton=1, decay=1, logit_bias=1))
    case = C.bind(on, lv)
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(2, N_COLS, generator=g)
    prompt = torch.zeros(2, L, dtype=torch.long)
    for gen, allowed0, allowed1 in (([], [21, 31], [21, 31]), ([21], [22, 23], [22, 23]), ([21, 23], [], []),
                                    ([31, 32], list(range(V, V + 6)), list(range(V + 6, V + 14)))):
        ids = torch.cat([prompt, torch.tensor([gen, gen], dtype=torch.long)], 1)
        got = chain(case, ids, rows.clone())
        assert not bool(torch.isnan(got).any())
        for b, ok in enumerate((allowed0, allowed1)):
            assert torch.isfinite(got[b]).nonzero().flatten().tolist() == ok, (gen, b)      # after (21, 23): 24 alone, and the bias bans it
    # off the automaton at a step past the decay's start: EOS ids only, edited by the decay, every other column -inf
    ids = torch.cat([prompt, torch.tensor([[21, 5, 5, 5], [31, 32, 5, 5]], dtype=torch.long)], 1)
    got = chain(case, ids, rows.clone())
    for b in range(2):
        assert torch.isfinite(got[b]).nonzero().flatten().tolist() == [EOS, EOS2]
    a = decay_table(lv.decay, C.T_NEW)[4]
    v = rows[:, EOS2]
    assert torch.equal(got[:, EOS2], v + v.abs() * a)
