"""Shared by test_generate_combinations_cpu.py / test_generate_combinations_gpu.py: generate()'s options in combination.

Three things, all importable without a GPU:

  * the combination array — FACTORS (11 factors, level 0 = the default) → `build_array()`: a deterministic greedy covering array in which
    every pair of levels of two different factors occurs in at least one row, grown from SEEDS (the combinations no earlier suite ran: partial
    rows the greedy completes) — and `cover_rows()`, the greedy set cover "every non-default level at least once, one row the patch trio" for the merged groups;
  * `make_levels` / `bind`: the concrete values of the levels for one model and one prompt set, and a row bound to them (a "case") with
    its generate() keywords for the device path (`device_kwargs`) and for the hooked twin (`reference_kwargs`);
  * `reference_processors(case, cfg, kw, L)`: HF's own processor classes in GenerationMixin._get_logits_processor's order, the list that
    replaces the built-in options on the hooked loop.  Two things are not HF's: the decay is wrapped (`keep_minus_inf`: a column that was -inf
    on entry is -inf on exit, where HF's class produces NaN — the one documented deviation), and every class runs on host copies of the rows
    (`on_host`), which is the arithmetic test_generate_combinations_cpu.py pins to generation.score_bias_row bit for bit (a device-side
    division by a Python scalar need not be a correctly rounded division)."""
import itertools
import types
from collections import namedtuple

import torch

import token_automaton_util as T
from padt_amd.generation import StepMode
from test_token_automaton_gpu import LABELS                      # [[21, 22], [21, 23, 24], [31, 32]]
from test_token_logprobs_gpu import SCHED                        # text-only steps, VRT-only steps, a forced EOS

INF = float("inf")
T_NEW = 12
MAX_ROWS = 20
SAMPLING = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=11)
WARPERS = dict(min_p=0.05, typical_p=0.9)
PENALTY = 1.3
TOP_K = 3
# the list of test_decay_is_hfs_exponential_decay_length_penalty_on_the_hooked_loop (a literal inside that test, so it cannot be imported)
DECAY_CANDIDATES = ((2, 2.0), (2, 4.0), (1, 16.0), (0, 64.0))

# factor → levels; level 0 is the default ("off")
FACTORS = (
    ("selection", ("greedy", "sampling", "warpers")),
    ("repetition_penalty", ("pen1", "pen1.3")),
    ("bans", ("nobans", "bans")),
    ("automaton", ("free", "automaton")),
    ("logit_bias", ("nolb", "lb")),
    ("patch_bias", ("nopb", "pb")),
    ("decay", ("nodecay", "decay")),
    ("forced_tokens", ("unforced", "forced")),
    ("outputs", ("scores", "scores+lp", "scores+lp+top+patch", "lp_only")),
    ("execution", ("captured", "eager")),
    ("schedule", ("nosched", "sched")),
)
NAMES = tuple(n for n, _ in FACTORS)
Row = namedtuple("Row", NAMES)                                    # one level index per factor
# the factors that edit a score or the selection: switching one off must change a run somewhere in the array.  `outputs` and `execution`
# are the two that must change NOTHING (what every row's comparison with its hooked twin asserts instead).
EDITING = ("selection", "repetition_penalty", "bans", "automaton", "logit_bias", "patch_bias", "decay", "forced_tokens", "schedule")

# the combinations the feature suites never ran together, as partial rows (factor → level name); the greedy fills in the other factors
SEEDS = (
    dict(decay="decay", automaton="automaton"),                                                        # EOS banned in most states
    dict(decay="decay", schedule="sched"),                                                             # a schedule step masks EOS
    # patch prior + patch log-probs + a VRT state.  Without the schedule: its text-only steps 0-4 sit on the VRT states a label of two or
    # three tokens leads to, and no patch column would ever be a candidate
    dict(patch_bias="pb", outputs="scores+lp+top+patch", automaton="automaton", schedule="nosched"),
    dict(selection="warpers", forced_tokens="forced", outputs="scores+lp+top+patch"),                  # warpers + forced + top_logprobs
    dict(logit_bias="lb", automaton="automaton", forced_tokens="forced"),                              # -inf bias on the only edge's column
    dict(selection="greedy", forced_tokens="forced", outputs="lp_only", logit_bias="lb", bans="bans"),  # the probe head, bias, a ban bitmap, no row
    dict(selection="greedy", repetition_penalty="pen1.3", decay="decay", outputs="scores"),             # a penalised EOS column under the decay, rows kept
)


# ------------------------------------------------------------------------------------------------------------ the array
def all_pairs():
    """every (factor i, level a, factor j, level b), i < j"""
    out = set()
    for i, j in itertools.combinations(range(len(FACTORS)), 2):
        for a in range(len(FACTORS[i][1])):
            for b in range(len(FACTORS[j][1])):
                out.add((i, a, j, b))
    return out


def pairs_of(row):
    return {(i, row[i], j, row[j]) for i, j in itertools.combinations(range(len(row)), 2)}


def _complete(partial, uncovered):
    """Fill the free factors of `partial` (list, None = free) one at a time — the factor with the most levels first, ties in table order —
    with the level that covers the most uncovered pairs against what is already set; ties: the level with the most uncovered pairs against
    the still-free factors, then the lowest level."""
    row = list(partial)
    free = sorted((f for f in range(len(row)) if row[f] is None), key=lambda f: (-len(FACTORS[f][1]), f))
    for n, f in enumerate(free):
        best = None
        for lvl in range(len(FACTORS[f][1])):
            now = sum(1 for g in range(len(row)) if g != f and row[g] is not None
                      and ((f, lvl, g, row[g]) if f < g else (g, row[g], f, lvl)) in uncovered)
            later = sum(1 for p in uncovered if (p[0] == f and p[1] == lvl and row[p[2]] is None) or (p[2] == f and p[3] == lvl and row[p[0]] is None))
            key = (now, later, -lvl)
            if best is None or key > best[0]:
                best = (key, lvl)
        row[f] = best[1]
    return Row(*row)


def build_array():
    """The covering array: SEEDS completed in order, then rows grown around the factor level that still has the most uncovered pairs, until
    every pair of levels of two different factors is in some row.  Deterministic: no random choice, every tie broken by table order."""
    uncovered = all_pairs()
    rows = []

    def add(row):
        rows.append(row)
        uncovered.difference_update(pairs_of(row))
    for seed in SEEDS:
        partial = [None] * len(FACTORS)
        for name, level in seed.items():
            f = NAMES.index(name)
            partial[f] = FACTORS[f][1].index(level)
        add(_complete(partial, uncovered))
    while uncovered:
        count = {}
        for i, a, j, b in uncovered:
            count[(i, a)] = count.get((i, a), 0) + 1
            count[(j, b)] = count.get((j, b), 0) + 1
        f, lvl = max(sorted(count), key=lambda k: count[k])
        partial = [None] * len(FACTORS)
        partial[f] = lvl
        row = _complete(partial, uncovered)
        assert pairs_of(row) & uncovered
        add(row)
    return rows


def row_id(index, row):
    """r07-sampling-pen1.3-automaton-decay-lp_only: the row's index and its non-default levels"""
    on = [FACTORS[f][1][lvl] for f, lvl in enumerate(row) if lvl]
    return "r%02d-%s" % (index, "-".join(on) if on else "defaults")


def is_patch_trio(row):
    """the automaton, the patch bias and the patch log-probs on together: what the merged groups have to number by row_base / vrt_off"""
    return bool(row.automaton and row.patch_bias and row.outputs == 2)


def cover_items(row):
    """what a row contributes to the cover: its non-default (factor, level)s, and the patch trio as an item of its own"""
    return {(f, lvl) for f, lvl in enumerate(row) if lvl} | ({"patch trio"} if is_patch_trio(row) else set())


def cover_rows(rows):
    """Greedy set cover: the indices of a smallest-found set of rows in which every non-default LEVEL of every factor occurs at least once
    — more than "every factor off its default": the four `outputs` levels are four sets of buffers — and one row is the patch trio (each
    step: the row that adds the most items, ties to the lowest index)."""
    todo, out = set().union(*(cover_items(r) for r in rows)), []
    assert "patch trio" in todo and {x for x in todo if x != "patch trio"} == {(f, lvl) for f, (_, lv) in enumerate(FACTORS) for lvl in range(1, len(lv))}
    while todo:
        gain = [len(todo & cover_items(r)) for r in rows]
        k = max(range(len(rows)), key=lambda i: (gain[i], -i))
        out.append(k)
        todo -= cover_items(rows[k])
    return out


def switched_off(row, factor):
    return row._replace(**{factor: 0})


# ------------------------------------------------------------------------------------------------------------ the levels' values
def text_ids(tokens, cfg, exclude=(), fallback=(41, 42, 43, 44, 45, 46)):
    """the distinct plain text ids (below image_token_id, no EOS / pad, none of `exclude`) of a run's tokens in order, then the fallback ids"""
    out = []
    skip = set(int(e) for e in exclude) | {int(cfg.eos_token_id), int(cfg.pad_token_id)}
    for x in list(tokens) + list(fallback):
        x = int(x)
        if 0 <= x < min(int(cfg.vocab_size), int(cfg.image_token_id)) and x not in skip and x not in out:
            out.append(x)
    return out


def patch_map(h2, w2, shift=0):
    """a (h/2, w/2) prior: -inf outside a 2 x 3 window, graded inside"""
    m = torch.full((h2, w2), -INF)
    r = shift % max(1, h2 - 1)
    m[r: r + 2, 1: 4] = torch.tensor([[0.0, 2.0, -1.5], [0.5, 0.0, 3.0]])[: h2 - r, : w2 - 1]
    return m


def make_levels(cfg, grids, plain_tokens, eos, decay, forced=None, shift=0):
    """The non-default levels' values for one prompt set.  grids: the samples' (t, h, w); plain_tokens (2, T): the plain run's generated
    tokens — the bans and two bias entries are taken from it so that they bite by construction; eos: the call's EOS list; decay: (start,
    factor).  The label tokens are named on purpose: 31 — one of the start state's two edges — is suppressed at the first step and 22 at
    every step, so a dropped union of the two ban bitmaps shows in the first score row; 22 is also pushed up by the bias; 24 — the ONLY
    edge after (21, 23) — carries the -inf bias and is the last forced id of row 0."""
    labels = {x for lb in LABELS for x in lb}
    a = text_ids(plain_tokens[0], cfg, exclude=set(eos) | labels)
    b = text_ids(plain_tokens[1][1:], cfg, exclude=set(eos) | labels | set(a[:4]))
    lb = {22: 3.0, 1500: 3.125, int(cfg.eos_token_id): -2.0, 24: -INF, a[0]: -4.0, b[0]: -6.5}
    maps = [None] * (len(grids) - 1) + [patch_map(int(grids[-1][1]) // 2, int(grids[-1][2]) // 2, shift)]
    return types.SimpleNamespace(
        eos=[int(e) for e in eos],
        bans=dict(no_repeat_ngram_size=2, suppress_tokens=[22, a[3]], bad_words_ids=[[a[1], a[2]]], begin_suppress_tokens=[a[0], 31]),
        logit_bias=lb, patch_bias=maps, decay=(int(decay[0]), float(decay[1])),
        forced=[[21, 23, 24], [-1, 23]] if forced is None else forced,      # row 0: steps 0-2; row 1: step 1 only; everything else free
        automaton=T.label_automaton(LABELS, repeat=True))


def bind(row, lv):
    """a row of the array with its levels' values: what device_kwargs / reference_kwargs / reference_processors read"""
    on = lambda name: bool(getattr(row, name))
    return types.SimpleNamespace(row=row, lv=lv, sampling=row.selection >= 1, warpers=row.selection == 2,
                                 penalty=PENALTY if on("repetition_penalty") else 1.0, bans=lv.bans if on("bans") else None,
                                 automaton=lv.automaton if on("automaton") else None, logit_bias=lv.logit_bias if on("logit_bias") else None,
                                 patch_bias=lv.patch_bias if on("patch_bias") else None, decay=lv.decay if on("decay") else None,
                                 forced=lv.forced if on("forced_tokens") else None, outputs=row.outputs, use_graph=not on("execution"),
                                 schedule=list(SCHED) if on("schedule") else None, eos=list(lv.eos))


def selection_kwargs(case):
    kw = dict(SAMPLING) if case.sampling else dict(do_sample=False)
    if case.warpers:
        kw.update(WARPERS)
    return kw


def output_kwargs(case):
    kw = dict(output_scores=case.outputs != 3)
    if case.outputs >= 1:
        kw["output_token_logprobs"] = True
    if case.outputs == 2:
        kw.update(top_logprobs=TOP_K, output_patch_logprobs=True)
    return kw


def shared_kwargs(case):
    """what both sides of a comparison get: selection, forced tokens, schedule, the EOS list, the length"""
    kw = dict(selection_kwargs(case), max_new_tokens=T_NEW, eos_token_id=list(case.eos))
    if case.forced is not None:
        kw["forced_tokens"] = [list(r) for r in case.forced]
    if case.schedule is not None:
        kw["schedule"] = list(case.schedule)
    return kw


def device_kwargs(case):
    """the options as generate() arguments"""
    kw = dict(shared_kwargs(case), **output_kwargs(case), repetition_penalty=case.penalty, use_graph=case.use_graph)
    if case.bans is not None:
        kw.update(case.bans)
    if case.automaton is not None:
        kw["token_automaton"] = case.automaton
    if case.logit_bias is not None:
        kw["logit_bias"] = dict(case.logit_bias)
    if case.patch_bias is not None:
        kw["patch_bias"] = list(case.patch_bias)
    if case.decay is not None:
        kw["exponential_decay_length_penalty"] = case.decay
    return kw


def identity_processor(input_ids, scores):
    return scores


def reference_kwargs(case, cfg, kw, L):
    """the hooked twin: no built-in option except selection, forced tokens and the schedule; HF's classes as logits_processor (a row without
    any edit still goes through the hooked loop: one processor that returns its input); the same output flags plus output_scores"""
    procs = reference_processors(case, cfg, kw, L) or [identity_processor]
    return dict(shared_kwargs(case), **dict(output_kwargs(case), output_scores=True), repetition_penalty=1.0, logits_processor=procs)


def expected_mode(case, reference=False):
    """the StepMode a call of this row resolves to — on the device path, or on the hooked twin"""
    dev = not reference
    return StepMode(sampling=case.sampling, keep_scores=case.outputs != 3 or reference, keep_logits=False, rules=dev and case.bans is not None,
                    token_logprobs=case.outputs >= 1, top_k=TOP_K if case.outputs == 2 else 0, patches=case.outputs == 2,
                    processors=reference, reference=False, warpers=case.warpers, forced=case.forced is not None,
                    automaton=dev and case.automaton is not None,
                    bias=dev and (case.logit_bias is not None or case.patch_bias is not None or case.decay is not None))


# ------------------------------------------------------------------------------------------------------------ the reference chain
def on_host(proc):
    """`proc` on host copies of (input_ids, scores): fp32 CPU arithmetic, whatever device the loop's rows live on"""
    def run(input_ids, scores):
        return proc(input_ids.cpu(), scores.to(torch.float32).cpu())
    return run


def keep_minus_inf(proc):
    """The one deviation from HF: a column that is -inf on entry is -inf again on exit (ExponentialDecayLengthPenalty computes
    -inf + |-inf| * a = NaN on an EOS column a ban, the schedule or the automaton removed)."""
    def run(input_ids, scores):
        dead = scores == -INF
        out = proc(input_ids, scores)
        return torch.where(dead, torch.full_like(out, -INF), out)
    return run


def reference_processors(case, cfg, kw, L):
    """HF's processors for the row's options, in GenerationMixin._get_logits_processor's order restricted to what is used: SequenceBias, the
    patch-vector adder (where a second sequence bias would sit), RepetitionPenalty, NoRepeatNGram, NoBadWords, PrefixConstrained, the (wrapped)
    ExponentialDecayLengthPenalty, SuppressTokens, SuppressTokensAtBegin.  cfg: the model config (vocab_size); kw: the call's inputs
    (image_grid_thw → the rows' patch ranges); L: the prompt length."""
    from transformers.generation import logits_process as lp
    import test_score_bias_gpu as SB
    import test_token_automaton_gpu as TAG
    grids = torch.as_tensor(kw["image_grid_thw"]).tolist()
    eos = list(case.eos)
    out = []
    if case.logit_bias is not None:
        out.append(SB.hf_sequence_bias(case.logit_bias))
    if case.patch_bias is not None:
        out.append(SB.add_patch_vector(cfg, grids, case.patch_bias))
    if case.penalty != 1.0:
        out.append(lp.RepetitionPenaltyLogitsProcessor(case.penalty))
    if case.bans is not None:
        out.append(lp.NoRepeatNGramLogitsProcessor(case.bans["no_repeat_ngram_size"]))
        out.append(lp.NoBadWordsLogitsProcessor(case.bans["bad_words_ids"], eos))
    if case.automaton is not None:
        fn = T.prefix_fn(case.automaton, L, cfg.vocab_size, TAG.patch_ranges(kw["image_grid_thw"], kw.get("image_index")), eos)
        out.append(lp.PrefixConstrainedLogitsProcessor(fn, 1))
    if case.decay is not None:
        out.append(keep_minus_inf(lp.ExponentialDecayLengthPenalty(case.decay, eos, L)))
    if case.bans is not None:
        out.append(lp.SuppressTokensLogitsProcessor(case.bans["suppress_tokens"]))
        out.append(lp.SuppressTokensAtBeginLogitsProcessor(case.bans["begin_suppress_tokens"], L))
    return [on_host(p) for p in out]
