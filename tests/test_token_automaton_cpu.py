"""generate(token_automaton=A), host side: the TokenAutomaton class (tries, normal form, validation, caps), `allowed()` — the specification
the kernel is compared against — by hand and against the installed HF PrefixConstrainedLogitsProcessor, the packed table, the C-ABI
declaration and its wrapper, the options (GenOptions.automaton / StepMode.automaton) and the entry points.  No GPU."""
import dataclasses
import inspect

import pytest
import torch

import token_automaton_util as T
from padt_amd import _lib, ops
from padt_amd.generation import (GenOptions, StepMode, TokenAutomaton, check_generate_kwargs, check_token_automaton, resolve_options)

TA = TokenAutomaton
VRT, TEXT, EOS = TA.VRT, TA.TEXT, TA.EOS
INF = float("inf")


# ------------------------------------------------------------------------------------------------------------ tries
def test_from_sequences_builds_the_category_trie():
    cats = [[5, 6], [5, 7, 8], [9]]
    A = TA.from_sequences([c + [VRT] * 2 for c in cats])
    n_text, rng, eos = 20, (3, 6), [2]
    patches = [23, 24, 25]
    assert A.allowed([], n_text, rng, eos) == [5, 9]
    assert A.allowed([5], n_text, rng, eos) == [6, 7]                        # the shared prefix branches
    assert A.allowed([5, 7], n_text, rng, eos) == [8]
    assert A.allowed([5, 6], n_text, rng, eos) == patches and A.allowed([9, 24], n_text, rng, eos) == patches
    assert A.allowed([9, 24, 23], n_text, rng, eos) == [2]                   # complete: EOS and nothing else
    assert A.allowed([9, 24, 23, 2], n_text, rng, eos) == [2]                # the terminal state: the empty set → EOS
    # repeat: the end of a sequence also carries the start state's edges
    R = TA.from_sequences([c + [VRT] * 2 for c in cats], repeat=True)
    assert R.allowed([9, 24, 23], n_text, rng, eos) == [2, 5, 9]
    assert R.allowed([9, 24, 23, 5, 7], n_text, rng, eos) == [8] and R.allowed([], n_text, rng, eos) == [5, 9]
    assert len(R.edges) == len(A.edges) and R != A
    # every complete sequence ends in ONE terminal state entered through EOS
    term = [s for s, e in enumerate(A.edges) if not e]
    assert len(term) == 1 and all(k == EOS for st in A.edges for k, nx in st if nx == term[0])
    # a sequence that is a prefix of another: EOS or go on; with repeat the restart must not collide with the continuation
    P = TA.from_sequences([[5], [5, 6]])
    assert P.allowed([5], n_text, rng, [2, 3]) == [2, 3, 6]
    with pytest.raises(ValueError, match="token_automaton"):
        TA.from_sequences([[5], [5, 5]], repeat=True)
    for bad in ([], [[]], [[5, EOS]], [[5, -4]], [[5.0]], [5]):
        with pytest.raises(ValueError, match="token_automaton"):
            TA.from_sequences(bad)


def test_normal_form_equal_automata_have_equal_keys():
    seqs = [[5, 6, VRT], [5, 7, VRT], [9, TEXT, VRT]]
    a, b = TA.from_sequences(seqs, repeat=True), TA.from_sequences([tuple(s) for s in reversed(seqs)], repeat=True)
    assert a == b and a.key == b.key and hash(a) == hash(b) and len({a, b}) == 1
    assert a != TA.from_sequences(seqs) and a != TA.from_sequences(seqs[:2], repeat=True)
    hash(a.key)                                                              # hashable: the decode-group key
    for st in a.edges:
        assert list(st) == sorted(st)                                        # sorted per state, classes (negative keys) first
    x = TA([[(7, 0), (VRT, 0), (3, 0), (EOS, 1), (TEXT, 0)], []])
    y = TA([((TEXT, 0), (EOS, 1), (3, 0), (VRT, 0), (7, 0)), ()], start=0)
    assert x == y and x.edges[0] == ((EOS, 1), (TEXT, 0), (VRT, 0), (3, 0), (7, 0))
    assert TA([[(3, 0)], [(3, 1)]], start=1) != TA([[(3, 0)], [(3, 1)]], start=0)


@pytest.mark.parametrize("edges,start,what", [
    ([[(3, 0), (3, 0)]], 0, "duplicate key 3"),
    ([[(VRT, 0), (VRT, 0)]], 0, "duplicate key VRT"),
    ([[(3, 1)]], 0, "next_state 1"),
    ([[(3, -1)]], 0, "next_state -1"),
    ([[(3, 0)]], 1, "start state"),
    ([[(-4, 0)]], 0, "key -4"),
    ([[(3.5, 0)]], 0, "integers"),
    ([[(True, 0)]], 0, "integers"),
    ([[(3,)]], 0, "pair"),
    ([[(3, 1)], []], 0, "state 1 has no edges"),                             # reachable, edgeless, entered through an id
    ([[(EOS, 1), (TEXT, 1)], []], 0, "state 1 has no edges"),                # ... through EOS and through TEXT
    ([[]], 0, "start state 0 has no edges"),
    (5, 0, "list of per-state"),
])
def test_malformed_tables_raise_value_error_naming_the_argument(edges, start, what):
    with pytest.raises(ValueError, match="token_automaton") as e:
        TA(edges, start=start)
    assert what in str(e.value)


def test_validation_against_the_vocabulary_and_the_argument_type():
    A = TA([[(999, 0), (EOS, 1)], []])
    assert check_token_automaton(A, 1000) is A and check_token_automaton(None, 1000) is None
    with pytest.raises(ValueError, match="token_automaton.*id 999"):
        check_token_automaton(A, 999)
    TA([[(3, 0), (EOS, 1)], [], []])                                         # an UNREACHABLE edgeless state is nobody's business
    for bad in (lambda b, ids: [1], [[(3, 0)]], "x"):
        with pytest.raises(ValueError, match="token_automaton"):
            check_token_automaton(bad, 1000)


def test_caps_hold_4096_states_and_32768_edges():
    assert TA.MAX_STATES >= 4096 and TA.MAX_EDGES >= 32768
    S, per = TA.MAX_STATES, TA.MAX_EDGES // TA.MAX_STATES
    full = TA([[(k, (s + 1) % S) for k in range(per)] for s in range(S)])
    assert sum(len(e) for e in full.edges) == TA.MAX_EDGES
    t = ops.token_automaton_tensor(full)
    assert t.numel() == ops.TOKEN_AUTOMATON_INTS == 5 + S + 2 * TA.MAX_EDGES and t.dtype == torch.int32
    with pytest.raises(NotImplementedError, match=f"token_automaton.*{TA.MAX_STATES} states"):
        TA([[(0, 0)]] * (S + 1))
    with pytest.raises(NotImplementedError, match=f"token_automaton.*{TA.MAX_EDGES} edges"):
        TA([[(k, 0) for k in range(TA.MAX_EDGES + 1)]])
    with pytest.raises(NotImplementedError, match=f"{TA.MAX_EDGES} edges"):
        ops.token_automaton_tensor(key=(0, (tuple((k, 0) for k in range(TA.MAX_EDGES + 1)),)))


# ------------------------------------------------------------------------------------------------------------ allowed(): the specification
def test_allowed_by_hand():
    n_text, rng = 40, (2, 5)
    patches = [42, 43, 44]
    A = TA([[(TEXT, 1), (7, 2), (9, 3)],              # 0: any text but EOS; 7 and 9 explicitly (9 is an EOS id: explicit wins over the carve-out)
            [(VRT, 1), (EOS, 4), (TEXT, 0)],          # 1: everything; with an EOS edge the EOS ids stay in the TEXT range
            [(VRT, 2)],                               # 2: VRT only
            [(5, 0)],                                 # 3
            []])                                      # 4: terminal
    eos = [9, 11]
    text = list(range(n_text))
    assert A.allowed([], n_text, rng, eos) == [c for c in text if c != 11]                # 11 carved out, 9 kept by its explicit edge
    assert A.allowed([], n_text, rng, [11]) == [c for c in text if c != 11]
    assert A.allowed([3], n_text, rng, eos) == text + patches                             # via TEXT → 1
    assert A.allowed([7], n_text, rng, eos) == patches and A.allowed([7, 43], n_text, rng, eos) == patches
    assert A.walk([9], n_text, rng, eos) == 3 and A.walk([9], n_text, rng, [11]) == 3     # explicit over EOS / over TEXT
    assert A.walk([11], n_text, rng, eos) == TA.OFF                                       # an EOS id is not TEXT, and state 0 has no EOS edge
    assert A.walk([3, 11], n_text, rng, eos) == 4 and A.walk([3, 44, 12], n_text, rng, eos) == 0
    # off the automaton: a token without an edge — a foreign patch, a column past the table, text where only VRT goes — for good
    for toks in ([7, 45], [7, 41], [7, 3], [9, 6], [7, 10 ** 6], [7, -1]):
        assert A.walk(toks, n_text, rng, eos) == TA.OFF and A.allowed(toks, n_text, rng, eos) == eos
        assert A.allowed(toks + [7, 42], n_text, rng, eos) == eos
    # the empty set → EOS: the terminal state, and a VRT-only state of a sample without patches
    assert A.allowed([3, 9], n_text, rng, eos) == eos
    assert A.allowed([7], n_text, (5, 5), eos) == eos and A.allowed([7], n_text, (5, 5), [11, 9, 11]) == eos
    assert A.allowed([3], n_text, (5, 5), eos) == text                                    # ... while a mixed state just loses the range
    assert A.accepts([3, 44, 12, 7, 42, 43], n_text, rng, eos) and A.accepts([3, 9, 0, 0], n_text, rng, eos)
    assert not A.accepts([7, 3], n_text, rng, eos) and not A.accepts([11], n_text, rng, eos)


def test_allowed_is_what_hfs_prefix_constrained_processor_applies():
    """`allowed()` wrapped as HF's prefix_allowed_tokens_fn: PrefixConstrainedLogitsProcessor gives -inf exactly outside it and the input
    bits elsewhere — on random automata, histories on and off the automaton, all three rows of the kernel cases."""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    g = torch.Generator().manual_seed(0)
    L = 4
    ranges = list(zip(T.VRT_OFF[:-1], T.VRT_OFF[1:]))
    n_off = 0
    for seed in range(6):
        eos = T.EOS_LISTS[seed % 2]
        A = T.random_automaton(seed, eos)
        for length in T.HISTORY_LENGTHS:
            hist = [T.random_history(100 * seed + b, A, length, ranges[b], eos) for b in range(3)]
            ids = torch.tensor([[1] * L + h for h in hist], dtype=torch.long)
            scores = torch.randn(3, T.N_COLS, generator=g)
            out = PrefixConstrainedLogitsProcessor(T.prefix_fn(A, L, T.V, ranges, eos), 1)(ids, scores.clone())
            for b in range(3):
                ban = T.ban_row(A, hist[b], ranges[b], eos)
                assert bool((out[b][ban] == -INF).all()) and torch.equal(out[b][~ban].view(torch.int32), scores[b][~ban].view(torch.int32))
                assert not ban.all()
                n_off += A.walk(hist[b], T.V, ranges[b], eos) == TA.OFF
    assert n_off >= 3, "precondition: some histories leave the automaton"


def test_random_automata_have_the_states_the_kernel_cases_need():
    for seed in range(6):
        A = T.random_automaton(seed, T.EOS_LISTS[seed % 2])
        assert len(A.edges) == T.N_STATES + 1
        assert sum(k >= 0 for k, _ in A.edges[T.BIG_STATE]) > 300 and A.edges[T.VRT_ONLY_STATE] == ((VRT, A.edges[T.VRT_ONLY_STATE][0][1]),)
        kinds = {k for st in A.edges for k, _ in st if k < 0}
        assert kinds == {VRT, TEXT, EOS}


# ------------------------------------------------------------------------------------------------------------ the packed table, the C ABI
def test_packed_table_layout():
    A = TA([[(7, 1), (VRT, 0), (EOS, 2)], [(TEXT, 0)], []], start=1)
    t = ops.token_automaton_tensor(A).tolist()
    assert t == [ops.TOKEN_AUTOMATON_MAGIC, 3, 4, 1,   0, 3, 4, 4,   EOS, 2, VRT, 0, 7, 1,   TEXT, 0]
    assert torch.equal(ops.token_automaton_tensor(key=A.key), ops.token_automaton_tensor(A))


def test_header_and_wrapper_argument_lists():
    decl = _lib.parse_header()
    assert decl["padt_token_automaton"][2] == ["stream", "table", "table_ints", "gen_cfg", "vrt_off", "tokens", "ld_tokens", "step", "unfinished",
                                               "state", "ban", "ban_words", "rules_ban", "n_cols", "vocab", "batch"]
    assert "padt_token_automaton_f16" not in _lib.parse_header(_lib.HEADER_F16)           # type-independent: compiled once
    assert hasattr(_lib.load(), "padt_token_automaton")
    p = inspect.signature(ops.token_automaton).parameters
    assert list(p) == ["table", "gen_cfg", "vrt_off", "tokens", "step", "unfinished", "state", "ban", "n_cols", "vocab", "rules_ban"]
    assert p["rules_ban"].default is None
    assert list(inspect.signature(ops.token_automaton_tensor).parameters) == ["automaton", "key"]
    # the wrappers this feature leaves alone keep their lists
    assert list(inspect.signature(ops.gen_rules).parameters) == ["rules", "hist", "hist_len", "tokens", "step", "ban", "n_cols"]
    assert list(inspect.signature(ops.vrt_head).parameters)[-2:] == ["ban", "part_sum"]


# ------------------------------------------------------------------------------------------------------------ options, entry points
def hf_defaults():
    from types import SimpleNamespace
    return SimpleNamespace(repetition_penalty=1.0, eos_token_id=[7], pad_token_id=0, do_sample=False, temperature=1.0, top_k=50, top_p=1.0,
                           no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None)


def test_the_option_is_part_of_equality_hash_and_repr_and_selects_a_step_mode():
    a, b = TA.from_sequences([[5, VRT], [6, VRT]]), TA.from_sequences([[6, VRT], [5, VRT]])
    c = TA.from_sequences([[5, VRT]])
    base = resolve_options(hf_defaults(), 7, 1000)
    assert base.automaton is None and GenOptions().automaton is None and StepMode().automaton is False
    assert base == GenOptions(eos_ids=(7,)) and "automaton=None" in repr(base)            # without the argument: today's options
    on, on_b, on_c = (dataclasses.replace(base, automaton=x.key) for x in (a, b, c))
    assert on != base and hash(on) != hash(base) and on == on_b and hash(on) == hash(on_b) and on != on_c
    assert repr(on) != repr(base) and repr(on) == repr(on_b) and repr(on) != repr(on_c)
    assert dataclasses.replace(on, keep_scores=True).automaton == a.key and dataclasses.replace(on, forced=True).automaton == a.key
    assert dataclasses.replace(on, automaton=None) == base
    assert "automaton" not in {f.name for f in dataclasses.fields(GenOptions)}
    assert on.generate_kwargs() == base.generate_kwargs() and not any("automaton" in k for k in on.generate_kwargs())
    assert "automaton" not in inspect.signature(resolve_options).parameters
    # one step mode — one captured graph — for every automaton; another than without
    assert on.step_mode() == on_c.step_mode() == base.step_mode()._replace(automaton=True) != base.step_mode()
    assert on.step_mode(processors=True).automaton and on.step_mode(reference=True).automaton


def test_every_entry_point_takes_the_argument_with_default_none():
    from padt_amd import harness, pipeline
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    p = inspect.signature(M.generate).parameters
    assert "token_automaton" not in p and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD        # popped from **kwargs, like forced_tokens
    for fn in (M.generate, M.score_completions):
        doc = inspect.getdoc(fn)
        assert "token_automaton" in doc and "ALLOWED" in doc and "closed-set" in doc
    assert "prefix_allowed_tokens_fn" in inspect.getdoc(M.generate) and "dict(automaton=" in inspect.getdoc(M.generate_launch)
    for fn in (pipeline.rec_batch, pipeline.PipelinedRunner.submit, harness.infer_dataset):
        assert inspect.signature(fn).parameters["token_automaton"].default is None
    assert inspect.signature(M.score_completions).parameters["generate_kwargs"].kind is inspect.Parameter.VAR_KEYWORD


class _Launched(Exception):
    pass


def _resolving_model():
    """An uninitialised instance whose _launch reports what generate() resolved."""
    from types import SimpleNamespace
    from padt_amd.modeling import PaDTForConditionalGeneration as M

    class Probe(M):
        def _launch(self, opts, *a, **kw):
            raise _Launched(opts, kw)
    m = object.__new__(Probe)
    m.generation_config = hf_defaults()
    m.config = SimpleNamespace(eos_token_id=7, vocab_size=1000)
    m.prefers_bf16, m.precision = False, "default"
    return m


def _resolved(m, **kw):
    with pytest.raises(_Launched) as e:
        m.generate(input_ids=torch.zeros(2, 3, dtype=torch.long), attention_mask=None, pixel_values=None, image_grid_thw=None, **kw)
    return e.value.args


def test_generate_resolves_none_to_todays_options_and_an_automaton_to_its_key():
    m = _resolving_model()
    A = TA.from_sequences([[5, VRT], [6, VRT]], repeat=True)
    plain, kw0 = _resolved(m, max_new_tokens=4)
    none, kw1 = _resolved(m, max_new_tokens=4, token_automaton=None)
    assert plain == none == GenOptions(eos_ids=(7,)) and kw0["automaton"] is None and kw1["automaton"] is None and kw1["hooks"] is None
    on, kw2 = _resolved(m, max_new_tokens=4, token_automaton=A)
    assert on.automaton == A.key and on != plain and kw2["automaton"] is A and kw2["hooks"] is None
    both, kw3 = _resolved(m, max_new_tokens=4, token_automaton=A, forced_tokens=[[5], [6]], no_repeat_ngram_size=2)
    assert both.automaton == A.key and both.forced and both.rules is not None and kw3["forced"] is not None
    with pytest.raises(ValueError, match="token_automaton"):
        _resolved(m, max_new_tokens=4, token_automaton=lambda b, ids: [1])
    with pytest.raises(ValueError, match="token_automaton.*id 1000"):
        _resolved(m, max_new_tokens=4, token_automaton=TA([[(1000, 0)]]))


def test_the_refused_names_are_still_refused():
    for name in ("prefix_allowed_tokens_fn", "sequence_bias", "forced_eos_token_id", "constraints"):
        exc = ValueError if name == "constraints" else NotImplementedError                 # never a known name here: HF's unused-kwarg error
        with pytest.raises(exc, match=name):
            check_generate_kwargs({name: [1]}, 4, None, 3)
    for name, v in (("force_words_ids", [[1]]), ("min_new_tokens", 2), ("num_beams", 2)):
        with pytest.raises(NotImplementedError, match=name):
            check_generate_kwargs({name: v}, 4, None, 3)
    with pytest.raises(ValueError, match="token_automaton"):                               # left in **kwargs it is a stray keyword
        check_generate_kwargs({"token_automaton": 1}, 4, None, 3)
    m = _resolving_model()
    with pytest.raises(NotImplementedError, match="prefix_allowed_tokens_fn"):
        m.generate(input_ids=torch.zeros(1, 3, dtype=torch.long), attention_mask=None, pixel_values=None, image_grid_thw=None, max_new_tokens=4,
                   prefix_allowed_tokens_fn=lambda b, ids: [1])


def test_the_bf16_rerun_passes_the_automaton_object_on():
    import warnings
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    calls = []

    class Twin:
        def generate(self, **kw):
            calls.append(kw)
            return "out"

    me = object.__new__(M)
    me.operands, me.dtype, me.overflow_reruns, me.prefers_bf16, me._batches_seen, me._fallback = "auto", torch.float16, 0, False, 10, Twin()
    me.precision, me._sd_factory = "default", (lambda: None)
    A = TA.from_sequences([[5, VRT]])
    for auto in (A, None):
        opts = dataclasses.replace(GenOptions(eos_ids=(7,)), automaton=None if auto is None else auto.key)
        group = dict(opts=opts, T_max=4, schedule=None, sync_every=4, use_graph=True, lane=0)
        sub = dict(inputs=(None, None, None, None), input_ids=None, forced=None, automaton=auto)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert me._non_finite_batch(group, sub, True, True, False, False) == "out"
    assert calls[0]["token_automaton"] is A and "token_automaton" not in calls[1]
