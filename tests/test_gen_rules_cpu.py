"""Host side of the device-side bans (no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens) and of
generate(generation_config=): the rule packer (ops.gen_rules_key / gen_rules_tensor: canonical form, caps, the text-id rule, HF's EOS filter),
the packed table's meaning against the installed HF classes (a host model of the kernel walks the table), and the argument policy.  No GPU and
no library: every generate() call here ends in the policy, before anything touches the model."""
from types import SimpleNamespace

import pytest
import torch

import gen_rules_util as G
from padt_amd import ops


def test_packing_round_trips_and_is_canonical():
    key = ops.gen_rules_key(3, [[9, 8, 7], [5], [9, 8, 7], [2, 2]], [40, 4, 40], [6, 1], eos_ids=[77], vocab_size=100)
    assert key == (3, (4, 5, 40), (1, 6), ((2, 2), (9, 8, 7)))               # sorted, no duplicates, the 1-token word among the static ids
    tab = ops.gen_rules_tensor(3, [[9, 8, 7], [5], [9, 8, 7], [2, 2]], [40, 4, 40], [6, 1], eos_ids=[77], vocab_size=100)
    assert tab.dtype == torch.int32 and tab.shape == (ops.GEN_RULES_INTS,)
    assert ops.gen_rules_unpack(tab) == key
    assert torch.equal(tab, ops.gen_rules_tensor(key=key))
    # another order / another container of the same rules: the same key (batches of a merged decode group compare it)
    assert ops.gen_rules_key(3, ((2, 2), (9, 8, 7), (5,)), (4, 40), torch.tensor([1, 6]), eos_ids=(77,), vocab_size=100) == key
    # nothing banned: no key (no kernel, no bitmap), and the table of "nothing" is all zero
    for off in (dict(), dict(no_repeat_ngram_size=0, bad_words_ids=[], suppress_tokens=[], begin_suppress_tokens=[]),
                dict(no_repeat_ngram_size=None, bad_words_ids=None), dict(bad_words_ids=[[77]], eos_ids=[77])):
        assert ops.gen_rules_key(vocab_size=100, **off) is None
    assert not ops.gen_rules_tensor(vocab_size=100).any()
    # every kind alone makes a key
    for on in (dict(no_repeat_ngram_size=1), dict(bad_words_ids=[[1]]), dict(bad_words_ids=[[1, 2]]), dict(suppress_tokens=[0]),
               dict(begin_suppress_tokens=[99])):
        assert ops.gen_rules_key(vocab_size=100, **on) is not None


def test_eos_single_token_bad_words_are_dropped_as_hf_does():
    # NoBadWordsLogitsProcessor filters the words equal to [eos] for any EOS id; longer words ending in EOS and suppress_tokens=[eos] stay
    key = ops.gen_rules_key(0, [[7], [9], [3, 7], [5]], [9], None, eos_ids=[7, 5], vocab_size=50)
    assert key == (0, (9,), (), ((3, 7),))
    rules = dict(bad_words_ids=[[7], [9], [3, 7], [5]])
    for hist in ([3], [1, 3], [7, 3]):
        assert torch.equal(G.table_ban(ops.gen_rules_tensor(eos_ids=[7, 5], vocab_size=50, **rules), hist, 0, 50), G.hf_ban(rules, [7, 5], hist, 1, 50))


@pytest.mark.parametrize("kw,exc,name", [
    (dict(no_repeat_ngram_size=17), NotImplementedError, "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=-1), ValueError, "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=2.5), ValueError, "no_repeat_ngram_size"),
    (dict(bad_words_ids=[list(range(17))]), NotImplementedError, "bad_words_ids"),
    (dict(bad_words_ids=[[]]), ValueError, "bad_words_ids"),
    (dict(bad_words_ids=[3]), ValueError, "bad_words_ids"),
    (dict(bad_words_ids=[[1, -2]]), ValueError, "bad_words_ids"),
    (dict(bad_words_ids=[[1, 100]]), NotImplementedError, "bad_words_ids"),                  # a VRT id (>= vocab_size) as a word's last id
    (dict(bad_words_ids=[[100, 1]]), NotImplementedError, "bad_words_ids"),
    (dict(suppress_tokens=[100]), NotImplementedError, "suppress_tokens"),
    (dict(suppress_tokens=[1.5]), ValueError, "suppress_tokens"),
    (dict(begin_suppress_tokens=[3, 250]), NotImplementedError, "begin_suppress_tokens"),
    (dict(suppress_tokens=list(range(4093)), vocab_size=5000), NotImplementedError, "suppress_tokens"),      # 4 + 4093 ints: one too many
    (dict(bad_words_ids=[[i, i + 1, i + 2] for i in range(900)], vocab_size=5000), NotImplementedError, "bad_words_ids"),     # 4 + 900 * (1 + 1 + 3)
])
def test_caps_and_the_text_id_rule_raise_by_name(kw, exc, name):
    with pytest.raises(exc, match=name):
        ops.gen_rules_key(**dict(dict(vocab_size=100), **kw))


def test_the_caps_themselves_pack():
    key = ops.gen_rules_key(16, [list(range(16))], list(range(4092 - 18)), None, vocab_size=5000)
    assert ops.gen_rules_unpack(ops.gen_rules_tensor(key=key)) == key       # 4 + 4074 static + 1 offset + 17: exactly 4096 ints


def test_packed_table_means_what_the_hf_classes_do():
    """The kernel's statement, walked on the host over the packed table, against the installed HF classes on the GPU test's seeded cases —
    and the conditions those cases are chosen for: most have a non-empty ban set, every rule kind bites in at least 10 of them."""
    n_rows = nonempty = 0
    bites = dict.fromkeys(G.KINDS, 0)
    for seed in range(G.N_CASES):
        rules, lens, t, tokens, prompts = G.random_case(seed)
        tab = ops.gen_rules_tensor(eos_ids=G.EOS, vocab_size=G.V, **rules)
        hit = set()
        for L, p, tk in zip(lens, prompts, tokens):
            want = G.hf_ban(rules, G.EOS, p + tk, L, G.WIDTH)
            assert torch.equal(G.table_ban(tab, p + tk, t, G.WIDTH), want), (seed, rules, p, tk)
            n_rows += 1
            nonempty += bool(want.any())
            hit |= {k for k in G.KINDS if G.hf_ban(rules, G.EOS, p + tk, L, G.WIDTH, kinds=(k,)).any()}
        for k in hit:
            bites[k] += 1
    assert nonempty >= 0.9 * n_rows, (nonempty, n_rows)
    assert min(bites.values()) >= 10, bites


# ------------------------------------------------------------------------------------------------ generate() argument policy
class _Launched(Exception):
    pass


def _model():
    """An uninitialised instance whose generate_launch reports what generate() resolved: the policy runs before anything touches the model."""
    from padt_amd.modeling import PaDTForConditionalGeneration
    m = PaDTForConditionalGeneration.__new__(PaDTForConditionalGeneration)
    m.generation_config = SimpleNamespace(pad_token_id=0, repetition_penalty=1.0)

    def launch(input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens, do_sample, *a, **kw):
        raise _Launched(dict(kw, max_new_tokens=max_new_tokens, do_sample=do_sample))
    m.generate_launch = launch
    return m


def _resolved(m, **kw):
    with pytest.raises(_Launched) as e:
        m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), **kw)
    return e.value.args[0]


def test_the_four_bans_are_named_parameters_and_reach_the_launch():
    got = _resolved(_model(), max_new_tokens=3, no_repeat_ngram_size=2, bad_words_ids=[[1, 2]], suppress_tokens=[5], begin_suppress_tokens=[6])
    assert (got["no_repeat_ngram_size"], got["bad_words_ids"], got["suppress_tokens"], got["begin_suppress_tokens"]) == (2, [[1, 2]], [5], [6])
    got = _resolved(_model(), max_new_tokens=3)
    assert got["no_repeat_ngram_size"] is None and got["bad_words_ids"] is None           # None: the checkpoint's generation_config decides


def test_generation_config_object_and_dict_are_accepted_and_explicit_arguments_win():
    from transformers import GenerationConfig
    gc = GenerationConfig(no_repeat_ngram_size=3, bad_words_ids=[[1, 2]], suppress_tokens=[7], begin_suppress_tokens=[8], max_new_tokens=11,
                          repetition_penalty=1.2, do_sample=True, top_k=9, temperature=0.5)
    for cfg in (gc, gc.to_dict(), dict(no_repeat_ngram_size=3, bad_words_ids=[[1, 2]], suppress_tokens=[7], begin_suppress_tokens=[8],
                                       max_new_tokens=11, repetition_penalty=1.2, do_sample=True, top_k=9, temperature=0.5)):
        if isinstance(cfg, dict):
            cfg = {k: v for k, v in cfg.items() if v is not None and k in gc.to_diff_dict()}
        got = _resolved(_model(), generation_config=cfg)
        assert got["max_new_tokens"] == 11 and got["do_sample"] is True and got["top_k"] == 9 and got["temperature"] == 0.5
        assert got["repetition_penalty"] == 1.2 and got["no_repeat_ngram_size"] == 3 and got["bad_words_ids"] == [[1, 2]]
        assert got["suppress_tokens"] == [7] and got["begin_suppress_tokens"] == [8]
        # explicit arguments win, as in HF — "off" values included
        got = _resolved(_model(), generation_config=cfg, max_new_tokens=4, no_repeat_ngram_size=0, bad_words_ids=[], do_sample=False, top_k=50)
        assert got["max_new_tokens"] == 4 and got["no_repeat_ngram_size"] == 0 and got["bad_words_ids"] == [] and got["do_sample"] is False
        assert got["top_k"] == 50 and got["suppress_tokens"] == [7] and got["repetition_penalty"] == 1.2
    assert _resolved(_model(), generation_config=GenerationConfig(), max_new_tokens=2)["max_new_tokens"] == 2      # a default config changes nothing
    assert _resolved(_model(), generation_config={}, max_new_tokens=2)["no_repeat_ngram_size"] is None
    assert _resolved(_model(), generation_config=dict(output_scores=True), max_new_tokens=2)["keep_scores"] is True


def test_generation_config_fields_go_through_the_keyword_policy():
    from transformers import GenerationConfig
    m = _model()
    for cfg in (GenerationConfig(num_beams=4), dict(num_beams=4)):
        with pytest.raises(NotImplementedError, match="num_beams"):
            m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, generation_config=cfg)
    for field, value in (("min_new_tokens", 3), ("min_length", 5), ("sequence_bias", {(1,): -1.0}), ("forced_eos_token_id", 2), ("penalty_alpha", 0.6)):
        with pytest.raises(NotImplementedError, match=field):
            m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, generation_config={field: value})
    with pytest.raises(ValueError, match="not used by the model.*no_such_field"):
        m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, generation_config=dict(no_such_field=1))
    with pytest.raises(NotImplementedError, match="pad_token_id"):                       # a named field is checked like the argument
        m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, generation_config=dict(pad_token_id=5))
    # benign fields pass (bos_token_id, the bookkeeping entries of a saved config)
    assert _resolved(m, generation_config=dict(bos_token_id=1, transformers_version="5.0", _from_model_config=True), max_new_tokens=2)["max_new_tokens"] == 2


@pytest.mark.parametrize("value", [object(), "greedy", 3, [("num_beams", 1)]], ids=["object", "str", "int", "list"])
def test_a_non_config_object_raises_naming_generation_config(value):
    with pytest.raises(NotImplementedError, match="generation_config"):
        _model().generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, generation_config=value)


def test_stray_keywords_stay_refused_and_load_generation_config_reads_the_fields():
    from padt_amd.modeling import PaDTForConditionalGeneration, check_generate_kwargs
    for k, v in (("no_repeat_ngram_size", 2), ("bad_words_ids", [[1]]), ("suppress_tokens", [1]), ("begin_suppress_tokens", [1])):
        with pytest.raises(NotImplementedError, match=k):
            check_generate_kwargs({k: v}, 4, None, 9)
        assert check_generate_kwargs({k: None}, 4, None, 9) == 4
    m = PaDTForConditionalGeneration.__new__(PaDTForConditionalGeneration)
    m.generation_config = SimpleNamespace(repetition_penalty=1.0, eos_token_id=[1], pad_token_id=0, do_sample=False, temperature=1.0, top_k=50, top_p=1.0,
                                          no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None)
    g = m.load_generation_config({"no_repeat_ngram_size": 3, "bad_words_ids": [[4, 5], [6]], "suppress_tokens": [7], "begin_suppress_tokens": [8, 9]})
    assert (g.no_repeat_ngram_size, g.bad_words_ids, g.suppress_tokens, g.begin_suppress_tokens) == (3, [[4, 5], [6]], [7], [8, 9])
