"""generation.GenOptions: what generate_launch's arguments and the checkpoint's generation_config resolve to (resolve_options), that equality
of two option sets is decode-group compatibility, that generate_kwargs() spells an option set as explicit arguments which resolve back to it
under any generation_config (the range guard's re-run on the bf16 twin), and which options select the decode step's kernel sequence
(StepMode: the captured-graph key).  Host logic only: no model, no GPU."""
import dataclasses
import inspect
import itertools
from types import SimpleNamespace

import pytest
import torch

from padt_amd.generation import GenOptions, Sampling, StepMode, resolve_options

EOS, VOCAB = 7, 1000


def hf_defaults():
    """the generation_config of a model whose checkpoint carries none (HF GenerationConfig defaults)"""
    return SimpleNamespace(repetition_penalty=1.0, eos_token_id=[EOS], pad_token_id=0, do_sample=False, temperature=1.0, top_k=50, top_p=1.0,
                           no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None)


def checkpoint():
    """... and one whose every field differs from them"""
    return SimpleNamespace(repetition_penalty=1.2, eos_token_id=[EOS, 9], pad_token_id=0, do_sample=True, temperature=0.7, top_k=20, top_p=0.9,
                           no_repeat_ngram_size=3, bad_words_ids=[[4, 5], [6]], suppress_tokens=[11], begin_suppress_tokens=[12])


def resolve(gc, **kw):
    return resolve_options(gc, EOS, VOCAB, **kw)


ALL_RULES = dict(no_repeat_ngram_size=3, bad_words_ids=[[40, 41, 42], [43]], suppress_tokens=[50, 51], begin_suppress_tokens=[60])


# ------------------------------------------------------------------------------------------------------------ resolution
def test_defaults_come_from_the_generation_config():
    o = resolve(checkpoint(), seed=5)
    assert o == GenOptions(1.2, (EOS, 9), Sampling(0.7, 20, 0.9, 5), (3, (6, 11), (12,), ((4, 5),)))
    assert isinstance(o.sampling, Sampling) and o.sampling.top_k == 20 and o.sampling.seed == 5
    assert resolve(hf_defaults()) == GenOptions(eos_ids=(EOS,))


def test_explicit_arguments_win_off_values_included():
    off = resolve(checkpoint(), do_sample=False, repetition_penalty=1.0, eos_token_id=EOS, no_repeat_ngram_size=0, bad_words_ids=[],
                  suppress_tokens=[], begin_suppress_tokens=[])
    assert off == GenOptions(eos_ids=(EOS,))
    on = resolve(checkpoint(), temperature=2, top_k=3, top_p=1, seed=11, repetition_penalty=2, eos_token_id=[9, EOS, 8])
    assert on.sampling == Sampling(2.0, 3, 1.0, 11) and on.repetition_penalty == 2.0 and on.eos_ids == (9, EOS, 8)
    assert isinstance(on.sampling.temperature, float) and isinstance(on.repetition_penalty, float)
    flags = resolve(hf_defaults(), keep_scores=1, output_token_logprobs=1, top_logprobs=4, output_patch_logprobs=1)
    assert (flags.keep_scores, flags.token_logprobs, flags.top_logprobs, flags.patch_logprobs) == (True, True, 4, True)
    assert resolve(hf_defaults(), top_logprobs=None).top_logprobs == 0


def test_sampling_among_the_single_best_token_is_greedy():
    assert resolve(hf_defaults(), do_sample=True, top_k=1).sampling is None
    gc = checkpoint()
    gc.top_k = 1
    assert resolve(gc).sampling is None
    assert resolve(hf_defaults(), do_sample=True, top_k=2, seed=0).sampling is not None


def test_eos_as_an_int_and_as_a_list():
    assert resolve(hf_defaults(), eos_token_id=EOS).eos_ids == (EOS,)
    assert resolve(hf_defaults(), eos_token_id=[3, EOS]).eos_ids == (3, EOS)
    assert resolve(hf_defaults(), eos_token_id=torch.tensor([EOS, 2])).eos_ids == (EOS, 2)


@pytest.mark.parametrize("exc,match,kw", [
    (ValueError, "temperature", dict(do_sample=True, temperature=0.0)),
    (ValueError, "temperature", dict(do_sample=True, temperature=-1)),
    (NotImplementedError, "top_p", dict(do_sample=True, top_p=0.9, top_k=0)),
    (NotImplementedError, "top_p", dict(do_sample=True, top_p=0.9, top_k=1025)),
    (NotImplementedError, "eos_token_id", dict(eos_token_id=[3, 4])),
    (NotImplementedError, "eos_token_id", dict(eos_token_id=[EOS, 1, 2, 3, 4])),
    (NotImplementedError, "output_logits", dict(keep_logits=True, suppress_tokens=[5])),
    (NotImplementedError, "output_logits", dict(keep_logits=True, no_repeat_ngram_size=2)),
    (ValueError, "top_logprobs", dict(top_logprobs=-1)),
    (ValueError, "top_logprobs", dict(top_logprobs=2.5)),
    (NotImplementedError, "top_logprobs=33", dict(top_logprobs=33)),
    (NotImplementedError, "bad_words_ids", dict(bad_words_ids=[[VOCAB]])),
])
def test_refusals_keep_their_type_and_name_the_argument(exc, match, kw):
    with pytest.raises(exc, match=match):
        resolve(hf_defaults(), **kw)


def test_what_is_not_refused():
    assert resolve(hf_defaults(), temperature=0.0).sampling is None                       # the warpers' checks apply under sampling only
    assert resolve(hf_defaults(), do_sample=True, top_p=0.9, top_k=1024, seed=1).sampling.top_k == 1024
    o = resolve(hf_defaults(), do_sample=True, seed=1, keep_scores=True, keep_logits=True, suppress_tokens=[5])
    assert o.keep_logits and o.rules is not None                                          # under sampling the raw rows have a stash of their own
    g = resolve(hf_defaults(), keep_scores=True, keep_logits=True)
    assert g.keep_scores and not g.keep_logits                                            # greedy: the logits ARE the scores


def test_the_seed_is_drawn_from_the_global_generator_only_when_sampling_without_one():
    torch.manual_seed(1234)
    a = resolve(hf_defaults(), do_sample=True).sampling.seed
    b = resolve(hf_defaults(), do_sample=True).sampling.seed
    torch.manual_seed(1234)
    assert resolve(hf_defaults(), do_sample=True).sampling.seed == a and a != b and 0 <= a < 2 ** 31 - 1
    state = torch.get_rng_state()
    resolve(hf_defaults())                                                                # greedy
    resolve(checkpoint(), do_sample=False)
    resolve(hf_defaults(), do_sample=True, top_k=1)                                       # greedy after all
    resolve(checkpoint(), seed=3)                                                         # sampling with a seed
    assert torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------------------------------------------------------------ equality
def test_any_single_field_makes_two_option_sets_unequal():
    base = resolve(hf_defaults(), do_sample=True, seed=1, **ALL_RULES)
    other = dict(repetition_penalty=1.3, eos_ids=(EOS, 9), sampling=None, rules=None, keep_scores=True, keep_logits=True, token_logprobs=True,
                 top_logprobs=3, patch_logprobs=True)
    assert set(other) == {f.name for f in dataclasses.fields(GenOptions)}
    for name, v in other.items():
        assert dataclasses.replace(base, **{name: v}) != base, name
    for i, v in enumerate((0.5, 21, 0.5, 2)):                                             # ... and so does every sampling setting, the seed included
        assert dataclasses.replace(base, sampling=base.sampling._replace(**{Sampling._fields[i]: v})) != base
    assert dataclasses.replace(base, rules=(2,) + base.rules[1:]) != base
    assert dataclasses.replace(base) == base and hash(dataclasses.replace(base)) == hash(base)
    with pytest.raises(dataclasses.FrozenInstanceError):
        base.keep_scores = True


def test_bans_as_lists_tuples_or_in_another_order_are_one_option_set():
    a = resolve(hf_defaults(), **ALL_RULES)
    b = resolve(hf_defaults(), no_repeat_ngram_size=3, bad_words_ids=((43,), (40, 41, 42), (43,)), suppress_tokens=(51, 50, 51),
                begin_suppress_tokens=torch.tensor([60]))
    c = resolve(hf_defaults(), no_repeat_ngram_size=3, bad_words_ids=[[40, 41, 42]], suppress_tokens=[43, 50, 51], begin_suppress_tokens=[60])
    assert a == b == c and hash(a) == hash(b) == hash(c) and len({a, b, c}) == 1
    assert a != resolve(hf_defaults(), **dict(ALL_RULES, suppress_tokens=[50]))


# ------------------------------------------------------------------------------------------------------------ round trip
def option_grid(gc):
    for samp, rules, pen, lp, top, patch, scores in itertools.product(
            (dict(do_sample=False), dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=17)),
            (dict(no_repeat_ngram_size=0, bad_words_ids=[], suppress_tokens=[], begin_suppress_tokens=[]), ALL_RULES), (1.0, 1.3), (False, True),
            (0, 5), (False, True), (False, True)):
        yield resolve(gc, repetition_penalty=pen, keep_scores=scores, output_token_logprobs=lp, top_logprobs=top, output_patch_logprobs=patch,
                      **samp, **rules)


@pytest.mark.parametrize("gc", [hf_defaults, checkpoint])
def test_generate_kwargs_resolve_back_to_the_options(gc):
    n = 0
    for o in option_grid(gc()):
        kw = o.generate_kwargs()
        assert all(v is not None for v in kw.values()), kw                               # an off value is spelled as off, never as "the default"
        for other in (hf_defaults(), checkpoint()):                                       # ... so no generation_config can switch it back on
            assert resolve(other, keep_scores=o.keep_scores, keep_logits=o.keep_logits, **kw) == o
        n += 1
    assert n == 128
    o = resolve(gc(), do_sample=True, seed=2, keep_scores=True, keep_logits=True, **ALL_RULES)      # output_logits under sampling
    assert o.keep_logits and resolve(gc(), keep_scores=True, keep_logits=True, **o.generate_kwargs()) == o
    assert set(o.generate_kwargs()) <= set(inspect.signature(resolve_options).parameters)


# ------------------------------------------------------------------------------------------------------------ derived facts, step mode
def test_derived_facts():
    g, s = resolve(hf_defaults()), resolve(hf_defaults(), do_sample=True, seed=1)
    assert not g.want_rows and not g.write_back and not g.reads_prompt and not s.write_back
    for kw in (dict(keep_scores=True), dict(output_token_logprobs=True), dict(top_logprobs=2), dict(output_patch_logprobs=True)):
        assert resolve(hf_defaults(), do_sample=True, seed=1, **kw).write_back and not resolve(hf_defaults(), **kw).write_back, kw
    assert resolve(hf_defaults(), top_logprobs=2).want_rows and resolve(hf_defaults(), output_patch_logprobs=True).want_rows
    assert resolve(hf_defaults(), repetition_penalty=1.1).reads_prompt and resolve(hf_defaults(), suppress_tokens=[3]).reads_prompt


def test_the_step_mode_is_what_selects_the_kernel_sequence():
    base = resolve(hf_defaults(), do_sample=True, seed=1, suppress_tokens=[3])
    mode = base.step_mode()
    assert isinstance(mode, StepMode) and mode == StepMode(sampling=True, rules=True) and GenOptions().step_mode() == StepMode()
    # read from device memory by the captured step: the graph is shared
    for same in (dict(repetition_penalty=1.3), dict(eos_token_id=[EOS, 9]), dict(seed=2), dict(temperature=0.5, top_k=3, top_p=0.5),
                 dict(suppress_tokens=[4, 5], no_repeat_ngram_size=2)):
        assert resolve(hf_defaults(), **dict(dict(do_sample=True, seed=1, suppress_tokens=[3]), **same)).step_mode() == mode, same
    # another kernel sequence or output buffer: a graph of its own
    modes = {mode}
    for other in (dict(do_sample=False), dict(suppress_tokens=[]), dict(keep_scores=True), dict(keep_scores=True, keep_logits=True),
                  dict(output_token_logprobs=True), dict(top_logprobs=3), dict(top_logprobs=4), dict(output_patch_logprobs=True)):
        m = resolve(hf_defaults(), **dict(dict(do_sample=True, seed=1, suppress_tokens=[3]), **other)).step_mode()
        assert m not in modes, other
        modes.add(m)
    assert base.step_mode(processors=True) not in modes and base.step_mode(reference=True) not in modes
    assert base.step_mode(processors=True) != base.step_mode(reference=True)
    assert base.step_mode(processors=[object()], reference=1) == mode._replace(processors=True, reference=True)


# ------------------------------------------------------------------------------------------------------------ frozen signatures
def test_the_public_signatures_did_not_move():
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    assert list(inspect.signature(M.generate).parameters) == [
        "self", "input_ids", "attention_mask", "pixel_values", "image_grid_thw", "use_cache", "max_new_tokens", "do_sample", "output_hidden_states",
        "return_dict_in_generate", "synced_gpus", "schedule", "sync_every", "use_graph", "lane", "repetition_penalty", "eos_token_id", "temperature",
        "top_k", "top_p", "seed", "max_length", "output_scores", "output_logits", "pad_token_id", "logits_processor", "stopping_criteria",
        "no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "generation_config", "image_index",
        "output_token_logprobs", "top_logprobs", "output_patch_logprobs", "kwargs"]
    launch = ["self", "input_ids", "attention_mask", "pixel_values", "image_grid_thw", "max_new_tokens", "do_sample", "schedule", "sync_every",
              "use_graph", "lane", "decode_stream", "group", "n_slots", "repetition_penalty", "eos_token_id", "temperature", "top_k", "top_p", "seed",
              "vit_stream", "inputs_ready", "keep_scores", "hooks", "keep_logits", "no_repeat_ngram_size", "bad_words_ids", "suppress_tokens",
              "begin_suppress_tokens", "image_index", "output_token_logprobs", "top_logprobs", "output_patch_logprobs"]
    assert list(inspect.signature(M.generate_launch).parameters) == launch
    # every option argument of generate_launch is one of resolve_options, under the same name and with the same default
    res = inspect.signature(resolve_options).parameters
    for name in list(res)[3:]:
        assert name in launch and res[name].default == inspect.signature(M.generate_launch).parameters[name].default, name
