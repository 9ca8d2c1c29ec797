"""generate(min_p=, typical_p=, epsilon_cutoff=, eta_cutoff=) without a GPU: the fp64 reference chain the GPU tests compare the kernel with is
pinned to HF's own classes, and the four values resolve into GenOptions from every source a generate() call has."""
import inspect
from types import SimpleNamespace

import pytest
import torch

import sampling_warpers_util as U
from padt_amd.generation import WARPER_NAMES, GenOptions, Sampling, StepMode, resolve_options, with_warpers

EOS, VOCAB = 7, 100
WARP = dict(min_p=0.1, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=1e-2)


# ------------------------------------------------------------------------------------------------------------ the reference chain is HF's
@pytest.mark.parametrize("n", U.WIDTHS)
@pytest.mark.parametrize("T", [1.0, 0.7])
def test_the_reference_chain_has_hf_support(n, T):
    rows = U.make_rows(n, T)
    for setting in U.SINGLE + [U.COMBINED]:
        hf = U.hf_support(rows, **setting)
        for r in range(rows.shape[0]):
            kept, amb = U.ref_chain(rows[r], **setting)
            assert kept.any() and not (kept & ~(rows[r] > float("-inf"))).any()
            U.check_support(hf[r], kept, amb, U.AMBIGUOUS_MAX, f"n={n} T={T} {U.setting_id(setting)} row {r}")


def test_the_reference_chain_on_planted_rows():
    ninf = float("-inf")
    # a typical-p cut inside a run of equal keys: p = (.4, .15 x 4): the key of the four equal entries is the smaller one, the cumulative mass
    # reaches 0.4 at the third of them, all four stay and the 0.4 entry goes
    row = torch.tensor([0.4, 0.15, 0.15, 0.15, 0.15]).log()
    kept, amb = U.ref_chain(row, typical_p=0.4)
    assert kept.tolist() == [False, True, True, True, True] and not amb.any()
    assert U.hf_support(row[None], typical_p=0.4)[0].tolist() == kept.tolist()
    # entries tied with the top score stay under any epsilon; min_p = 1 keeps the top ties only
    row = torch.tensor([1.0, ninf, 1.0, 0.5, 1.0, -3.0])
    assert U.ref_chain(row, eps=0.9)[0].tolist() == [True, False, True, False, True, False]
    assert U.ref_chain(row, eta=0.9)[0].tolist() == [True, False, True, False, True, False]
    assert U.ref_chain(row, min_p=1.0)[0].tolist() == [True, False, True, False, True, False]
    assert U.hf_support(row[None], eps=0.9)[0].tolist() == [True, False, True, False, True, False]
    # one survivor stays, a row without any has none
    row = torch.tensor([ninf, 2.0, ninf])
    assert U.ref_chain(row, **U.COMBINED)[0].tolist() == [False, True, False]
    assert not U.ref_chain(torch.full((5,), ninf), **U.COMBINED)[0].any()


def test_the_planted_rows_of_the_gpu_test_are_what_they_claim():
    rows, expect, settings = U.planted_rows()
    for r, setting in enumerate(settings):
        kept, amb = U.ref_chain(rows[r], **setting)
        assert torch.equal(kept, expect[r]), (r, setting, kept.nonzero().flatten().tolist()[:8])
        if r != 1:                                                # row 1: 6000 ranks of mass 1e-4 each, some within the band of typical_p
            assert not amb.any(), r
        if expect[r].any():
            assert torch.equal(U.hf_support(rows[r][None], **setting)[0], expect[r]), (r, setting)
    assert int((rows[1] > float("-inf")).sum()) > 4096 and not expect[1][rows[1].argmax()]


# ------------------------------------------------------------------------------------------------------------ resolve_options
def hf_defaults():                                                # no attribute for the four: off
    return SimpleNamespace(repetition_penalty=1.0, eos_token_id=[EOS], pad_token_id=0, do_sample=False, temperature=1.0, top_k=50, top_p=1.0,
                           no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None)


def populated():
    return SimpleNamespace(repetition_penalty=1.2, eos_token_id=[EOS, 9], pad_token_id=0, do_sample=True, temperature=0.7, top_k=20, top_p=0.9,
                           no_repeat_ngram_size=3, bad_words_ids=[[4, 5]], suppress_tokens=[11], begin_suppress_tokens=[12],
                           min_p=0.3, typical_p=0.4, epsilon_cutoff=0.02, eta_cutoff=0.03)


def resolve(gc, **kw):
    """resolve_options as generate_launch calls it: the call's four warper values in front of the config's (with_warpers)"""
    warp = {k: kw.pop(k) for k in WARPER_NAMES if k in kw}
    return resolve_options(with_warpers(gc, warp), EOS, VOCAB, **kw)


def test_the_four_values_arrive_in_the_sampling_options():
    s = resolve(hf_defaults(), do_sample=True, seed=3, **WARP).sampling
    assert s == Sampling(1.0, 50, 1.0, 3, 0.1, 0.9, 1e-3, 1e-2) and s.warpers
    assert (s.min_p, s.typical_p, s.epsilon_cutoff, s.eta_cutoff) == (0.1, 0.9, 1e-3, 1e-2)
    s = resolve(populated(), seed=3).sampling                      # from the checkpoint's generation_config
    assert (s.min_p, s.typical_p, s.epsilon_cutoff, s.eta_cutoff) == (0.3, 0.4, 0.02, 0.03)
    s = resolve(populated(), seed=3, min_p=0.0, eta_cutoff=0.5).sampling      # an explicit argument wins, an "off" included
    assert (s.min_p, s.typical_p, s.epsilon_cutoff, s.eta_cutoff) == (0.0, 0.4, 0.02, 0.5)
    assert Sampling(0.7, 20, 0.9, 5) == Sampling(0.7, 20, 0.9, 5, 0.0, 1.0, 0.0, 0.0) and not Sampling(0.7, 20, 0.9, 5).warpers


def test_values_hf_builds_no_warper_for_are_off():
    plain = resolve(hf_defaults(), do_sample=True, seed=1)
    assert plain.sampling[4:] == (0.0, 1.0, 0.0, 0.0) and not plain.sampling.warpers and not plain.write_back
    assert resolve(hf_defaults(), do_sample=True, seed=1, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0) == plain
    assert resolve(hf_defaults(), do_sample=True, seed=1, min_p=0, typical_p=1, epsilon_cutoff=0, eta_cutoff=0) == plain
    g = hf_defaults()
    g.min_p = g.typical_p = g.epsilon_cutoff = g.eta_cutoff = None                      # a GenerationConfig's own defaults for three of them
    assert resolve(g, do_sample=True, seed=1) == plain
    # under greedy decoding nothing is set, as in HF
    assert resolve(hf_defaults(), **WARP) == resolve(hf_defaults()) and resolve(hf_defaults(), **WARP).sampling is None
    assert resolve(populated(), do_sample=False).sampling is None
    assert resolve(hf_defaults(), do_sample=True, top_k=1, **WARP).sampling is None    # sampling among one token is the arg-max


@pytest.mark.parametrize("name, value", [("min_p", -0.1), ("min_p", 1.5), ("typical_p", 0.0), ("typical_p", 1.2), ("typical_p", -1), ("epsilon_cutoff", 1.0),
                                         ("epsilon_cutoff", -0.5), ("eta_cutoff", 1.0), ("eta_cutoff", 2), ("min_p", "0.1"), ("eta_cutoff", float("nan"))])
def test_out_of_range_values_raise_naming_the_argument(name, value):
    with pytest.raises(ValueError, match=name):
        resolve(hf_defaults(), do_sample=True, seed=1, **{name: value})
    g = hf_defaults()
    setattr(g, name, value)
    with pytest.raises(ValueError, match=name):                   # ... from the checkpoint's config too
        resolve(g, do_sample=True, seed=1)
    for ok_name, ok in (("min_p", 0.0), ("min_p", 1.0), ("typical_p", 1.0), ("epsilon_cutoff", 0.0), ("eta_cutoff", 0.999)):
        resolve(hf_defaults(), do_sample=True, seed=1, **{ok_name: ok})


def test_a_changed_value_is_another_decode_group_and_one_graph():
    base = resolve(hf_defaults(), do_sample=True, seed=1, **WARP)
    assert base == resolve(hf_defaults(), do_sample=True, seed=1, **WARP) and hash(base) == hash(resolve(hf_defaults(), do_sample=True, seed=1, **WARP))
    for name, v in (("min_p", 0.2), ("typical_p", 0.8), ("epsilon_cutoff", 2e-3), ("eta_cutoff", 0.0)):
        other = resolve(hf_defaults(), do_sample=True, seed=1, **dict(WARP, **{name: v}))
        assert other != base, name
        assert other.step_mode() == base.step_mode(), name          # the captured step reads the values from device memory
    plain = resolve(hf_defaults(), do_sample=True, seed=1)
    assert plain != base
    # the step mode carries the flag only when a warper is active
    assert base.step_mode() == StepMode(sampling=True, warpers=True) and plain.step_mode() == StepMode(sampling=True)
    assert resolve(hf_defaults(), **WARP).step_mode() == StepMode() and not GenOptions().step_mode().warpers
    for name, v in WARP.items():
        assert resolve(hf_defaults(), do_sample=True, seed=1, **{name: v}).step_mode().warpers, name
    # the row must hold what top-k / top-p left before the new kernel reads it
    assert base.write_back and not plain.write_back


def test_the_gen_cfg_slots():
    import struct
    base = resolve(hf_defaults(), do_sample=True, seed=1, temperature=0.7, top_k=20, top_p=0.9, **WARP)
    raw = base.gen_cfg()
    assert raw.dtype == torch.int32 and raw.numel() == 16
    f = struct.unpack("<f4iiIfifii4f", raw.numpy().tobytes())
    assert f[5:12] == (1, 1, pytest.approx(0.7), 20, pytest.approx(0.9), 1, 0)          # the twelve slots before: where they were
    assert f[12:] == tuple(pytest.approx(v) for v in (0.1, 0.9, 1e-3, 1e-2))
    off = struct.unpack("<f4iiIfifii4f", resolve(hf_defaults()).gen_cfg().numpy().tobytes())
    assert off[12:] == (0.0, 1.0, 0.0, 0.0)


@pytest.mark.parametrize("gc", [hf_defaults, populated])
def test_generate_kwargs_round_trip(gc):
    for kw in (dict(do_sample=False), dict(do_sample=True, seed=17), dict(do_sample=True, seed=17, **WARP),
               dict(do_sample=True, seed=17, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)):
        o = resolve(gc(), **kw)
        spelled = dict(o.generate_kwargs(), **o.warper_kwargs())
        assert all(spelled[k] is not None for k in WARP), spelled    # off is 0.0 / 1.0, never None: no config can switch it back on
        assert set(o.generate_kwargs()) <= set(inspect.signature(resolve_options).parameters) and set(o.warper_kwargs()) == set(WARP)
        for other in (hf_defaults(), populated()):
            assert resolve(other, **spelled) == o, (kw, spelled)


# ------------------------------------------------------------------------------------------------------------ through generate()
class _Launched(Exception):
    pass


def _model(gc=None):
    """An uninitialised model whose generate_launch reports what the call resolved to."""
    from padt_amd.modeling import PaDTForConditionalGeneration
    m = PaDTForConditionalGeneration.__new__(PaDTForConditionalGeneration)
    m.generation_config = gc or hf_defaults()
    names = set(inspect.signature(resolve_options).parameters)

    def launch(input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens, do_sample, *a, **kw):
        warp = (kw.get("hooks") or {}).get("warpers", {})         # generate_launch's channel for the call's own values
        raise _Launched(resolve(m.generation_config, do_sample=do_sample, **{k: v for k, v in kw.items() if k in names},
                                **{k: v for k, v in warp.items() if v is not None}))
    m.generate_launch = launch
    return m


def _resolved(m, **kw):
    with pytest.raises(_Launched) as e:
        m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, **kw)
    return e.value.args[0]


def test_generate_takes_them_from_arguments_configs_and_the_checkpoint():
    from transformers import GenerationConfig
    want = (0.1, 0.9, 1e-3, 1e-2)
    assert _resolved(_model(), do_sample=True, seed=1, **WARP).sampling[4:] == want
    for cfg in (dict(do_sample=True, **WARP), GenerationConfig(do_sample=True, **WARP)):
        assert _resolved(_model(), generation_config=cfg, seed=1).sampling[4:] == want
        assert _resolved(_model(), generation_config=cfg, seed=1, min_p=0.25, typical_p=1.0).sampling[4:] == (0.25, 1.0, 1e-3, 1e-2)
        assert _resolved(_model(), generation_config=cfg, do_sample=False).sampling is None
    m = _model()
    m.load_generation_config(dict(do_sample=True, **WARP))
    assert _resolved(m, seed=1).sampling[4:] == want
    assert _resolved(m, seed=1, generation_config=dict(eta_cutoff=0.5)).sampling[4:] == (0.1, 0.9, 1e-3, 0.5)
    assert _resolved(m, seed=1, epsilon_cutoff=0).sampling[4:] == (0.1, 0.9, 0.0, 1e-2)
    with pytest.raises(ValueError, match="typical_p"):
        _model().generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, do_sample=True, typical_p=0.0)
    # what stays out of scope keeps raising as before
    for field, value in (("min_new_tokens", 3), ("num_return_sequences", 2), ("forced_eos_token_id", 2), ("sequence_bias", {(1,): -1.0})):
        with pytest.raises(NotImplementedError, match=field):
            _model().generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, do_sample=True, min_p=0.1, **{field: value})
    with pytest.raises(NotImplementedError, match="top_p"):
        _resolved(_model(), do_sample=True, top_p=0.9, top_k=0, min_p=0.1)


def test_every_entry_point_takes_the_four():
    from padt_amd import pipeline
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    for fn in (pipeline.PipelinedRunner.submit, pipeline.rec_batch):
        params = inspect.signature(fn).parameters
        for name in WARP:
            assert name in params and params[name].default is None, (fn.__qualname__, name)
    # generate takes them as keywords and hands them to generate_launch as hooks["warpers"]; processors travel next to them
    m = _model()
    seen = {}
    m.generate_launch = lambda *a, **kw: seen.update(kw) or (_ for _ in ()).throw(_Launched())
    with pytest.raises(_Launched):
        m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, do_sample=True, min_p=0.1)
    assert seen["hooks"] == dict(warpers=dict(min_p=0.1, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)) and seen["keep_scores"] is False
    with pytest.raises(_Launched):
        m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2)
    assert seen["hooks"] is None
    proc = [lambda i, s: s]
    with pytest.raises(_Launched):
        m.generate(input_ids=torch.zeros((1, 4), dtype=torch.long), max_new_tokens=2, do_sample=True, eta_cutoff=0.5, logits_processor=proc)
    assert seen["hooks"]["processors"] is proc and seen["hooks"]["warpers"]["eta_cutoff"] == 0.5 and seen["keep_scores"] is True
    with pytest.raises(ValueError, match="not a sampling warper"):
        with_warpers(hf_defaults(), dict(top_p=0.5))
    assert with_warpers(m.generation_config, dict(min_p=None)) is m.generation_config
