"""``PaDTForConditionalGeneration`` — drop-in surface of ``src/PaDT/models/padt.py`` on the MI355X HIP path.

Kept callable exactly as the reference's callers use them (eval/test_demo.py:20-113, eval/evaluation_scripts/utils.py:
194-246): ``from_pretrained``, ``generate(**processor_outputs, use_cache=True, max_new_tokens=…, do_sample=False,
output_hidden_states=True, return_dict_in_generate=True[, synced_gpus=False])`` → object with ``.sequences /
.hidden_states / .past_image_embeds / .past_logit_mask / .past_high_res_image_embeds / .past_visual_pe`` (attribute and
``['key']`` access, padt.py:786-798), ``vl_decode(feats, low, high, image_grid_thw, visual_pe)`` → dict (padt.py:397-412),
``.config.vision_config.spatial_merge_size`` and ``.model.embed_tokens.weight.shape[0]``.

There is no HuggingFace modeling code and no PyTorch compute on this path: the methods sequence kernels from
libpadt_hip.so (see vision.py / llm.py / decoder.py) and fail loudly if that library is missing.
"""
import dataclasses
import json
import os
from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from . import _lib, ops
from .config import PaDTConfig
from .decoder import PaDTDecoder
from .generation import (_GENERATE_CONFIG_NAMED, _GENERATE_CONFIG_OWN, check_beam, check_beam_compatible, check_beam_session, check_decay_length_penalty, check_forced_tokens, check_generate_kwargs,  # noqa: F401
                         check_count_penalties, check_logit_bias, check_max_tokens, check_patch_suppression, check_min_tokens, check_patch_bias, check_stop_sequences, check_token_automaton, check_top_logprobs, completion_logprobs, forced_tokens_active, generation_config_fields, resolve_options, with_warpers,
                         WARPER_NAMES)
from .llm import (LanguageModel, PromptPrefix, check_shared_destinations, plan_prefix_build, plan_prompt, plan_prompt_prefix,
                  plan_prompt_shared, unpadded_rows)
from .vision import VisionEncoder
from .weights import Fp16RangeError, load_checkpoint_state_dict, prepare_weights, synthetic_state_dict


class StepHiddenStates:
    """Lazy stand-in for HF's ``hidden_states`` (T-tuple of per-layer tuples): ``hs[step][-1]`` is the last-layer,
    post-final-norm state that predicted completion token ``step`` — (B, L, D) for step 0, (B, 1, D) afterwards
    (padt.py:732-737; consumed at padt_processor.py:125).  Only the last layer is retained."""

    class _Layers:
        def __init__(self, last):
            self._last = last

        def __getitem__(self, i):
            if i in (-1,):
                return self._last()
            raise IndexError("only the last layer ([-1]) is retained on the MI355X path")

        def __len__(self):
            return 1

    def __init__(self, hidden_buf, n_steps, prefill_packed, lens, L_pad):
        self.buf, self.n, self.prefill, self.lens, self.L = hidden_buf, n_steps, prefill_packed, lens, L_pad
        self._prefill_padded = None

    def __len__(self):
        return self.n

    def _step0(self):
        if self._prefill_padded is None:
            B, D = len(self.lens), self.prefill.shape[1]
            out = torch.zeros((B, self.L, D), device=self.prefill.device, dtype=self.prefill.dtype)
            o = 0
            for b, l in enumerate(self.lens):
                out[b, self.L - l:] = self.prefill[o:o + l]          # left padding, as the reference's callers produce
                o += l
            self._prefill_padded = out
        return self._prefill_padded

    def __getitem__(self, step):
        if isinstance(step, slice):
            return [self[i] for i in range(*step.indices(self.n))]
        if step < 0:
            step += self.n
        if not 0 <= step < self.n:
            raise IndexError(step)
        if step == 0:
            return self._Layers(self._step0)
        return self._Layers(lambda s=step: self.buf[s].unsqueeze(1))

    def last_layer_rows(self):
        """(T, B, D) tensor of the per-step last-position states (step 0 = last prompt position)."""
        return self.buf[: self.n]


class CustomGenerateDecoderOnlyOutput(dict):
    """Attribute + item access like HF's ModelOutput (padt.py:40-45)."""
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class PaDTForConditionalGeneration:
    def __init__(self, config: PaDTConfig, state_dict, device="cuda", dtype=torch.bfloat16, llm_weights: str = "bf16", operands=None,
                 state_dict_factory=None, precision: str = "default"):
        """dtype: the checkpoint's (the reference's torch_dtype argument; PaDT checkpoints are bf16).  operands: the 16-bit MFMA operand type
        ViT / LLM compute in, fp32 accumulation either way (weights.prepare_weights):
          "auto" (default; env PADT_OPERANDS) — fp16 operands (8x closer to the fp32 reference than bf16 at the same MFMA rate) UNDER A RANGE
                 GUARD: every generate() checks its ViT output rows, prototypes and the post-norm hidden rows of the prompt pass and of every
                 decode step for inf / NaN on the device (fp16 ends at 65504; an overflow of any un-normalised fp16 tensor — SwiGLU hidden,
                 q / k / v, attention output, merger hidden — arrives there, csrc/common.h rope_fin); a flagged batch is RE-RUN on the bf16
                 instantiation of the same kernels (fp32 range; built lazily from the same checkpoint, +13 GB at 3B) and a warning is logged;
          "fp16" — the same guard, but a flagged batch raises PaDTHipError (no second weight set is ever built);
          "bf16" — bf16 operands (the reference's own dtype): nothing to guard but NaN weights; a flagged batch raises.
        state_dict_factory: callable returning the checkpoint's state dict again (from_pretrained / from_synthetic pass one so that the
        fallback does not have to keep a second copy of the checkpoint alive); default: the dict given here is retained.
        precision: "default" — 16-bit MFMA operands as above (boxes within the north star's 1e-3 of the fp32 reference, mask logits at the
        3.7e-3 floor of the operand type); "reference" — ViT / LLM on the split-precision machinery of the PaDT decoder (fp32 streams,
        (hi, lo) bf16 GEMM operands at twice the MFMA work, fp32 attention and an fp32 KV cache: padt_amd/reference.py): every float output within
        1e-3 (measured 3e-6 on boxes, 5e-5 on mask logits), at a fifth of the default throughput (bench.py `reference_precision`); needs 16-bit LLM weights."""
        if dtype != torch.bfloat16:
            raise ValueError("PaDT checkpoints are bf16: pass torch_dtype=torch.bfloat16 (the MFMA operand type is chosen with operands=)")
        _lib.load()                                            # fail loudly before touching any weight
        self.config = config
        self.device = torch.device(device)
        operands = operands or os.environ.get("PADT_OPERANDS", "auto")
        if operands not in ("auto", "fp16", "bf16"):
            raise ValueError("operands must be 'auto', 'fp16' or 'bf16'")
        self.operands = operands
        self._llm_weights = llm_weights
        self._sd_factory = state_dict_factory if state_dict_factory is not None else (lambda sd=state_dict: sd) if operands == "auto" else None
        self._fallback = None                                  # the bf16-operand twin, built on the first flagged batch (operands="auto")
        self.overflow_reruns = 0                               # batches answered by the twin so far
        self._batches_seen = 0
        self.prefers_bf16 = False                              # "auto": set once most batches overflow — new decode groups then start on the twin directly
        try:
            self.W = prepare_weights(state_dict, config, self.device, llm_weights=llm_weights, operands="bf16" if operands == "bf16" else "fp16")
        except Fp16RangeError as e:                            # a weight fp16 cannot hold: "auto" multiplies bf16 operands from the start
            if operands != "auto":
                raise
            import warnings
            warnings.warn("padt_amd: %s — operands='auto' falls back to bf16 MFMA operands for this checkpoint" % e, RuntimeWarning, stacklevel=2)
            self.W = prepare_weights(state_dict, config, self.device, llm_weights=llm_weights, operands="bf16")
        self.dtype = self.W.op16                               # what pixel_values / hidden_states / past_image_embeds are held in
        self.visual = VisionEncoder(config, self.W, self.device)
        self.lm = LanguageModel(config, self.W, self.device)
        if precision not in ("default", "reference"):
            raise ValueError("precision must be 'default' or 'reference'")
        self.precision = precision
        self.ref = None
        if precision == "reference":
            if llm_weights != "bf16" or self.dtype != torch.float16:
                raise ValueError("precision='reference' needs 16-bit LLM weights and fp16 attention operands (operands='auto' or 'fp16')")
            from .reference import ReferencePath
            self.ref = ReferencePath(config, state_dict, self)
        self.vl_decoder = PaDTDecoder(config, self.W, self.device, torch.bfloat16)
        self.model = SimpleNamespace(embed_tokens=SimpleNamespace(weight=self.W["llm.embed"]))
        self.use_visual_prototype_projection = config.use_visual_prototype_projection
        self.rope_deltas = None
        # defaults HF's generate() takes from the checkpoint's generation_config.json (padt.py:436 _prepare_generation_config,
        # :570-580 logits processors / stopping criteria); from_pretrained fills it, explicit generate() kwargs override it
        self.generation_config = SimpleNamespace(repetition_penalty=1.0, eos_token_id=[config.eos_token_id],
                                                 pad_token_id=config.pad_token_id, do_sample=False, temperature=1.0,
                                                 top_k=50, top_p=1.0, no_repeat_ngram_size=0, bad_words_ids=None,
                                                 suppress_tokens=None, begin_suppress_tokens=None)          # HF GenerationConfig defaults

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=torch.bfloat16, attn_implementation=None,
                        device_map=None, config=None, llm_weights: str = "bf16", operands=None, precision: str = "default", **_):
        """Loads ``config.json`` + ``*.safetensors`` (checkpoint key layout of PaDT-MLLM/PaDT_*).  ``attn_implementation``
        is accepted and ignored: attention is always the HIP flash kernel."""
        path = str(pretrained_model_name_or_path)
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path}: checkpoints must be a local directory (no hub access on this path)")
        if config is None:
            config = PaDTConfig.from_hf_dict(json.load(open(os.path.join(path, "config.json"))))
        elif isinstance(config, dict):
            config = PaDTConfig.from_hf_dict(config)
        device = "cuda"
        if isinstance(device_map, dict) and "" in device_map:
            d = device_map[""]
            device = f"cuda:{d}" if isinstance(d, int) else str(d)
        elif isinstance(device_map, (str, torch.device)):
            device = str(device_map)
        model = cls(config, load_checkpoint_state_dict(path), device=device, dtype=torch_dtype, llm_weights=llm_weights, operands=operands,
                    state_dict_factory=lambda: load_checkpoint_state_dict(path), precision=precision)
        gpath = os.path.join(path, "generation_config.json")
        if os.path.exists(gpath):
            model.load_generation_config(json.load(open(gpath)))
        return model

    def load_generation_config(self, d: dict):
        """generation_config.json → defaults of generate(), as HF's GenerationMixin applies them (padt.py:436): repetition_penalty,
        eos_token_id (int or list), pad_token_id, do_sample / temperature / top_k / top_p, and the pure-ban processors no_repeat_ngram_size /
        bad_words_ids / suppress_tokens / begin_suppress_tokens, and the warpers after top-p: min_p / typical_p / epsilon_cutoff / eta_cutoff."""
        g = self.generation_config
        if d.get("repetition_penalty") is not None:
            g.repetition_penalty = float(d["repetition_penalty"])
        if d.get("eos_token_id") is not None:
            e = d["eos_token_id"]
            g.eos_token_id = [int(e)] if isinstance(e, int) else [int(x) for x in e]
        if d.get("pad_token_id") is not None:
            g.pad_token_id = int(d["pad_token_id"])
        for k, cast in (("do_sample", bool), ("temperature", float), ("top_k", int), ("top_p", float)):
            if d.get(k) is not None:
                setattr(g, k, cast(d[k]))
        if d.get("no_repeat_ngram_size") is not None:
            g.no_repeat_ngram_size = int(d["no_repeat_ngram_size"])
        if d.get("bad_words_ids") is not None:
            g.bad_words_ids = [[int(i) for i in wd] for wd in d["bad_words_ids"]]
        for k in ("suppress_tokens", "begin_suppress_tokens"):
            if d.get(k) is not None:
                setattr(g, k, [int(i) for i in d[k]])
        for k in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"):      # validated where they are used (generation.resolve_options)
            if d.get(k) is not None:
                setattr(g, k, float(d[k]))
        if d.get("exponential_decay_length_penalty") is not None:             # (start, factor); the range check needs the call's max_new_tokens
            g.exponential_decay_length_penalty = check_decay_length_penalty(d["exponential_decay_length_penalty"])
        return g

    @classmethod
    def from_synthetic(cls, config: PaDTConfig, seed=0, device="cuda", state_dict=None, **kw):
        """Random-init weights of the given architecture (no checkpoints offline)."""
        kw_llm, kw_op, kw_prec = kw.pop("llm_weights", "bf16"), kw.pop("operands", None), kw.pop("precision", "default")
        make = (lambda: state_dict) if state_dict is not None else (lambda: synthetic_state_dict(config, seed=seed, device=device, dtype=torch.bfloat16, **kw))
        return cls(config, make(), device=device, llm_weights=kw_llm, operands=kw_op, state_dict_factory=make, precision=kw_prec)

    def fallback_model(self):
        """The bf16-operand twin of an operands="auto" model (same checkpoint, same kernels in their bf16 instantiation: fp32 range), built on
        first use; its generation defaults follow this model's."""
        if self._fallback is None:
            if self.operands != "auto" or self._sd_factory is None:
                raise _lib.PaDTHipError("no bf16 fallback: the model was built with operands=%r" % self.operands)
            if self.precision != "default":
                raise _lib.PaDTHipError("precision='reference' has no bf16 twin: a non-finite batch is an error there")
            fb = PaDTForConditionalGeneration(self.config, self._sd_factory(), device=self.device, llm_weights=self._llm_weights, operands="bf16")
            fb.generation_config = self.generation_config
            self._fallback = fb
        return self._fallback

    def eval(self):
        return self

    # ------------------------------------------------------------------ generate (padt.py:414-616 → 618-800)
    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, pixel_values=None, image_grid_thw=None, use_cache=True,
                 max_new_tokens=None, do_sample=None, output_hidden_states=True, return_dict_in_generate=True,
                 synced_gpus=False, schedule: Optional[Sequence[Optional[str]]] = None, sync_every: int = 16,
                 use_graph: bool = True, lane: int = 0, repetition_penalty: Optional[float] = None, eos_token_id=None,
                 temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None,
                 seed: Optional[int] = None, max_length: Optional[int] = None, output_scores: bool = False, output_logits: bool = False,
                 pad_token_id: Optional[int] = None, logits_processor=None, stopping_criteria=None, no_repeat_ngram_size: Optional[int] = None,
                 bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, generation_config=None, image_index=None,
                 output_token_logprobs: bool = False, top_logprobs: Optional[int] = None, output_patch_logprobs: bool = False, **kwargs):
        """Greedy generation over the unified text‖VRT vocabulary.

        ``image_index`` (several queries on one image): a length-B sequence or int tensor; sample b uses image ``image_index[b]`` of the
        N <= B images in ``pixel_values`` / ``image_grid_thw``.  The call returns what it returns on the expanded inputs (image
        ``image_index[b]``'s patches repeated for sample b, ``image_grid_thw[image_index]``, no index) — sequences, per-sample VRT id ranges,
        hidden states, scores, ``rope_deltas``, one ``past_*`` entry per sample — but the ViT runs on the N images only and the prompt pass
        computes the rows that queries on one image have in common (everything up to the first token in which they differ: system text,
        image tokens, a repeated instruction) ONCE, fanning their K / V rows out to every member's cache.  Nothing is kept between calls.  Pass
        ``image_grid_thw[image_index]`` to ``vl_decode``.  Not available with ``precision="reference"``.

        ``prefix`` (a keyword; the handle of ``encode_prefix``) keeps that sharing ACROSS calls: ``input_ids`` / ``attention_mask`` are the full
        rows as for an ``image_index`` call, ``pixel_values`` / ``image_grid_thw`` must be ``None`` (``ValueError``), ``image_index[b]`` names the
        handle's image for row b (default ``range(B)`` when B equals the handle's image count).  Every row must start with its image's prefix
        (VRT ids compared in image-local numbering) and keep a token of its own — ``ValueError`` naming the row and the first differing
        position.  The ViT does not run, the prompt pass computes the own tokens only (llm.plan_prompt_prefix; the cached K / V rows reach
        the rows' cache images through ``padt_kv_prefix_fanout``), and the call returns what the ``image_index`` call returns; the handle is
        not modified.  ``precision="reference"`` rejects it by name; HF's ``past_key_values`` stays rejected by name.

        ``no_repeat_ngram_size`` / ``bad_words_ids`` / ``suppress_tokens`` / ``begin_suppress_tokens`` (padt.py:570-580 → HF's NoRepeatNGram /
        NoBadWords / SuppressTokens / SuppressTokensAtBegin processors): pure bans, served ON THE DEVICE in every mode — one kernel per step
        builds each row's ban bitmap from its history (the padded prompt row and the tokens so far, VRT ids included) inside the captured step,
        and the logit head writes ``-inf`` there (before the repetition penalty, which a banned logit no longer needs; before the caller's
        ``logits_processor``).  Rule ids must be text ids (< vocab_size); n-gram size and bad-word length at most 16, the packed rules at most
        4096 ints — ``NotImplementedError`` beyond.  A row whose every candidate is banned continues with the pad token.  Defaults come from the
        checkpoint's generation_config.json.
        ``generation_config``: a ``transformers.GenerationConfig`` or a dict of its fields; every field it sets goes through the policy of the
        same-named argument (so one with ``num_beams=4`` raises naming ``num_beams``), explicit arguments win over it, as in HF;
        ``use_cache`` / ``output_hidden_states`` / ``return_dict_in_generate`` follow the call's own arguments.

        ``logits_processor`` / ``stopping_criteria`` (padt.py:422-423,570-580,717,752; round 6): HF ``LogitsProcessorList`` / ``StoppingCriteriaList``
        objects or plain lists of callables ``f(input_ids, scores)``.  They run where the reference runs them — the processors on the step's fp32
        score rows AFTER the logit mask and the built-in processors (repetition penalty), before the arg-max / the sampler; the criteria on the
        sequences including the step's token, OR-ed into the stop state next to EOS and the length limit — on the HOOKED loop: decode steps launched
        kernel by kernel (no captured graph: the callables are host code), one host sync per step, ``.scores`` = the processed rows.  A row whose
        every score the processors set to ``-inf`` continues with the pad token, like a row the built-in bans emptied.  Not available
        inside ``pipeline.PipelinedRunner``'s merged decode groups.

        Arguments of the reference's ``generate`` (padt.py:414-434 + the HF generation kwargs it forwards) that this path does not
        implement are REJECTED by name (``NotImplementedError``: ``streamer``, ``prefix_allowed_tokens_fn``, ``min_length``, ``min_new_tokens``,
        ``num_beams`` > 1, video inputs, ``inputs_embeds`` …), arguments that cannot change the
        result here are accepted and ignored (``use_cache``, ``attn_implementation``, ``synced_gpus=False`` …), anything else raises the
        ``ValueError`` HF's ``_validate_model_kwargs`` raises (padt.py:440) — a caller never gets silently different behaviour.
        ``max_length`` (padt.py:511-520): total length incl. the (padded) prompt; ``max_new_tokens`` wins when both are given, as in HF.

        ``schedule`` (synthetic weights only): per-step logits-processor code — 't' text rows only, 'v' the sample's own
        VRT rows only, 'e' force EOS, None free — applied where HF's ``logits_processor`` sits (padt.py:717).
        ``lane`` selects an independent decode session (KV caches, token ring, graph) so several batches can be in
        flight on different HIP streams (pipeline.PipelinedRunner).
        ``repetition_penalty`` / ``eos_token_id`` (int or list) / ``do_sample``: default to the checkpoint's
        generation_config.json (self.generation_config), exactly the entries HF's generate turns into a logits processor /
        stopping criterion / sampling switch (padt.py:436,570-580,740-743); explicit arguments override.
        ``output_scores=True`` (padt.py:719-720): ``.scores`` = T-tuple of (B, table rows) fp32 tensors — the step's logits after the logit mask
        (padt.py:292-301) and the logits processors (repetition penalty, the synthetic ``schedule``), i.e. what the arg-max saw; under
        ``do_sample=True`` also after HF's warpers, which are part of ``logits_processor`` there (padt.py:717-720): ``logits / temperature`` on
        the tokens top-k / top-p keep, ``-inf`` on every other one.  Stopping criteria that take scores get the same rows.
        ``output_token_logprobs=True``: ``.token_logprobs`` = a (B, n_steps) fp32 tensor (n_steps = the generated columns of ``sequences``) with
        ``token_logprobs[b, t] = log_softmax(scores[t][b])[token]`` for the rows ``output_scores=True`` would return — after the logit mask, the
        ``schedule``, the repetition penalty, the four bans, the caller's ``logits_processor`` and, under ``do_sample=True``, the warpers: HF's
        ``compute_transition_scores(..., normalize_logits=True)`` — WITHOUT any logit row being written: the head reduces every 16-row block to
        (max, Σ exp) in registers and the bookkeeping kernel folds the blocks (sampling / caller processors: one extra pass over the fp32 row
        the selection kernel reads anyway).  Two deviations: steps after a row's EOS (its pad tokens) hold ``0.0``, so ``token_logprobs.sum(1)``
        is the completion's log-prob (the EOS step holds its value); a row whose every candidate is banned emits pad and holds ``-inf`` there.
        Default ``False``: the field is ``None`` and no kernel changes.
        ``top_logprobs=k`` (1 <= k <= 32; ``None`` / 0: off; negative or not an integer: ``ValueError``; above 32: ``NotImplementedError``):
        ``.top_token_ids`` (B, n_steps, k) int64 and ``.top_logprobs`` (B, n_steps, k) fp32 — entry j of step t is the column with the j-th
        largest value of the row ``output_scores=True`` would return as ``scores[t][b]`` (same processing as above, warpers included) and
        ``log_softmax(scores[t][b])`` there; descending, equal values to the lower column first (the arg-max's rule: under greedy decoding
        entry 0 is the generated token).  Ids are numbered like ``sequences`` (VRT ids >= vocab_size, within the batch).  A step with fewer
        than k finite candidates (a forced EOS, a sampler ``top_k`` below k, every column banned) fills the rest with id ``-1`` / ``-inf``;
        so do all slots of the steps after a row's EOS (the EOS step holds its values).
        ``output_patch_logprobs=True``: ``.patch_logprobs`` (B, n_steps, P) fp32, P = the largest patch count of the batch's samples:
        ``patch_logprobs[b, t, j] = log_softmax(scores[t][b])[vocab_size + vrt_off[b] + j]`` — sample b's own patch j under the full-row
        normaliser: the model's pointing belief over the image at that step; ``-inf`` for j past the sample's patch count, after the row's
        EOS, and wherever the mask, schedule, a ban or a warper removed the column.
        Both come from one selection pass over the step's fp32 row (``padt_topk_logprob_rows_f32``, inside the captured step; in plain
        greedy mode the head writes the row into the session's single row buffer) — no row is kept.  They are independent of each other, of
        ``output_token_logprobs`` and of ``output_scores``; a ``generation_config`` may carry them; off: the fields are ``None`` and no kernel changes.
        ``output_logits=True`` (padt.py:721-724, the rows BEFORE the processors and warpers): served when no processor is active
        (repetition_penalty == 1, no schedule, none of the four bans — then, under greedy decoding, they ARE the scores), rejected otherwise.  ``pad_token_id``: must be the config's (the greedy kernel pads finished
        rows with it, padt.py:749).
        ``do_sample=True``: multinomial sampling after HF's Temperature → TopK → TopP warpers (``temperature`` / ``top_k`` /
        ``top_p``, defaults from generation_config, HF's own defaults 1.0 / 50 / 1.0) on a device counter-based generator keyed
        by ``seed`` (default: drawn from torch's global generator, so torch.manual_seed makes runs repeatable).  The draws are
        not torch.multinomial's; the distribution is.
        Keywords ``min_p`` (in [0, 1]; 0: off) / ``typical_p`` (in (0, 1]; 1: off) / ``epsilon_cutoff`` / ``eta_cutoff`` (in [0, 1); 0: off): the rest of
        HF's warper list, in its order (MinP → Typical → Epsilon → Eta after top-p, ``min_tokens_to_keep = 1``, each over the softmax of
        what the stage before it kept), on the device inside the captured step (``padt_warp_sample_rows_f32``); defaults from
        generation_config / ``generation_config=``, ``ValueError`` naming the argument outside the range, ignored under greedy decoding as
        in HF.  ``.scores``, ``token_logprobs``, ``top_logprobs`` / ``patch_logprobs`` and stopping criteria see the fully warped row.  A value
        HF builds no warper for is the same call as without the argument: same kernels, same decode group.
        Keyword ``forced_tokens=F`` (a (B, n) integer tensor or a list of B id lists, n <= max_new_tokens; ids numbered like
        ``sequences[:, L:]``): the caller's completion, forced INSIDE the decode loop.  Where ``F[b, t] >= 0`` and row b is unfinished, step
        t's token IS ``F[b, t]`` whatever the scores say — appended, fed to the next step, entered into the repetition penalty's and the
        n-gram ban's history, finishing the row when it is an EOS id; a negative entry, a ragged row's missing entries and every step past n
        are free steps (the arg-max, or the draw — the generator is counter-based, so free steps draw what they would have drawn).  The scores
        are untouched: ``.scores``, ``top_token_ids`` / ``top_logprobs`` and ``patch_logprobs`` describe the step's processed row as before,
        ``token_logprobs[b, t]`` is its log-softmax AT THE FORCED TOKEN (``-inf``, never NaN, for a token the mask, a ban or the ``schedule``
        removed — it is still forced), and ``hidden_states`` hold the row that predicted each step, so ``parseVRTintoCompletion`` +
        ``vl_decode`` decode forced VRT tokens.  Forcing a run's own output reproduces it bit for bit.  ``ValueError`` naming the argument for a
        wrong batch size, n > max_new_tokens, a non-integer dtype or an id outside the table; an all-free table is the call without the
        argument.  It is NOT HF's ``forced_decoder_ids`` / ``forced_eos_token_id`` and NOT ``labels``: no prompt-pass scorer, no loss
        (``forward(is_main=True)`` keeps raising).  ``score_completions`` names the scoring use.
        Keyword ``token_automaton=A`` (a ``padt_amd.generation.TokenAutomaton``; ``None``: off, the call without the argument): which tokens
        a row may emit at a position GIVEN WHAT IT EMITTED SO FAR, decided on the device inside the captured step.  Before the head runs,
        ``padt_token_automaton`` advances every unfinished row's state by its last token and writes the step's ban bitmap — every table
        column banned except the keys of the state's edges (explicit text ids, ``A.VRT`` = the row's own patch tokens, ``A.TEXT`` = any text
        id but the EOS ids, ``A.EOS`` = the call's EOS ids); the head writes ``-inf`` at a banned column exactly as for the four bans, so
        ``.scores``, the arg-max, the sampler and its warpers, ``top_logprobs`` / ``patch_logprobs``, ``forced_tokens`` and the caller's
        ``logits_processor`` all see the constrained row, and with one of the four bans active the head reads the union of both bitmaps.
        ``token_logprobs`` under an automaton is therefore the log-softmax OVER THE ALLOWED COLUMNS: the closed-set probability of the token
        among the candidates the automaton admits.  A forced token (or a caller processor's / a ``schedule``'s) that has no edge takes its row
        off the automaton; such a row, like any row whose allowed set is empty, is allowed its EOS ids and nothing else.  It is NOT HF's
        ``prefix_allowed_tokens_fn`` (a Python callback per row and step cannot run inside a captured graph; that argument stays refused):
        the automaton is a table in device memory, so one captured graph per step mode serves every automaton, and batches share a decode
        group only when their automata are equal.  ``ValueError`` naming ``token_automaton`` for anything that is not a ``TokenAutomaton`` or
        names an id outside the text vocabulary.
        Keywords ``logit_bias`` / ``patch_bias`` / ``exponential_decay_length_penalty``: the three edits that ADD to a score, applied by the
        logit head itself where a logit becomes a score (``padt_vrt_head_bias``), so the arg-max, ``token_logprobs``, the sampler and its
        warpers, ``.scores``, ``top_logprobs`` / ``patch_logprobs``, the value a forced token is scored at and the caller's ``logits_processor``
        all see the edited row.  The order is HF's processor order (generation.score_bias_row is the specification): the bias is added to the
        masked logit FIRST (where HF's ``SequenceBiasLogitsProcessor`` sits), then the repetition penalty, then the bans, the decay last.
        ``logit_bias`` (the OpenAI / vLLM name): a dict ``{id: bias}`` or a list of ``[id, bias]`` pairs over TEXT ids, one fp32 add per
        listed column; ``-inf`` is a legal bias and a ban; NaN / ``+inf`` raise ``ValueError``, a VRT id ``NotImplementedError`` pointing to
        ``patch_bias``.  With an EOS id it is a soft length control.  It is NOT HF's ``sequence_bias`` (multi-token sequences), which stays
        refused by name like ``min_new_tokens``, ``min_length`` and ``forced_eos_token_id``.
        ``patch_bias``: a list of B entries — ``None``, a 1-D float tensor over the row's own patches in VRT-id order, or a 2-D ``(h/2, w/2)``
        map over its merged patch grid — added to the row's own patch columns: a prior over where the row points (``-inf`` outside a region of
        interest, on patches of objects already found, a saliency map of the previous frame).  ``patch_logprobs`` is then ``-inf`` outside
        the region and renormalised inside.  With ``image_index`` every query carries its own entry.  ``ValueError`` naming the argument and
        the row for a wrong length or shape, NaN or ``+inf``.
        ``exponential_decay_length_penalty=(start, factor)`` (HF's ``ExponentialDecayLengthPenalty``; defaults from ``generation_config=`` /
        generation_config.json): once more than ``start`` tokens were generated (t > start), every EOS column's score v becomes
        ``v + |v| * fp32(factor ** (t - start) - 1)``, product and sum rounded separately as HF's two tensor ops are.  ``start`` an integer >= 0,
        ``factor`` a positive real with ``factor ** max_new_tokens`` finite in fp32, else ``ValueError``.  One deviation: an EOS column that is
        already ``-inf`` (banned, masked by a ``schedule``) stays ``-inf`` where HF produces NaN.
        Bias vector and decay table live in the session's device memory: one captured graph (its own step mode) serves every value;
        batches share a decode group only when ``logit_bias`` and the decay are equal and both or neither carry a ``patch_bias``.  Without the
        three the call is what it was: same kernels, same step mode.  ``output_logits=True`` under greedy decoding is refused with any of them;
        under ``do_sample=True`` it is served as with the bans: ``.logits`` are the rows the head wrote, BEFORE the warpers but already carrying
        the bias and the decay (HF's raw logits carry no processor).  A ``generation_config=`` that sets no decay leaves the checkpoint's
        ``exponential_decay_length_penalty`` in force, as for every other named field here (HF replaces the model's config wholesale);
        pass ``exponential_decay_length_penalty=(0, 1.0)`` to switch it off.
        Keywords ``stop_sequences`` / ``min_tokens`` / ``max_tokens``: how a ROW ends, decided on the device inside the captured step
        (generation.stop_ban_ids / stop_state are the specification; ``padt_stop_ban`` in front of the head, ``padt_stop_match`` behind the
        bookkeeping kernel).  ``stop_sequences=[[id, ...], ...]``: up to 32 sequences of up to 32 TEXT ids (``NotImplementedError`` naming the
        argument and the cap beyond, and for a VRT id; ``ValueError`` for an empty list or sequence); a row is finished by the step whose
        token completes one of them within its GENERATED tokens — the prompt is never matched — and the sequence's tokens stay in the output,
        as an EOS does.  ``min_tokens=n`` (an int, or one int per row): while a row has generated fewer than n tokens every id that would end
        it (the config's EOS and the call's EOS list) scores ``-inf`` — exactly HF's ``MinNewTokensLengthLogitsProcessor(prompt_len, n,
        eos_ids)``, seen by the arg-max, the sampler and its warpers, ``.scores``, the log-prob outputs and a caller's ``logits_processor``
        — and a stop sequence that completes while the row holds fewer than n tokens is ignored, not matched retroactively later (vLLM's
        rule); a forced EOS still wins, with log-prob ``-inf``; ``n < 0`` or n above the row's budget: ``ValueError``.  ``max_tokens`` (an int,
        or one int per row, each in ``[1, max_new_tokens]``): row b is finished by its ``max_tokens[b]``-th token.  With one of the three the
        output object also has ``finish_reason`` (a list of ``"eos"`` / ``"stop"`` / ``"length"``; ``"criteria"`` for a row the caller's
        ``stopping_criteria`` ended on the hooked loop), ``stop_index`` (the matched sequence's place in the list, or -1) and ``finish_step``
        (the index of the row's last token; -1, with reason ``"length"``, for a row still running when the call reached ``max_new_tokens``), and
        ``sequences`` ends with the step in which the last row finished, whatever ``sync_every`` is.  Several conditions in one step: EOS, then
        the stop sequence of the lowest index, then the budget.  Batches share a decode group only when ``stop_sequences`` and a one-value
        ``min_tokens`` are equal and both or neither carry per-row lists (each batch writes its own rows of the session's minima and budgets);
        one captured graph serves every value; without the three the call is what it was: same kernels, same step mode, same output
        object.  They are NOT HF's ``min_new_tokens`` / ``min_length`` / ``stop_strings`` / ``max_time``, which stay refused by name.
        Keywords ``frequency_penalty`` / ``presence_penalty`` / ``patch_suppression``: the edits that GROW with what a row has already
        generated, applied by the logit head from per-row counts the captured step keeps on the device (generation.count_state /
        count_penalty_row are the specification; ``padt_count_update`` behind the bookkeeping kernel, ``padt_vrt_head_counts``).
        ``frequency_penalty=f`` / ``presence_penalty=p`` (each a float or one float per row, finite and within [-2, 2], else ``ValueError``;
        0 / ``None``: off) are the OpenAI / vLLM pair: with n the number of times the row GENERATED the column — the prompt is never counted,
        unlike the repetition penalty; forced tokens are; a row's own VRT columns count like text ids — ``s = s - f * n``, then
        ``s = s - p * (n > 0)``, vLLM's ``apply_penalties`` arithmetic in fp32.  ``patch_suppression=(radius, penalty)`` (or a list of B such
        pairs / ``None`` entries): non-maximum suppression in the pointing space — once a run of VRT tokens is COMPLETED (followed by a non-VRT
        token), every patch within ``max(|dy|, |dx|) <= radius`` of one of its tokens, on the row-major merged grid ``(h/2, w/2)`` that
        ``patch_bias`` maps use, loses ``penalty`` per such token; ``penalty=inf`` bans it.  A run still open suppresses nothing, so an object's
        own VRT tokens may sit next to each other.  ``radius``: an integer in [0, 7] (above: ``NotImplementedError``; negative or not an
        integer: ``ValueError``); ``penalty`` > 0, finite or ``+inf`` (else ``ValueError``).  Order in the head: bias, repetition penalty,
        token counts, patch neighbourhood, mask / schedule / bans, EOS decay — so the arg-max, ``token_logprobs``, a forced column's value,
        the sampler and its warpers, ``.scores``, ``top_logprobs`` / ``patch_logprobs`` and a caller's ``logits_processor`` all see the
        edited row; a row whose every candidate ends at ``-inf`` continues with the pad token.  Also read from the dict form of
        ``generation_config=``.  Works with ``precision="reference"`` (the same head).  The options carry only WHETHER each mechanism is
        on: batches with different values share a decode group (each writes its own rows), a batch with the feature and one without do
        not; one captured graph serves every value; without the three the call is what it was: same kernels, same step mode.
        Keywords ``beam_width=K`` / ``n_best=n`` / ``beam_length_penalty=1.0`` / ``beam_early_stopping=False``: beam search — the n best
        completions of every query with their sequence scores, the hypotheses kept and reordered ON THE DEVICE inside the captured step
        (generation.beam_step / beam_backtrace are the specification: HF 5.x's ``_beam_search`` rule, spelled without its ``-1e9``
        arithmetic).  The call is expanded on the host to B * K rows (each input row K times, ``image_index`` / ``prefix`` composed with the
        repeat), so the ViT runs once per image and the prompt rows once per query; a beam step then selects every row's
        ``keep = max(2, 1 + #eos) * K`` best candidates (``padt_topk_logprob_rows_f32``), ``padt_beam_step`` merges them per query — live
        beams, the finished store of K entries scored ``sum of log-probs / length ** beam_length_penalty``, HF's early-stopping heuristic
        for ``beam_early_stopping`` False / True / ``"never"`` — and ``padt_beam_reorder_kv`` makes the packed KV caches follow the beams.
        A step's score is the log-softmax of the PROCESSED row (``schedule``, ``logit_bias`` / ``patch_bias`` / the EOS decay applied first:
        the value ``token_logprobs`` defines; HF normalises before its processors).  Returned: B * n rows, row ``b * n + r`` query b's r-th
        best, shaped like a plain call on the inputs repeated n times — ``sequences`` trimmed to the longest returned hypothesis (pad behind
        a shorter one), per-row VRT ranges and ``past_*`` entries to match, so ``parseVRTintoCompletion`` + ``vl_decode`` work unchanged
        with ``image_grid_thw`` repeated — plus ``sequences_scores`` (B * n,), ``sequence_lengths`` (B * n,) and, when asked,
        ``token_logprobs``.  K: an integer in [1, 8] with keep <= 32 and B * K <= 128 rows (``NotImplementedError`` naming ``beam_width`` beyond), 1 <= n <= K,
        a finite penalty, else ``ValueError`` naming the argument; one of the other three without ``beam_width``: ``ValueError``.  Refused by
        name together with ``beam_width`` (``NotImplementedError``): ``do_sample``, ``repetition_penalty != 1``, the four bans,
        ``token_automaton``, ``forced_tokens``, ``stop_sequences`` / ``min_tokens`` / ``max_tokens``, the count penalties,
        ``top_logprobs``, ``output_patch_logprobs``, ``output_scores``, ``output_logits``, ``logits_processor`` / ``stopping_criteria``,
        ``precision="reference"`` and a model without the packed caches (head_dim != 128) — the state that depends on a row's generated
        history does not follow the beams yet.  A beam batch is always its own decode group; one captured graph per width (and candidate
        count) serves every penalty, early-stopping mode and ``max_new_tokens``.  They are NOT HF's ``num_beams`` /
        ``num_return_sequences`` / ``length_penalty`` / ``early_stopping``, which stay refused by name; without ``beam_width`` the call
        is what it was: same kernels, same step mode, same output object.
        """
        if synced_gpus:
            raise NotImplementedError("generate(synced_gpus=True) is the ZeRO-3 / FSDP lock-step loop (padt.py:445,670): every rank holds a full "
                                      "replica on this path — pass synced_gpus=False")
        # HF's warpers after top-p are keywords of this call (not named parameters: the parameter list is frozen)
        min_p, typical_p, epsilon_cutoff, eta_cutoff = (kwargs.pop(k, None) for k in WARPER_NAMES)
        forced_tokens = kwargs.pop("forced_tokens", None)             # ... and so is the table of forced completion tokens
        token_automaton = kwargs.pop("token_automaton", None)         # ... and the automaton that says which tokens may follow
        logit_bias, patch_bias = kwargs.pop("logit_bias", None), kwargs.pop("patch_bias", None)      # ... and the three additive score edits
        decay = kwargs.pop("exponential_decay_length_penalty", None)
        stop_sequences, min_tokens, max_tokens = (kwargs.pop(k, None) for k in ("stop_sequences", "min_tokens", "max_tokens"))      # ... and how a row ends
        frequency_penalty, presence_penalty, patch_suppression = (kwargs.pop(k, None) for k in ("frequency_penalty", "presence_penalty", "patch_suppression"))      # ... and the count edits
        prefix = kwargs.pop("prefix", None)                           # ... and the handle of encode_prefix
        beam = {k: kwargs.pop(k, None) for k in ("beam_width", "n_best", "beam_length_penalty", "beam_early_stopping")}      # ... and beam search
        if generation_config is not None:
            named = dict(max_new_tokens=max_new_tokens, max_length=max_length, do_sample=do_sample, repetition_penalty=repetition_penalty,
                         eos_token_id=eos_token_id, pad_token_id=pad_token_id, temperature=temperature, top_k=top_k, top_p=top_p,
                         no_repeat_ngram_size=no_repeat_ngram_size, bad_words_ids=bad_words_ids, suppress_tokens=suppress_tokens,
                         begin_suppress_tokens=begin_suppress_tokens, min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff,
                         eta_cutoff=eta_cutoff, exponential_decay_length_penalty=decay)
            for k, v in generation_config_fields(generation_config).items():
                if k in _GENERATE_CONFIG_NAMED:
                    if named[k] is None:
                        named[k] = v
                elif k == "output_scores":
                    output_scores = output_scores or bool(v)
                elif k == "output_logits":
                    output_logits = output_logits or bool(v)
                elif k == "top_logprobs":
                    top_logprobs = v if top_logprobs is None else top_logprobs
                elif k == "output_patch_logprobs":
                    output_patch_logprobs = output_patch_logprobs or bool(v)
                elif k == "frequency_penalty":
                    frequency_penalty = v if frequency_penalty is None else frequency_penalty
                elif k == "presence_penalty":
                    presence_penalty = v if presence_penalty is None else presence_penalty
                elif k == "patch_suppression":
                    patch_suppression = v if patch_suppression is None else patch_suppression
                elif k not in _GENERATE_CONFIG_OWN:
                    kwargs.setdefault(k, v)                           # the keyword policy below names what this path does not implement
            (max_new_tokens, max_length, do_sample, repetition_penalty, eos_token_id, pad_token_id, temperature, top_k, top_p, no_repeat_ngram_size,
             bad_words_ids, suppress_tokens, begin_suppress_tokens, min_p, typical_p, epsilon_cutoff, eta_cutoff, decay) = (
                named[k] for k in _GENERATE_CONFIG_NAMED)
        max_new_tokens = check_generate_kwargs(kwargs, max_new_tokens, max_length, None if input_ids is None else input_ids.shape[1])
        top_logprobs = check_top_logprobs(top_logprobs)
        if pad_token_id is not None and int(pad_token_id) != int(self.generation_config.pad_token_id):
            raise NotImplementedError(f"generate(pad_token_id={pad_token_id}): finished rows are padded with the checkpoint's pad token "
                                      f"({self.generation_config.pad_token_id}) on this path")
        processors = logits_processor if logits_processor is not None and len(logits_processor) > 0 else None
        criteria = stopping_criteria if stopping_criteria is not None and len(stopping_criteria) > 0 else None
        hooks = None
        if processors is not None or criteria is not None:
            hooks = dict(processors=processors, criteria=criteria, pass_scores=bool(output_scores))
            use_graph, sync_every = False, 1                          # host callables between the kernels of every step
        hooked = hooks is not None
        warpers = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        if any(v is not None for v in warpers.values()):
            hooks = dict(hooks or {}, warpers=warpers)                # generate_launch's channel for them (see there)
        if forced_tokens is not None:
            hooks = dict(hooks or {}, forced=forced_tokens)           # the same channel
        if token_automaton is not None:
            hooks = dict(hooks or {}, automaton=token_automaton)
        if logit_bias is not None or patch_bias is not None or decay is not None:
            hooks = dict(hooks or {}, bias=dict(logit_bias=logit_bias, patch_bias=patch_bias, decay=decay))
        if stop_sequences is not None or min_tokens is not None or max_tokens is not None:
            hooks = dict(hooks or {}, stop=dict(stop_sequences=stop_sequences, min_tokens=min_tokens, max_tokens=max_tokens))
        if frequency_penalty is not None or presence_penalty is not None or patch_suppression is not None:
            hooks = dict(hooks or {}, counts=dict(frequency_penalty=frequency_penalty, presence_penalty=presence_penalty,
                                                  patch_suppression=patch_suppression))
        if prefix is not None:
            hooks = dict(hooks or {}, prefix=prefix)
        if any(v is not None for v in beam.values()):
            check_beam(**beam)                                        # one of the other three without beam_width: ValueError
            for name, on in (("output_scores", output_scores), ("output_logits", output_logits), ("logits_processor", processors is not None),
                             ("stopping_criteria", criteria is not None)):
                if on:
                    raise NotImplementedError(f"generate(beam_width=...) with {name} is not implemented on the MI355X path: scores and host "
                                              "callbacks describe one hypothesis per row — drop the argument or run without beam_width")
            hooks = dict(hooks or {}, beam=beam)
        if output_logits:
            pen = self.generation_config.repetition_penalty if repetition_penalty is None else repetition_penalty
            if float(pen) != 1.0 or schedule is not None or processors is not None:
                raise NotImplementedError("generate(output_logits=True) with a logits processor active (repetition_penalty != 1, a schedule or a "
                                          "logits_processor): only the processed rows are kept on this path — ask for output_scores=True")
            # ... and so are the four bans under greedy decoding: generate_launch refuses there, where the defaults and the EOS filter are known
        ctx = self.generate_launch(input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens, do_sample,
                                   schedule, sync_every, use_graph, lane, repetition_penalty=repetition_penalty,
                                   eos_token_id=eos_token_id, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                   keep_scores=bool(output_scores or output_logits or hooked), hooks=hooks,
                                   keep_logits=bool(output_logits), no_repeat_ngram_size=no_repeat_ngram_size, bad_words_ids=bad_words_ids,
                                   suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, image_index=image_index,
                                   output_token_logprobs=bool(output_token_logprobs), top_logprobs=top_logprobs,
                                   output_patch_logprobs=bool(output_patch_logprobs))
        return self.generate_collect(ctx, output_hidden_states, return_dict_in_generate, output_scores=bool(output_scores),
                                     output_logits=bool(output_logits))

    @torch.no_grad()
    def generate_launch(self, input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens=1024, do_sample=None,
                        schedule=None, sync_every=16, use_graph=True, lane=0, decode_stream=None, group=None, n_slots=1,
                        repetition_penalty=None, eos_token_id=None, temperature=None, top_k=None, top_p=None, seed=None,
                        vit_stream=None, inputs_ready=None, keep_scores=False, hooks=None, keep_logits=False, no_repeat_ngram_size=None,
                        bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, image_index=None, output_token_logprobs=False,
                        top_logprobs=None, output_patch_logprobs=False):
        """Asynchronous half of generate(): host integer prep + every kernel up to the first host sync point, enqueued on
        the current stream (the decode steps on ``decode_stream`` if given, ordered after the prefill by an event).
        Returns a group context for generate_collect().

        Merged decode (pipeline.PipelinedRunner(merge=n)): ``n_slots`` batches share ONE decode session of n_slots*B
        rows — each call adds a batch (its ViT + prefill run now, its KV rows / prototypes land in the shared session),
        pass the returned context back as ``group`` for the next batch; the decode steps of all of them run together
        once the group is full (or on launch_decode()).  Every sample's math is unchanged (rows are independent in every
        decode kernel); the weights are streamed once per step for all rows.  Returns None instead of adding when the
        batch does not fit the group's session (caller closes the group and starts a new one).

        ``image_index`` (see generate()): the ViT and the prototype projection run on the N unique images and their rows are expanded per
        sample on the device; the prompt pass runs llm.plan_prompt_shared's token set.  Only THIS batch's prompt pass changes: the decode
        steps, and the rows of other batches of a merged group, are what they are without an index.

        ``hooks``: generate()'s caller processors / stopping criteria (``processors``, ``criteria``, ``pass_scores``) and / or the call's warpers
        after top-p, ``hooks=dict(warpers=dict(min_p=..., typical_p=..., epsilon_cutoff=..., eta_cutoff=...))`` (None entries: the
        generation config decides); warpers alone keep the captured step and merged groups.  ``hooks=dict(forced=F)``: generate()'s
        ``forced_tokens`` — per-batch data like the prompt; batches share a group only when both force or neither does.
        ``hooks=dict(automaton=A)``: generate()'s ``token_automaton``; batches share a group only when their automata are equal.
        ``hooks=dict(bias=dict(logit_bias=..., patch_bias=..., decay=...))``: generate()'s ``logit_bias`` / ``patch_bias`` /
        ``exponential_decay_length_penalty`` (None entries: off, the decay then follows the generation config); the patch tensors are per-batch
        data, the other two part of the options.
        ``hooks=dict(stop=dict(stop_sequences=..., min_tokens=..., max_tokens=...))``: generate()'s three arguments of that name (None
        entries: off); the sequences and a one-value ``min_tokens`` are part of the options, per-row lists are per-batch data.
        ``hooks=dict(counts=dict(frequency_penalty=..., presence_penalty=..., patch_suppression=...))``: generate()'s three arguments of that
        name (None entries: off); the values are per-batch data, the options only say which of the two mechanisms is on.
        ``hooks=dict(beam=dict(beam_width=..., n_best=..., beam_length_penalty=..., beam_early_stopping=...))``: generate()'s four
        arguments of that name; part of the options.  The batch is expanded to B * beam_width rows here and is its own decode group: with
        ``group`` given the call returns None, and the group it starts takes no second batch.
        """
        # a call's min_p / typical_p / epsilon_cutoff / eta_cutoff arrive as hooks["warpers"] (this method's parameter list is frozen) and are put
        # in front of the generation config's; what is left of `hooks` is the caller's processors / criteria, or nothing
        gen_cfg = self.generation_config
        if hooks is not None and "warpers" in hooks:
            gen_cfg = with_warpers(gen_cfg, hooks["warpers"])
            hooks = {k: v for k, v in hooks.items() if k != "warpers"} or None
        prefix = None
        if hooks is not None and "prefix" in hooks:
            prefix = hooks["prefix"]
            hooks = {k: v for k, v in hooks.items() if k != "prefix"} or None
            if prefix is not None:
                if not isinstance(prefix, PromptPrefix):
                    raise TypeError("generate(prefix=...) takes the handle encode_prefix returns (HF's past_key_values is not accepted)")
                if pixel_values is not None or image_grid_thw is not None:
                    raise ValueError("generate(prefix=...): the handle holds the images — pixel_values and image_grid_thw must be None")
                if getattr(self, "precision", "default") == "reference":
                    raise NotImplementedError("generate(prefix=...) is not implemented with precision='reference' (its prompt pass is its own: "
                                              "reference.ReferencePath.prefill): pass the images or use precision='default'")
        forced = None
        if hooks is not None and "forced" in hooks:
            if hooks["forced"] is not None:                       # shape / dtype now; the id bound once the batch's patch count is known (_launch)
                forced = check_forced_tokens(hooks["forced"], input_ids.shape[0], max_new_tokens, self.config.vocab_size)
            hooks = {k: v for k, v in hooks.items() if k != "forced"} or None
        automaton = None
        if hooks is not None and "automaton" in hooks:
            automaton = check_token_automaton(hooks["automaton"], self.config.vocab_size)
            hooks = {k: v for k, v in hooks.items() if k != "automaton"} or None
        logit_bias = patch_bias = None
        decay = getattr(gen_cfg, "exponential_decay_length_penalty", None)
        if hooks is not None and "bias" in hooks:
            hb = hooks["bias"] or {}
            logit_bias = check_logit_bias(hb.get("logit_bias"), self.config.vocab_size)
            patch_bias = check_patch_bias(hb.get("patch_bias"), input_ids.shape[0])      # lengths once the batch's patch counts are known (_launch)
            decay = hb.get("decay") if hb.get("decay") is not None else decay
            hooks = {k: v for k, v in hooks.items() if k != "bias"} or None
        stop_seqs = min_tok = max_tok = None
        if hooks is not None and "stop" in hooks:
            hs = hooks["stop"] or {}
            stop_seqs = check_stop_sequences(hs.get("stop_sequences"), self.config.vocab_size)
            max_tok = check_max_tokens(hs.get("max_tokens"), input_ids.shape[0], max_new_tokens)
            min_tok = check_min_tokens(hs.get("min_tokens"), input_ids.shape[0], max_new_tokens, max_tok)
            hooks = {k: v for k, v in hooks.items() if k != "stop"} or None
        counts = None
        if hooks is not None and "counts" in hooks:
            hc = hooks["counts"] or {}
            fpen, ppen = check_count_penalties(hc.get("frequency_penalty"), hc.get("presence_penalty"), input_ids.shape[0])
            supp = check_patch_suppression(hc.get("patch_suppression"), input_ids.shape[0])
            if fpen is not None or supp is not None:                  # all off: the call without the arguments
                counts = dict(frequency_penalty=fpen, presence_penalty=ppen, patch_suppression=supp)
            hooks = {k: v for k, v in hooks.items() if k != "counts"} or None
        beam_args = None
        if hooks is not None and "beam" in hooks:
            beam_args = hooks["beam"] or {}
            hooks = {k: v for k, v in hooks.items() if k != "beam"} or None
        decay = check_decay_length_penalty(decay, max_new_tokens)
        if decay is not None and decay[1] == 1.0:
            decay = None                                          # a[t] = 1 ** k - 1 = 0 at every step: the call without the argument
        if image_index is not None and getattr(self, "precision", "default") == "reference":
            raise NotImplementedError("generate(image_index=...) is not implemented with precision='reference' (its prompt pass is its own: "
                                      "reference.ReferencePath.prefill): expand the inputs or use precision='default'")
        # operands="auto" whose checkpoint keeps overflowing fp16: new decode groups start on the bf16 twin (a group stays with its owner).  The
        # options resolve the same on either: the twin shares this model's generation_config and config
        # ... and so do those of a call whose prefix was built there (a flagged encode_prefix): its rows are bf16 rows
        on_twin = self.prefers_bf16 or (prefix is not None and prefix.dtype == torch.bfloat16 and self.dtype == torch.float16
                                        and self.operands == "auto")
        owner = group["owner"] if group is not None else (self.fallback_model() if on_twin else self)
        opts = resolve_options(gen_cfg, self.config.eos_token_id, self.config.vocab_size, do_sample=do_sample,
                               repetition_penalty=repetition_penalty, eos_token_id=eos_token_id, temperature=temperature, top_k=top_k, top_p=top_p,
                               seed=seed, keep_scores=keep_scores, keep_logits=keep_logits, no_repeat_ngram_size=no_repeat_ngram_size,
                               bad_words_ids=bad_words_ids, suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens,
                               output_token_logprobs=output_token_logprobs, top_logprobs=top_logprobs, output_patch_logprobs=output_patch_logprobs)
        if forced_tokens_active(forced):
            opts = dataclasses.replace(opts, forced=True)
        else:
            forced = None                                         # an all-free table: the call without the argument
        if automaton is not None:
            opts = dataclasses.replace(opts, automaton=automaton.key)
        if logit_bias is not None or patch_bias is not None or decay is not None:
            opts = dataclasses.replace(opts, logit_bias=logit_bias, decay=decay, patch_bias=patch_bias is not None)
            if keep_logits and opts.sampling is None:
                raise NotImplementedError("generate(output_logits=True) with a logits processor active (logit_bias, patch_bias or "
                                          "exponential_decay_length_penalty): only the processed rows are kept on this path — ask for output_scores=True")
        stop = None
        if stop_seqs is not None or min_tok is not None or max_tok is not None:
            per_row = isinstance(min_tok, list)                   # one value for the call is part of the options; lists travel with the batch
            opts = dataclasses.replace(opts, stop_sequences=stop_seqs, min_tokens=None if per_row else min_tok,
                                       row_limits=per_row or max_tok is not None)
            stop = dict(min_tokens=min_tok if per_row else None, max_tokens=max_tok)
        if counts is not None:
            opts = dataclasses.replace(opts, count_penalties=counts["frequency_penalty"] is not None,
                                       patch_suppression=counts["patch_suppression"] is not None)
            if keep_logits and opts.sampling is None:
                raise NotImplementedError("generate(output_logits=True) with a logits processor active (frequency_penalty, presence_penalty or "
                                          "patch_suppression): only the processed rows are kept on this path — ask for output_scores=True")
        beam_orig = None
        beam = check_beam(n_eos=len(set(opts.eos_ids)), **beam_args) if beam_args is not None else None
        if beam is not None:
            # what depends on a row's generated history does not follow the beams (yet): refused by name, before anything is launched
            check_beam_compatible(opts, processors=bool(hooks and hooks.get("processors")), criteria=bool(hooks and hooks.get("criteria")),
                                  reference=getattr(self, "precision", "default") == "reference")
            check_beam_session(self.config, input_ids.shape[0], beam[0])      # the packed caches; B * K rows within what a session takes
            if group is not None:
                return None                                       # a beam batch is always its own decode group
            opts = dataclasses.replace(opts, beam=beam)
            # the call expanded to B * K rows: every input row K times in place, image_index / prefix composed with the repeat — the existing
            # sharing then runs the ViT once per image and the common prompt rows once (llm.plan_prompt_shared / plan_prompt_prefix)
            K, B0 = beam[0], input_ids.shape[0]
            beam_orig = dict(input_ids=input_ids, attention_mask=attention_mask, image_index=image_index, patch_bias=patch_bias)
            if image_index is None and (prefix is None or len(prefix.ids) == B0):
                image_index = list(range(B0))
            if image_index is not None:
                image_index = [int(i) for i in image_index for _ in range(K)]
            input_ids = input_ids.repeat_interleave(K, dim=0)
            V = self.config.vocab_size
            if bool((input_ids >= V).any()):
                # VRT ids of the prompt rows are numbered within the caller's batch; every expanded row owns a range of its own
                g = (prefix.grid if prefix is not None else image_grid_thw).detach().cpu().long().tolist()
                idx0 = list(range(B0)) if beam_orig["image_index"] is None else [int(i) for i in beam_orig["image_index"]]
                n_m = [g[u][0] * g[u][1] * g[u][2] // self.config.merge_unit for u in idx0]
                shift = [sum(n_m[:b]) * (K - 1) + c * n_m[b] for b in range(B0) for c in range(K)]      # the row's new offset minus its old one
                shift = torch.tensor(shift, dtype=input_ids.dtype, device=input_ids.device)[:, None]
                input_ids = torch.where(input_ids >= V, input_ids + shift, input_ids)
            attention_mask = None if attention_mask is None else attention_mask.repeat_interleave(K, dim=0)
            patch_bias = None if patch_bias is None else [pb for pb in patch_bias for _ in range(K)]
            n_slots = 1
        return owner._launch(opts, input_ids, attention_mask, pixel_values, image_grid_thw, image_index, max_new_tokens=max_new_tokens,
                             schedule=schedule, hooks=hooks, sync_every=sync_every, use_graph=use_graph, lane=lane, decode_stream=decode_stream,
                             group=group, n_slots=n_slots, vit_stream=vit_stream, inputs_ready=inputs_ready, forced=forced, automaton=automaton,
                             patch_bias=patch_bias, stop=stop, counts=counts, prefix=prefix, beam_orig=beam_orig)

    def _launch(self, opts, input_ids, attention_mask, pixel_values, image_grid_thw, image_index, *, max_new_tokens, schedule, hooks, sync_every,
                use_graph, lane, decode_stream, group, n_slots, vit_stream, inputs_ready, forced=None, automaton=None, patch_bias=None, stop=None,
                counts=None, prefix=None, beam_orig=None):
        """generate_launch on the group's owner, with the call's options resolved (generation.GenOptions).  beam_orig: a beam call's inputs
        before their expansion to B * K rows (what a re-run on the bf16 twin is given)."""
        self._batches_seen += 1
        if prefix is None and (pixel_values is None or image_grid_thw is None):
            raise ValueError("pixel_values and image_grid_thw are required (text-only input crashes in the reference too, "
                             "padt.py:292 with image_prototypes unbound)")
        cfg, dev = self.config, self.device
        handle = None if prefix is None else self._prefix_for(prefix)       # the build in this model's operand type
        grid = image_grid_thw.detach().cpu().long() if prefix is None else handle.grid
        B = input_ids.shape[0]
        T_max = int(max_new_tokens)
        k = 0 if group is None else len(group["subs"])
        row0 = k * B
        proto_row0 = 0 if group is None else group["proto_rows"]
        if prefix is not None:
            plan = plan_prompt_prefix(cfg, input_ids, attention_mask, handle, image_index, dev, row0=row0, proto_row0=proto_row0)
        elif image_index is None:
            plan = plan_prompt(cfg, input_ids, attention_mask, grid, dev, row0=row0, proto_row0=proto_row0)
        else:
            plan = plan_prompt_shared(cfg, input_ids, attention_mask, grid, image_index, dev, row0=row0, proto_row0=proto_row0)
        sh = plan.shared
        n_proto = plan.vrt_off[-1]
        p_max = max(plan.vrt_off[i + 1] - plan.vrt_off[i] for i in range(B))      # output_patch_logprobs: the widest sample of this batch
        need_s = max(plan.lens) + T_max
        if forced is not None:                                    # ids are the batch's own numbering: text ids and its n_proto patch rows
            forced = check_forced_tokens(forced, B, T_max, cfg.vocab_size, [n_proto] * B)
        if patch_bias is not None:                                # lengths and map shapes against the rows' own patch grids
            ms = cfg.vision_config.spatial_merge_size
            gi = grid if image_index is None else grid[torch.as_tensor([int(i) for i in image_index], dtype=torch.long)]
            patch_bias = check_patch_bias(patch_bias, B, [plan.vrt_off[i + 1] - plan.vrt_off[i] for i in range(B)],
                                          [(int(g[1]) // ms, int(g[2]) // ms) for g in gi])
        count_grids = None
        if opts.counts:                                           # each row's merged patch grid against its patch count, before any device state is touched:
            cv = counts or {}                                     # padt_count_update indexes the row's patches with it
            ms = cfg.vision_config.spatial_merge_size
            gi = grid if image_index is None else grid[torch.as_tensor([int(i) for i in image_index], dtype=torch.long)]
            count_grids = [(int(g[1]) // ms, int(g[2]) // ms) for g in gi]
            supp = cv.get("patch_suppression") or [None] * B
            for b, (hp_, wp_) in enumerate(count_grids):
                if hp_ * wp_ != plan.vrt_off[b + 1] - plan.vrt_off[b]:
                    if supp[b] is not None:
                        raise ValueError(f"generate(patch_suppression=...): row {b}: a merged patch grid of {hp_} x {wp_} for "
                                         f"{plan.vrt_off[b + 1] - plan.vrt_off[b]} patches")
                    count_grids[b] = (0, 0)                       # never read: the row's radius is -1
        if opts.rules is not None:
            need_s = max(need_s, plan.L_pad)                      # the session's history rows hold the padded prompt row
        if hooks is not None and (group is not None or n_slots != 1):
            raise NotImplementedError("logits_processor / stopping_criteria run on generate()'s own (un-merged) decode loop, not inside a merged decode group")
        if group is None:
            sess = self.lm.session(B * n_slots, need_s, n_proto * n_slots, T_max, lane=lane)
            group = dict(sess=sess, subs=[], proto_rows=0, B=B, n_slots=n_slots, T_max=T_max, sync_every=sync_every,
                         use_graph=use_graph, decode_stream=decode_stream, done=0, launched=False, schedule=schedule,
                         opts=opts, lane=lane, owner=self)
            # every row neutral and the options' buffers reset; the batches write their own rows (add_batch below).  Reference precision:
            # eager split-precision steps and fp32 hidden rows
            sess.begin(opts, p_max, processors=bool(hooks and hooks["processors"]), step_fn=self.ref.step if self.ref is not None else None,
                       automaton=automaton, n_steps=T_max, schedule=schedule)
            if hooks is not None:
                ids_dev = input_ids.detach().to(dev).long().contiguous()
                hk = dict(hooks, B=B, table_rows=cfg.vocab_size + n_proto, t=0)
                # `input_ids` as the reference's loop holds them (padt.py:751): the prompt and the tokens selected so far
                hk["sequences"] = lambda hk=hk, s=sess: ops.assemble_sequences(ids_dev, s.tokens[:B], hk["t"], cfg.vocab_size, 0)
                sess.hooks = hk
                group["hooks"] = hooks
        else:
            sess = group["sess"]
            if (group["launched"] or k >= group["n_slots"] or B != group["B"] or T_max != group["T_max"]
                    or schedule != group["schedule"] or opts != group["opts"] or sess.s_max < need_s
                    or sess.np_max < proto_row0 + n_proto or (opts.patch_logprobs and sess.p_cap < p_max)):
                return None
        if sh is not None:
            check_shared_destinations(sh, sess.B, sess.s_max)
        rows = slice(row0, row0 + B)
        sess.nf[rows].zero_()
        # this batch's range guard (ViT rows, prototypes, prompt-pass hidden rows).  Its zero fill must be ordered before EVERY check that ORs
        # into it: with a ViT stream the flag is zeroed ON that stream (the fill on the current stream would sit behind the
        # previous batch's prefill while the ViT checks of this batch already run — ADVICE r05); the prefill's check comes after
        # cur.wait_stream(vit_stream) below
        # The flag is slot k of the session's per-batch vector (read back with every other flag by ONE ops.collect_summary launch).
        nf = sess.nf_batch[k: k + 1]
        if vit_stream is None or self.ref is not None or prefix is not None:
            nf.zero_()

        # ---- ViT → prototypes → session table
        if prefix is not None:
            # no ViT: every per-sample output is a device row copy of the handle's rows, on the current stream (they were checked when built)
            if handle.ready is not None:
                torch.cuda.current_stream().wait_event(handle.ready)
            low, high = ops.gather_rows(handle.low, sh.low_rows), ops.gather_rows(handle.high, sh.patch_rows)
            pe = (ops.gather_rows(handle.pe[0], sh.patch_rows), ops.gather_rows(handle.pe[1], sh.patch_rows))
            proto = ops.gather_rows(handle.proto, sh.low_rows, out=sess.proto[proto_row0: proto_row0 + n_proto])
        elif self.ref is not None:
            low, high, pe = self.ref.visual(pixel_values.to(dev), grid, nf=nf)
            proto = self.ref.prototypes(low, sess, proto_row0, nf=nf)     # fp32 rows (→ past_image_embeds); sess.proto gets their fp16 image
        elif vit_stream is None:
            low, high, pe, proto = self._vit_and_prototypes(pixel_values, grid, sess.proto[proto_row0: proto_row0 + n_proto], nf, sh)
        else:
            # the ViT of this batch on its own stream: it needs the inputs (event `inputs_ready` of the caller's stream) and nothing of the
            # current stream — so it runs while the PREVIOUS batch's prefill is still on the current stream — except for the first batch of a
            # group, whose session may just have been (re)allocated or reset on the current stream
            cur = torch.cuda.current_stream()
            if inputs_ready is not None:
                vit_stream.wait_event(inputs_ready)
            if k == 0 or inputs_ready is None:
                vit_stream.wait_stream(cur)
            with torch.cuda.stream(vit_stream):
                nf.zero_()
                low, high, pe, proto = self._vit_and_prototypes(pixel_values, grid, sess.proto[proto_row0: proto_row0 + n_proto], nf, sh)
            cur.wait_stream(vit_stream)                           # the prefill below reads low / the prototype rows
            for t_ in (low, high, pe[0], pe[1]):                   # allocated on vit_stream, read on the prefill / decode streams
                t_.record_stream(cur)
                if decode_stream is not None:
                    t_.record_stream(decode_stream)
        # ---- per-generate device state of this batch's rows (the session writes its own buffers: DecodeSession.add_batch)
        sess.add_batch(opts, row0, proto_row0, plan.vrt_off, plan.lens, plan.next_pos,
                       prompt_ids=input_ids.detach().to(dev).long() if opts.reads_prompt else None, forced=forced, stop=stop, counts=counts,
                       count_grids=count_grids, patch_bias=patch_bias)
        self.rope_deltas = plan.rope_deltas

        # ---- prefill; the first token is selected together with the other batches of the group (launch_decode)
        if self.ref is not None:
            hn_all = self.ref.prefill(plan, low, sess, nf=nf)             # fp32 rows
            ops.gather_rows(hn_all, plan.last_idx, out=sess.hid32[0, rows])
            ops.cast_f32_x16(sess.hid32[0, rows], out=sess.hn_first[rows])
        else:
            hn_all = self.lm.prefill(plan, low, sess, nf=nf)
            ops.gather_rows(hn_all, plan.last_idx, out=sess.hn_first[rows])
        group["subs"].append(dict(plan=plan, low=low, high=high, pe=pe, proto=proto, hn_all=hn_all, input_ids=input_ids,
                                  n_proto=n_proto, row0=row0, proto_row0=proto_row0, nf=nf, p_max=p_max, forced=forced, automaton=automaton,
                                  patch_bias=patch_bias, stop=stop, counts=counts, prefix=prefix, beam_orig=beam_orig,
                                  row_grids=(grid if image_index is None else grid[torch.as_tensor([int(i) for i in image_index], dtype=torch.long)]).tolist(),
                                  inputs=(attention_mask, pixel_values, image_grid_thw, image_index)))       # what a re-run on the bf16 twin needs
        group["proto_rows"] = proto_row0 + n_proto
        if len(group["subs"]) == group["n_slots"]:
            self.launch_decode(group)
        return group

    # ------------------------------------------------------------------ prompt prefixes kept across calls
    @torch.no_grad()
    def encode_prefix(self, input_ids, attention_mask, pixel_values, image_grid_thw) -> PromptPrefix:
        """ViT pass and prompt pass of N images and the prompt rows in front of every query on them, kept for later calls:
        ``generate(prefix=handle, image_index=[...])`` then computes each row's own tokens only.  Row u is the prompt up to wherever sharing
        is to end; it must contain image u's image tokens completely (``ValueError``).  The handle (llm.PromptPrefix) owns what it holds —
        merged / patch-level / PE / prototype rows, the prefix's last-layer hidden rows and, per LLM layer, its roped K rows and V rows in
        this model's 16-bit operand type: 2 * layers * Hkv * head_dim * 2 bytes per prefix token (``handle.nbytes``) — and keeps the inputs
        it was built from.  operands="auto": a build whose range guard fires is answered by the bf16 twin's (counted in
        ``overflow_reruns``); calls with such a handle run on the twin.  Synchronises once (the guard's flag)."""
        if getattr(self, "precision", "default") == "reference":
            raise NotImplementedError("encode_prefix / generate(prefix=...) is not implemented with precision='reference' (its prompt pass is "
                                      "its own: reference.ReferencePath.prefill)")
        owner = self.fallback_model() if self.prefers_bf16 else self
        h = owner._build_prefix(input_ids, attention_mask, pixel_values, image_grid_thw)
        if h is None:
            what = ("a non-finite value reached the ViT output / prototypes / post-norm hidden rows of a prompt prefix (%s MFMA operands)"
                    % ("fp16" if owner.dtype == torch.float16 else "bf16"))
            if owner is not self or self.operands != "auto" or self.dtype != torch.float16:
                raise _lib.PaDTHipError(what)
            import warnings
            self.overflow_reruns += 1
            warnings.warn("padt_amd: " + what + " — fp16 range exceeded; the prefix is built on the bf16-operand instantiation "
                          "(%d so far)" % self.overflow_reruns, RuntimeWarning, stacklevel=2)
            h = self.fallback_model()._build_prefix(input_ids, attention_mask, pixel_values, image_grid_thw)
            if h is None:
                raise _lib.PaDTHipError(what.replace("fp16", "bf16"))
        return h

    def _build_prefix(self, input_ids, attention_mask, pixel_values, image_grid_thw) -> Optional[PromptPrefix]:
        """encode_prefix in THIS model's operand type: → the handle, or None when the range guard fired.  The kernels are generate()'s at the
        same row counts — ViT, prototype projection, the prompt pass over the N rows — with one difference: the post-pass's only
        destinations are the handle's own layer slices (llm.plan_prefix_build), so no session is involved."""
        cfg, dev = self.config, self.device
        grid = image_grid_thw.detach().cpu().long()
        plan = plan_prefix_build(cfg, input_ids, attention_mask, grid, dev)
        rows = unpadded_rows(input_ids, attention_mask)
        V, cu = cfg.vocab_size, plan.cu.tolist()
        ids = [[t - plan.vrt_off[u] if t >= V else t for t in r] for u, r in enumerate(rows)]
        nf = torch.zeros(1, device=dev, dtype=torch.int32)
        low, high, pe = self.visual(pixel_values.to(dev), grid, nf=nf)
        proto = self.lm.prototypes(low, nf=nf)
        nl, kv, hd = cfg.num_hidden_layers, cfg.num_key_value_heads * cfg.head_dim, cfg.head_dim
        T = cu[-1]
        K, Vr = (torch.empty((nl, T, kv), device=dev, dtype=self.dtype) for _ in range(2))
        # what the prompt pass reads of a session: the prototype table, the id-range flag, the rope frequencies; the cache images are
        # never written (every destination is a join row), one small block stands in for all of them
        dummy = torch.zeros((1, cfg.num_key_value_heads, 64, hd), device=dev, dtype=self.dtype)
        stub = SimpleNamespace(proto=proto, err=torch.zeros(1, device=dev, dtype=torch.int32), s_max=64, cache_packed=False,
                               inv_freq=(1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))).to(dev),
                               kc=[dummy] * nl, vtc=[dummy.view(1, cfg.num_key_value_heads, hd, 64)] * nl)
        hidden = self.lm.prefill(plan, low, stub, nf=nf, kv_out=(K, Vr))
        flags = torch.cat([stub.err, nf]).cpu().tolist()
        if flags[0] != 0:
            raise AssertionError("input_ids.max() >= extended table rows (padt.py:203)")
        if flags[1] != 0:
            return None
        pos3 = plan.pos3.cpu()
        keep = lambda t: t.detach().clone() if isinstance(t, torch.Tensor) else t
        return PromptPrefix(ids=ids, grid=grid, pos3=[pos3[:, cu[u]: cu[u + 1]].clone() for u in range(len(rows))], next_pos=list(plan.next_pos),
                            dtype=self.dtype, low=low, high=high, pe=pe, proto=proto, hidden=hidden, k=K, v=Vr,
                            pre_off=torch.tensor(cu, dtype=torch.int32, device=dev), ready=torch.cuda.current_stream().record_event(),
                            inputs=tuple(keep(t) for t in (input_ids, attention_mask, pixel_values, image_grid_thw)))

    def _prefix_for(self, prefix: PromptPrefix) -> PromptPrefix:
        """The build of the caller's handle in this model's operand type: the handle itself, or — the bf16 twin answering for an fp16
        handle — its bf16 build, made once from the inputs the handle kept."""
        if prefix.dtype == self.dtype:
            return prefix
        if prefix.dtype == torch.float16 and self.dtype == torch.bfloat16:
            if prefix.twin is None:
                prefix.twin = self._build_prefix(*prefix.inputs)
                if prefix.twin is None:
                    raise _lib.PaDTHipError("a non-finite value reached the rows of a prompt prefix (bf16 MFMA operands): NaN / inf weights or inputs?")
            return prefix.twin
        raise ValueError(f"generate(prefix=...): the prefix was built with {prefix.dtype} operands, this model multiplies {self.dtype} — "
                         "build it with this model's encode_prefix")

    def _vit_and_prototypes(self, pixel_values, grid, proto_out, nf, sh):
        """ViT → prototypes into the session's table rows ``proto_out``, on the current stream: → (low, high, pe, proto).  With a shared plan
        (generate(image_index=)) the ViT blocks run on the N unique images and every output comes back per sample (VisionEncoder's
        ``expand``: device row copies of the patch-level rows, merger and prototype projection at the expanded row count)."""
        expand = None if sh is None else (sh.low_rows, sh.patch_rows, sh.grid_x)
        low, high, pe = self.visual(pixel_values.to(self.device), grid, nf=nf, expand=expand)
        return low, high, pe, self.lm.prototypes(low, out=proto_out, nf=nf)

    @torch.no_grad()
    def launch_decode(self, group):
        """First-token selection + the first chunk of decode steps (hipGraph replays, no host sync) for every batch of the
        group; ordered after their prefills (current stream) by an event when a decode stream is used."""
        if group["owner"] is not self:
            return group["owner"].launch_decode(group)
        if group["launched"]:
            return
        group["launched"] = True
        sess, T_max = group["sess"], group["T_max"]
        n = min(group["sync_every"], T_max - 1)
        if sess.hooks is not None:
            n = 0                                                    # hooked loop: the stop state is read after EVERY token, the first included (padt.py:752-757)

        def go():
            sess.head_and_select(sess.hn_first, advance=False)
            sess.run_steps(n, use_graph=group["use_graph"])
        ds = group["decode_stream"]
        if ds is not None:
            ev = torch.cuda.current_stream().record_event()
            with torch.cuda.stream(ds):
                ds.wait_event(ev)
                go()
        else:
            go()
        group["done"] = 1 + n

    @torch.no_grad()
    def generate_collect(self, group, output_hidden_states=True, return_dict_in_generate=True, all_batches=False, output_scores=False,
                         output_logits=False):
        """Synchronising half of generate(): remaining decode chunks, trimming to the reference's stop rule, output object — of the group's only
        batch, or a list over its batches.  Everything the host needs from the device per chunk — the table-range assert (padt.py:203), `any
        row unfinished`, the range guard's per-row / per-batch flags, each row's first EOS step — comes from ONE kernel + ONE pinned D2H copy
        (DecodeSession.read_summary over ops.collect_summary; round 6: no ATen reductions, no `.item()` round trips)."""
        if group["owner"] is not self:
            return group["owner"].generate_collect(group, output_hidden_states, return_dict_in_generate, all_batches, output_scores, output_logits)
        cfg, dev = self.config, self.device
        self.launch_decode(group)
        sess, T_max, opts = group["sess"], group["T_max"], group["opts"]
        n_sub = len(group["subs"])
        done_steps = group["done"]
        rec = sess.read_summary(done_steps, n_sub)
        while done_steps < T_max and rec["unfinished"]:
            n = min(group["sync_every"], T_max - done_steps)
            sess.run_steps(n, use_graph=group["use_graph"])
            done_steps += n
            rec = sess.read_summary(done_steps, n_sub)
        group["done"] = done_steps
        if rec["err"] != 0:
            raise AssertionError("input_ids.max() >= extended table rows (padt.py:203)")
        nf_rows, nf_batch, first_eos = rec["nf_rows"], rec["nf_batch"], rec["first_eos"]
        if opts.stop:                                             # a row's end is what padt_stop_match (or the hooked loop) recorded, whatever ended it
            fin_step, fin_reason, fin_index = rec["finish_step"], rec["finish_reason"], rec["stop_index"]
        outs = []
        for k_sub, sub in enumerate(group["subs"]):
            plan, row0, B = sub["plan"], sub["row0"], group["B"]
            if nf_batch[k_sub] != 0 or any(nf_rows[row0: row0 + B]):
                outs.append(self._non_finite_batch(group, sub, output_hidden_states, return_dict_in_generate, output_scores, output_logits))
                continue
            if opts.beam is not None:
                outs.append(self._collect_beams(group, sub, output_hidden_states, return_dict_in_generate))
                continue
            # the reference stops right after the step in which the last sequence finished (padt.py:756-757); any id of the EOS list finishes a row
            fe = fin_step[row0: row0 + B] if opts.stop else first_eos[row0: row0 + B]
            n_steps = max(fe) + 1 if all(f >= 0 for f in fe) else done_steps
            # [input_ids | tokens] with the group's session-global VRT ids shifted back to this batch's own (one launch, padt.py:751)
            sequences = ops.assemble_sequences(sub["input_ids"].to(dev), sess.tokens[row0: row0 + B], n_steps, cfg.vocab_size, sub["proto_row0"])
            # clone: the session's hidden_buf is reused by the lane's next generate(); the caller owns what it gets back
            hbuf = sess.hid32 if self.ref is not None else sess.hidden_buf      # reference precision keeps the per-step rows in fp32
            hidden = StepHiddenStates(hbuf[:n_steps, row0: row0 + B].clone(), n_steps, sub["hn_all"],
                                      plan.lens, plan.L_pad)
            table_rows = cfg.vocab_size + sub["n_proto"]
            def per_step(stash):
                # per step (B, table rows): text columns + this batch's own prototype columns of the session-wide rows (padt.py:719-724)
                V, p0 = cfg.vocab_size, sub["proto_row0"]
                rows_t = stash[:n_steps, row0: row0 + B]
                if p0 == 0:
                    return tuple(rows_t[t, :, :table_rows].clone() for t in range(n_steps))
                return tuple(torch.cat([rows_t[t, :, :V], rows_t[t, :, V + p0: V + p0 + sub["n_proto"]]], dim=1) for t in range(n_steps))
            scores = per_step(sess.scores) if output_scores or output_logits else None
            logits = (per_step(sess.raw_scores) if opts.keep_logits else scores) if output_logits else None
            top_ids = top_lp = patch_lp = None
            if opts.top_logprobs:                                 # session columns → this batch's own VRT numbering, as assemble_sequences does
                top_ids = sess.top_idx[row0: row0 + B, :n_steps].to(torch.int64)
                if sub["proto_row0"]:
                    top_ids = torch.where(top_ids >= cfg.vocab_size, top_ids - sub["proto_row0"], top_ids)
                top_lp = sess.top_val[row0: row0 + B, :n_steps].clone()
            if opts.patch_logprobs:
                patch_lp = sess.patch_lp[row0: row0 + B, :n_steps, :sub["p_max"]].clone()
            out = CustomGenerateDecoderOnlyOutput(
                sequences=sequences, scores=scores if output_scores else None, logits=logits, attentions=None,
                hidden_states=hidden if output_hidden_states else None, past_key_values=sess,
                token_logprobs=sess.logprobs[row0: row0 + B, :n_steps].clone() if opts.token_logprobs else None,
                top_token_ids=top_ids, top_logprobs=top_lp, patch_logprobs=patch_lp,
                past_image_embeds=sub["proto"].clone(),
                past_logit_mask=ops.logit_mask(sess.vrt_off[row0: row0 + B + 1], cfg.vocab_size, table_rows, sub["proto_row0"], B),
                past_high_res_image_embeds=sub["high"], past_visual_pe=sub["pe"])
            if opts.stop:                                         # a row still running at the call's end: -1, "length"
                out["finish_step"] = [int(f) for f in fe]
                out["finish_reason"] = [ops.STOP_REASONS[r] if f >= 0 and 0 < r < len(ops.STOP_REASONS) else "length"
                                        for f, r in zip(fe, fin_reason[row0: row0 + B])]
                out["stop_index"] = [int(i) if f >= 0 else -1 for f, i in zip(fe, fin_index[row0: row0 + B])]
            outs.append(out if return_dict_in_generate else sequences)
        return outs if all_batches else outs[0]

    def _collect_beams(self, group, sub, output_hidden_states, return_dict_in_generate):
        """The output object of a beam batch: B * n_best rows, row b * n_best + r query b's r-th best hypothesis, shaped like a plain call on
        the inputs repeated n_best times.  padt_beam_finalize walks the parents back on the device (tokens, log-probs, scores, lengths, the
        hidden rows gathered into StepHiddenStates' layout); the host selects the first n_best of every query's K identical prompt rows."""
        cfg, dev, sess, plan = self.config, self.device, group["sess"], sub["plan"]
        K, n_best = group["opts"].beam[0], group["opts"].beam[1]
        B, V = group["B"] // K, cfg.vocab_size
        sel = [b * K + r for b in range(B) for r in range(n_best)]                  # the expanded rows that stand for the returned ones
        n_patch = [plan.vrt_off[i + 1] - plan.vrt_off[i] for i in sel]
        off = [0]
        for n in n_patch:
            off.append(off[-1] + n)
        off_dev = torch.tensor(off, dtype=torch.int32).to(dev)
        fin = ops.beam_finalize(sess.beam, n_best, sess.hidden_buf, off_dev, cfg.pad_token_id, V)
        lengths = fin["lengths"].cpu().tolist()
        n_steps = max(lengths)
        sel_dev = torch.tensor(sel, dtype=torch.long, device=dev)
        sequences = ops.assemble_sequences(sub["input_ids"].to(dev)[sel_dev].contiguous(), fin["tokens"], n_steps, V, 0)
        # the selected rows of everything that is packed per expanded row: prompt hidden rows, prototypes, patch-level rows
        ranges = lambda offs: torch.cat([torch.arange(offs[i], offs[i + 1], dtype=torch.long) for i in sel]).to(dev)
        cu, patch_off = [0], [0]
        for l, g in zip(plan.lens, sub["row_grids"]):
            cu.append(cu[-1] + l)
            patch_off.append(patch_off[-1] + int(g[0]) * int(g[1]) * int(g[2]))
        hidden = StepHiddenStates(fin["hidden"][:n_steps], n_steps, sub["hn_all"][ranges(cu)], [plan.lens[i] for i in sel], plan.L_pad)
        prows = ranges(patch_off)
        out = CustomGenerateDecoderOnlyOutput(
            sequences=sequences, scores=None, logits=None, attentions=None, hidden_states=hidden if output_hidden_states else None,
            past_key_values=sess, token_logprobs=fin["logprobs"][:, :n_steps].clone() if group["opts"].token_logprobs else None,
            top_token_ids=None, top_logprobs=None, patch_logprobs=None, past_image_embeds=sub["proto"][ranges(plan.vrt_off)],
            past_logit_mask=ops.logit_mask(off_dev, V, V + off[-1], 0, len(sel)), past_high_res_image_embeds=sub["high"][prows],
            past_visual_pe=tuple(t[prows] for t in sub["pe"]), sequences_scores=fin["scores"],
            sequence_lengths=fin["lengths"].to(torch.int64))
        return out if return_dict_in_generate else sequences

    def _non_finite_batch(self, group, sub, output_hidden_states, return_dict_in_generate, output_scores, output_logits):
        """A batch whose range guard fired: inf / NaN reached its ViT output, prototypes or hidden rows.  With fp16 operands that is an
        overflow of an un-normalised 16-bit tensor (65504); operands="auto" answers it with the SAME batch on the bf16 instantiation."""
        what = ("a non-finite value reached the ViT output / prototypes / post-norm hidden rows of a batch (%s MFMA operands)"
                % ("fp16" if self.dtype == torch.float16 else "bf16"))
        if self.operands != "auto" or self.dtype != torch.float16:
            raise _lib.PaDTHipError(what + (": an un-normalised activation exceeded fp16's 65504 — build the model with operands='auto' (re-runs such "
                                            "batches on bf16 operands) or operands='bf16'" if self.dtype == torch.float16 else
                                            ": NaN / inf weights or inputs?"))
        import warnings
        fb = self.fallback_model()
        self.overflow_reruns += 1
        warnings.warn("padt_amd: " + what + " — fp16 range exceeded; the batch is re-run on the bf16-operand instantiation "
                      "(%d so far; operands='bf16' avoids the second pass)" % self.overflow_reruns, RuntimeWarning, stacklevel=3)
        if not self.prefers_bf16 and self.overflow_reruns >= 3 and 2 * self.overflow_reruns >= self._batches_seen:
            # this checkpoint's activations do not fit fp16 as a rule, not as an exception: stop paying for two passes
            self.prefers_bf16 = True
            warnings.warn("padt_amd: %d of %d batches exceeded fp16's range — operands='auto' now starts every new decode group on the bf16 "
                          "instantiation" % (self.overflow_reruns, self._batches_seen), RuntimeWarning, stacklevel=3)
        am, pix, grid, image_index = sub["inputs"]
        # the group's options spelled as explicit arguments (an "off" is 0 / [], never the default), and what this collect was asked to return
        kw = dict(group["opts"].generate_kwargs(), **group["opts"].warper_kwargs(), **group["opts"].bias_kwargs(), **group["opts"].stop_kwargs(),
                  **group["opts"].beam_kwargs(), output_scores=output_scores, output_logits=output_logits)
        if sub.get("stop") is not None:                           # the batch's own per-row lists: the options only say that there are some
            kw.update({k: v for k, v in sub["stop"].items() if v is not None})
        if sub.get("counts") is not None:                         # the batch's own per-row values: the options only say which mechanism is on
            kw.update(sub["counts"])
        if group.get("hooks") is not None:
            kw.update(logits_processor=group["hooks"]["processors"], stopping_criteria=group["hooks"]["criteria"])
        if sub.get("forced") is not None:
            kw.update(forced_tokens=sub["forced"])                # the caller's table, in the batch's own numbering
        if sub.get("automaton") is not None:
            kw.update(token_automaton=sub["automaton"])           # the batch's automaton object: the options carry its key only
        if sub.get("patch_bias") is not None:
            kw.update(patch_bias=sub["patch_bias"])               # the batch's tensors: the options only say that there are some
        if sub.get("prefix") is not None:
            kw.update(prefix=sub["prefix"])                       # the caller's handle: the twin reads its bf16 build (made once, _prefix_for)
        ids = sub["input_ids"]
        if sub.get("beam_orig") is not None:                      # a beam batch is re-run from the rows the caller gave, not from their expansion
            bo = sub["beam_orig"]
            ids, am, image_index = bo["input_ids"], bo["attention_mask"], bo["image_index"]
            if bo["patch_bias"] is not None:
                kw.update(patch_bias=bo["patch_bias"])
        return fb.generate(input_ids=ids, attention_mask=am, pixel_values=pix, image_grid_thw=grid, max_new_tokens=group["T_max"],
                           schedule=group["schedule"], sync_every=group["sync_every"], use_graph=group["use_graph"], lane=("fb", group["lane"]),
                           output_hidden_states=output_hidden_states, return_dict_in_generate=return_dict_in_generate, image_index=image_index, **kw)

    @torch.no_grad()
    def score_completions(self, input_ids, attention_mask, pixel_values, image_grid_thw, completions, **generate_kwargs):
        """Log-likelihood of given completions: ``generate(forced_tokens=completions, max_new_tokens=n, output_token_logprobs=True,
        **generate_kwargs)`` (n = the table's width) with two more fields on the output object — ``completion_token_logprobs`` (B, n_steps):
        ``token_logprobs`` with 0.0 wherever the step was not forced or lies after the row's first EOS; ``completion_logprobs`` (B,): its row
        sums.  completions: what ``forced_tokens`` takes.  Several candidates for one image: repeat the prompt rows and pass ``image_index``.
        ``token_automaton=A`` (default ``None``; one of ``**generate_kwargs``, handed to generate(token_automaton=)): every step's row is constrained to the columns A allows after the forced prefix,
        so ``token_logprobs`` is the log-softmax over the ALLOWED columns — the closed-set probability: over the labels of a trie the
        probabilities of the first branching step sum to 1.  A completion that leaves the automaton scores ``-inf`` at that token.
        ``max_tokens=[len(c) for c in completions]`` (one of ``**generate_kwargs``, generate(max_tokens=)) ends every row with its own
        completion instead of letting the short ones run free to the table's width; it is not passed by default."""
        for k in ("forced_tokens", "max_new_tokens", "output_token_logprobs", "return_dict_in_generate"):
            if k in generate_kwargs:
                raise ValueError(f"score_completions sets generate({k}=...) itself")
        table = check_forced_tokens(completions, input_ids.shape[0], 2 ** 31 - 1, self.config.vocab_size)
        if not forced_tokens_active(table):
            raise ValueError("score_completions: generate(forced_tokens=...) holds no token to score")
        out = self.generate(input_ids=input_ids, attention_mask=attention_mask, pixel_values=pixel_values, image_grid_thw=image_grid_thw,
                            forced_tokens=table, max_new_tokens=table.shape[1], output_token_logprobs=True, **generate_kwargs)
        # the ids the decode loop itself stopped rows on (config id + the resolved options' list), not a second resolution of the arguments
        eos = out.past_key_values.eos_ids
        L = input_ids.shape[1]
        out["completion_token_logprobs"], out["completion_logprobs"] = completion_logprobs(out.token_logprobs, out.sequences[:, L:], table, eos)
        return out

    # ------------------------------------------------------------------ vl_decode (padt.py:342-412)
    @torch.no_grad()
    def vl_decode(self, object_vp_feats, low_res_image_embeds, high_res_image_embeds, image_grid_thws, visual_pes):
        cfg, dev = self.config, self.device
        flat = sum(object_vp_feats, [])
        if len(flat) == 0:                                        # padt.py:406-412 (the dummy pass of 383-393 is skipped)
            f32 = torch.float32                                   # same dtypes as the non-empty result (boxes / scores / logits are fp32)
            return {"pred_boxes": torch.zeros((0, 4), device=dev, dtype=f32),
                    "pred_score": torch.zeros((0, 1), device=dev, dtype=f32),
                    "pred_mask": torch.zeros((0, 8, 8), device=dev, dtype=f32),
                    "pred_mask_valid_hw": (), "sample_idx": []}
        grids = [[int(x) for x in g] for g in torch.as_tensor(image_grid_thws).tolist()]
        patch_num = [g[0] * g[1] * g[2] for g in grids]
        patch_off = [0]
        for n in patch_num:
            patch_off.append(patch_off[-1] + n)
        obj_sample, n_vp = [], []
        for si, feats in enumerate(object_vp_feats):
            for f in feats:
                obj_sample.append(si)
                n_vp.append(int(f.shape[0]))
        # the PaDT decoder reads fp32 or bf16 rows (its own operand pairs are bf16 (hi, lo)): fp16 rows of an fp16-operand model enter it
        # as fp32 (exact), never through a bf16 rounding
        def dec_in(t):
            t = t.to(dev).contiguous()
            if t.dtype == torch.float16:
                t = ops.cast_x16_f32(t)
            if not self.W.dec_hp and t.dtype == torch.float32:                      # the bf16-storage decoder (PADT_DECODER_HP=0) reads bf16 rows
                t = ops.cast_f32_bf16(t)
            return t
        feats_cat = torch.cat([f.to(dev) for f in flat], dim=0)
        feats_cat = dec_in(feats_cat if feats_cat.dtype in (torch.float16, torch.float32) else feats_cat.to(torch.bfloat16))
        low_res_image_embeds = dec_in(low_res_image_embeds)
        high_res_image_embeds = dec_in(high_res_image_embeds)
        bbox, score, masks, hw = self.vl_decoder.forward_objects(
            feats_cat, n_vp, low_res_image_embeds, high_res_image_embeds, visual_pes, obj_sample, patch_off, patch_num, grids)
        # "sample_idx_t": the same list as a device tensor (cached with the decoder's plan) for the device-side result pack
        # "sample_idx_t" / "pred_mask_src_hw": device copies for the device-side consumers (result pack, mask post-processing) — shared with the
        # decoder's cached plan: read-only
        return {"pred_boxes": bbox, "pred_score": score, "pred_mask": masks, "pred_mask_valid_hw": hw,
                "sample_idx": obj_sample, "sample_idx_t": self.vl_decoder.last_sample_t, "pred_mask_src_hw": self.vl_decoder.last_src_hw}

    def forward(self, *args, is_main=True, **kwargs):
        if is_main:
            raise NotImplementedError("teacher-forced forward_main is a training surface (out of scope); use generate()")
        return self.vl_decode(*args, **kwargs)

    __call__ = forward
