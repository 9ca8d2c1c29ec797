"""What a ``generate()`` call asks for, as host logic that imports without a GPU: the drop-in surface's argument policy (which HF / reference
arguments are ignored, refused or unknown), ``GenOptions`` — the ONE named, hashable value a call's arguments and the checkpoint's
generation_config.json resolve to, carried from ``generate_launch`` through the decode session to a re-run on the bf16 twin — and
``StepMode``, the part of it that selects the decode step's kernel sequence (one captured graph per value)."""
import math
import numbers
import struct
from dataclasses import InitVar, dataclass, fields
from typing import NamedTuple, Optional

import torch

from . import ops


# ------------------------------------------------------------------------------------------------ generate() argument policy
# HF / reference generate() arguments that cannot change what this path returns: accepted when they hold one of the listed values
# (None = any value), otherwise NotImplementedError.
_GENERATE_IGNORED = {
    "attn_implementation": None, "tokenizer": None, "assistant_tokenizer": None, "cache_implementation": None, "logits_to_keep": None,
    "generation_config": (None,), "output_attentions": (False, None),
    # GenerationConfig fields callers pass routinely and the reference's generate() accepts without effect on this path:
    "bos_token_id": None, "decoder_start_token_id": None, "return_legacy_cache": None,
    "num_beams": (1, None), "num_beam_groups": (1, None), "num_return_sequences": (1, None), "penalty_alpha": (None,), "min_new_tokens": (0, None),
    "min_length": (0, None), "force_words_ids": (None,), "token_healing": (False, None),
    "length_penalty": (1.0, None), "early_stopping": (False, None), "typical_p": (1.0, None), "min_p": (None,), "epsilon_cutoff": (0.0, None),
    "eta_cutoff": (0.0, None), "encoder_repetition_penalty": (1.0, None), "guidance_scale": (None, 1.0), "renormalize_logits": (False, None),
}
# arguments the reference honours (padt.py:418-424,445,511-533,570-580,719-737) and this path does not implement
# ... and, through generate()'s NAMED parameters only, the four pure-ban processors: as a stray keyword of check_generate_kwargs they stay refused
_GENERATE_NAMED_ONLY = ("no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens")
_GENERATE_REJECTED = ("inputs", "prefix_allowed_tokens_fn", "assistant_model", "streamer",
                      "negative_prompt_ids", "negative_prompt_attention_mask", "pixel_values_videos", "video_grid_thw", "second_per_grid_ts",
                      "inputs_embeds", "past_key_values", "position_ids", "cache_position", "rope_deltas", "stop_strings", "max_time",
                      "sequence_bias", "forced_bos_token_id", "forced_eos_token_id",
                      "prompt_lookup_num_tokens", "dola_layers", "labels")


def check_generate_kwargs(kwargs: dict, max_new_tokens, max_length, prompt_len) -> int:
    """The drop-in surface's argument policy (see generate()): → the effective max_new_tokens.  Raises NotImplementedError naming an
    argument the reference honours and this path does not, ValueError (HF's _validate_model_kwargs wording) for an unknown one."""
    for k in list(kwargs):
        v = kwargs[k]
        if k in _GENERATE_REJECTED or k in _GENERATE_NAMED_ONLY:
            if v is None:
                continue                                              # the reference's own default
            raise NotImplementedError(f"generate({k}=...) is not implemented on the MI355X path (the reference honours it, padt.py:414-580): "
                                      "remove the argument or run the reference for this call")
        if k in _GENERATE_IGNORED:
            ok = _GENERATE_IGNORED[k]
            if ok is None or any(v is o or (not isinstance(v, (torch.Tensor, list, tuple, dict)) and v == o) for o in ok):
                continue
            raise NotImplementedError(f"generate({k}={v!r}) is not implemented on the MI355X path (supported: {ok})")
        raise ValueError(f"The following `model_kwargs` are not used by the model: ['{k}'] (note: typos in the generate arguments will also "
                         "show up in this list)")
    if max_new_tokens is None:
        if max_length is not None:
            if prompt_len is None or int(max_length) <= int(prompt_len):
                raise ValueError(f"Input length of input_ids is {prompt_len}, but `max_length` is set to {max_length}. This can lead to unexpected "
                                 "behavior. You should consider increasing `max_length` or, better yet, setting `max_new_tokens`.")
            return int(max_length) - int(prompt_len)
        return 1024
    return int(max_new_tokens)


TOP_LOGPROBS_MAX = ops.TOPK_ROWS_MAX_K


def check_top_logprobs(top_logprobs) -> int:
    """generate(top_logprobs=...) → k: None / 0 is off (0), 1 <= k <= 32 asks for the k best candidates of every step; a negative or
    non-integer value raises ValueError, a larger one NotImplementedError naming the argument and the cap."""
    if top_logprobs is None:
        return 0
    if isinstance(top_logprobs, bool) or not isinstance(top_logprobs, numbers.Integral) or int(top_logprobs) < 0:
        raise ValueError(f"generate(top_logprobs={top_logprobs!r}): a non-negative integer (or None) is required")
    if int(top_logprobs) > TOP_LOGPROBS_MAX:
        raise NotImplementedError(f"generate(top_logprobs={int(top_logprobs)}): at most top_logprobs={TOP_LOGPROBS_MAX} candidates per step are "
                                  "selected on the device — ask for output_scores=True and reduce the rows yourself beyond that")
    return int(top_logprobs)


# ------------------------------------------------------------------------------------------------ generate(forced_tokens=)
def check_forced_tokens(forced_tokens, B, max_new_tokens, vocab_size, patches_per_row=None) -> torch.Tensor:
    """generate(forced_tokens=F) → the table in its one normal form: an int32 CPU tensor (B, n), n <= max_new_tokens, every free entry -1.
    F: a (B, n) integer tensor or a list of B lists of ints (ragged rows are padded with -1); ids are numbered like ``sequences[:, L:]``
    (text ids < vocab_size, sample b's own VRT ids vocab_size + its patch offset in the batch).  ValueError naming ``forced_tokens`` for a
    wrong batch size, n > max_new_tokens, a non-integer dtype, or an id >= vocab_size + patches_per_row[b] (patches_per_row: the table rows
    past the text vocabulary that row b may name, i.e. the batch's prototype count; None skips that bound) — so the device never sees an id
    outside the table."""
    name = "generate(forced_tokens=...)"
    if isinstance(forced_tokens, torch.Tensor):
        t = forced_tokens.detach().cpu()
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError(f"{name}: an integer tensor is required, got dtype {t.dtype}")
        if t.dim() != 2:
            raise ValueError(f"{name}: a (batch, n) tensor is required, got shape {tuple(t.shape)}")
        t = t.to(torch.int64)
    else:
        try:
            rows = [list(r) for r in forced_tokens]
        except TypeError:
            raise ValueError(f"{name}: a (batch, n) integer tensor or a list of per-row id lists is required, got {forced_tokens!r}") from None
        n = max((len(r) for r in rows), default=0)
        t = torch.full((len(rows), n), -1, dtype=torch.int64)
        for b, r in enumerate(rows):
            for j, v in enumerate(r):
                if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                    if isinstance(v, torch.Tensor) and v.numel() == 1 and not (v.dtype.is_floating_point or v.dtype == torch.bool):
                        v = int(v)
                    else:
                        raise ValueError(f"{name}: token ids must be integers, got {v!r} (row {b})")
                t[b, j] = int(v)
    if t.shape[0] != int(B):
        raise ValueError(f"{name}: {t.shape[0]} rows for a batch of {int(B)} samples")
    if t.shape[1] > int(max_new_tokens):
        raise ValueError(f"{name}: {t.shape[1]} steps but max_new_tokens={int(max_new_tokens)}")
    t = torch.where(t < 0, torch.full_like(t, -1), t)
    if patches_per_row is None:
        limit = torch.full((t.shape[0], 1), 2 ** 31 - 1, dtype=torch.int64)
    else:
        if len(patches_per_row) != t.shape[0]:
            raise ValueError(f"{name}: patches_per_row has {len(patches_per_row)} entries for {t.shape[0]} rows")
        limit = (torch.as_tensor([int(p) for p in patches_per_row], dtype=torch.int64) + int(vocab_size))[:, None]
    bad = (t >= limit).nonzero()
    if bad.numel():
        b, j = (int(x) for x in bad[0])
        raise ValueError(f"{name}: id {int(t[b, j])} at row {b}, step {j} is outside the table ({int(limit[b if limit.shape[0] > 1 else 0, 0])} rows: "
                         "the text vocabulary and the batch's patches)")
    return t.to(torch.int32)


def forced_tokens_active(table) -> bool:
    """False for an absent, empty or all-free (-1) table: such a call IS the call without the argument — same options, same captured graph."""
    return table is not None and table.numel() > 0 and bool((table >= 0).any())


def completion_logprobs(token_logprobs: torch.Tensor, tokens: torch.Tensor, forced: torch.Tensor, eos_ids):
    """score_completions' masking, pure: → (completion_token_logprobs, completion_logprobs).  token_logprobs / tokens (B, n_steps): a forced
    generate's fields (tokens = sequences[:, L:]); forced: the normalised table (B, n) of check_forced_tokens.  An entry keeps its value where
    the step was forced (forced[b, t] >= 0, t < n) and no earlier token of the row is one of eos_ids (the EOS step itself counts); every other
    entry is 0.0.  The sums are over the kept entries, so a -inf log-prob makes the completion's -inf."""
    B, T = token_logprobs.shape
    f = torch.full((B, T), -1, dtype=torch.int64)
    n = min(T, forced.shape[1])
    f[:, :n] = forced[:, :n].to(torch.int64).cpu()
    tok = tokens.detach().cpu().to(torch.int64)
    is_eos = torch.zeros_like(tok, dtype=torch.bool)
    for e in eos_ids:
        is_eos |= tok == int(e)
    after = (is_eos.long().cumsum(1) - is_eos.long()) > 0
    keep = ((f >= 0) & ~after).to(token_logprobs.device)
    per = torch.where(keep, token_logprobs, torch.zeros_like(token_logprobs))
    return per, per.sum(1)


# ------------------------------------------------------------------------------------------------ generate(token_automaton=)
class TokenAutomaton:
    """Which tokens a row may emit next, given what it emitted so far: a deterministic automaton over the generated tokens, walked on the
    device inside the decode step (padt_token_automaton).  NOT HF's ``prefix_allowed_tokens_fn``: there is no callback — the table is data.

    States are 0 .. S - 1.  ``edges[s]`` lists state s' edges ``(key, next_state)``; a key is a text id (0 <= id < vocab_size) or a class:
    ``VRT`` — any of the row's own patch tokens (table columns vocab_size + vrt_off[row] .. vocab_size + vrt_off[row + 1] - 1), ``TEXT`` — any
    text id that is none of the call's EOS ids, ``EOS`` — any of the call's EOS ids.  An explicit id wins over a class.  The tokens allowed in
    a state are exactly the keys of its edges.  Two rules the device shares with ``allowed()``: a token without an edge (possible under
    ``forced_tokens``, a caller processor or a ``schedule`` only) takes the row to the off-automaton state ``OFF`` for good; and wherever the
    allowed set is empty (``OFF``, a terminal state, a ``VRT``-only state of a sample without patches) the EOS ids are allowed and nothing else.

    Normal form: per state the edges sorted by key (classes first), duplicate keys refused; ``key`` = (start, edges) is hashable and equal
    for equal tables — it decides whether two batches can share a decode group.  ``ValueError`` naming ``token_automaton`` for a malformed
    table (``check(vocab_size)`` adds the id range once the vocabulary is known), ``NotImplementedError`` above ``MAX_STATES`` states /
    ``MAX_EDGES`` edges (the packed table's caps)."""
    VRT, TEXT, EOS = -1, -2, -3
    OFF = -1
    MAX_STATES, MAX_EDGES = ops.TOKEN_AUTOMATON_MAX_STATES, ops.TOKEN_AUTOMATON_MAX_EDGES
    _CLASS_NAMES = {-1: "VRT", -2: "TEXT", -3: "EOS"}

    def __init__(self, edges, start=0):
        name = "token_automaton"
        try:
            table = [list(st) for st in edges]
        except TypeError:
            raise ValueError(f"{name}: a list of per-state edge lists [(key, next_state), ...] is required, got {edges!r}") from None
        S = len(table)
        n_edges = sum(len(st) for st in table)
        if S > self.MAX_STATES or n_edges > self.MAX_EDGES:
            raise NotImplementedError(f"{name}: {S} states / {n_edges} edges; at most {self.MAX_STATES} states and {self.MAX_EDGES} edges "
                                      "on the MI355X path")
        if isinstance(start, bool) or not isinstance(start, numbers.Integral) or not 0 <= int(start) < S:
            raise ValueError(f"{name}: the start state {start!r} is outside the table ({S} states)")
        norm = []
        for s, st in enumerate(table):
            out = []
            for e in st:
                try:
                    k, nx = e
                except (TypeError, ValueError):
                    raise ValueError(f"{name}: state {s}: an edge is a (key, next_state) pair, got {e!r}") from None
                for v in (k, nx):
                    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                        raise ValueError(f"{name}: state {s}: keys and states must be integers, got {e!r}")
                k, nx = int(k), int(nx)
                if k < self.EOS:
                    raise ValueError(f"{name}: state {s}: key {k} is neither a token id nor one of VRT / TEXT / EOS")
                if k >= 2 ** 31 - 1:
                    raise ValueError(f"{name}: state {s}: id {k} is outside the vocabulary")
                if not 0 <= nx < S:
                    raise ValueError(f"{name}: state {s}: next_state {nx} is outside the table ({S} states)")
                out.append((k, nx))
            out.sort()
            for a, b in zip(out, out[1:]):
                if a[0] == b[0]:
                    raise ValueError(f"{name}: state {s}: duplicate key {self._CLASS_NAMES.get(a[0], a[0])}")
            norm.append(tuple(out))
        self.start, self.edges = int(start), tuple(norm)
        # a reachable state without edges must be terminal: entered through EOS edges only
        seen, todo = {self.start}, [self.start]
        if not self.edges[self.start]:
            raise ValueError(f"{name}: the start state {self.start} has no edges")
        while todo:
            s = todo.pop()
            for k, nx in self.edges[s]:
                if not self.edges[nx] and k != self.EOS:
                    raise ValueError(f"{name}: state {nx} has no edges and is entered from state {s} through "
                                     f"{self._CLASS_NAMES.get(k, k)}, not through an EOS edge")
                if nx not in seen:
                    seen.add(nx)
                    todo.append(nx)

    @property
    def key(self):
        return (self.start, self.edges)

    def __eq__(self, other):
        return self.key == other.key if isinstance(other, TokenAutomaton) else NotImplemented

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return f"TokenAutomaton({len(self.edges)} states, {sum(len(e) for e in self.edges)} edges, start={self.start})"

    def check(self, vocab_size):
        """The id range, once the vocabulary is known: ValueError naming token_automaton for an explicit id outside [0, vocab_size).  → self."""
        for s, st in enumerate(self.edges):
            for k, _ in st:
                if k >= int(vocab_size):
                    raise ValueError(f"token_automaton: state {s}: id {k} is not a text id (0 <= id < {int(vocab_size)}); patch tokens are "
                                     "named through the VRT class")
        return self

    @classmethod
    def from_sequences(cls, seqs, repeat=False):
        """The trie of the given sequences (items: text ids or the class constants); every complete sequence is followed by an ``EOS`` edge
        into one terminal state.  ``repeat=True``: the end of a sequence also carries the start state's edges, so another sequence may follow —
        the OVD / closed-set-label case, ``from_sequences([name_ids + [VRT] * 5 for name_ids in categories], repeat=True)``.  States are
        numbered breadth-first in key order, so the same set of sequences gives the same key in whatever order it is listed."""
        name = "token_automaton"
        children, ends = [{}], set()
        n_seq = 0
        for seq in seqs:
            n_seq += 1
            node = 0
            try:
                items = list(seq)
            except TypeError:
                raise ValueError(f"{name}: from_sequences takes sequences of ids / class constants, got {seq!r}") from None
            if not items:
                raise ValueError(f"{name}: from_sequences: an empty sequence")
            for k in items:
                if isinstance(k, bool) or not isinstance(k, numbers.Integral) or int(k) < cls.EOS:
                    raise ValueError(f"{name}: from_sequences: {k!r} is neither a token id nor one of VRT / TEXT / EOS")
                k = int(k)
                if k == cls.EOS:
                    raise ValueError(f"{name}: from_sequences appends the EOS edge itself: sequences must not contain EOS")
                if k not in children[node]:
                    if len(children) > 2 * cls.MAX_EDGES:
                        raise NotImplementedError(f"{name}: more than {cls.MAX_STATES} states / {cls.MAX_EDGES} edges on the MI355X path")
                    children[node][k] = len(children)
                    children.append({})
                node = children[node][k]
            ends.add(node)
        if n_seq == 0:
            raise ValueError(f"{name}: from_sequences needs at least one sequence")
        term = len(children)
        table = []
        for node, ch in enumerate(children):
            st = dict(ch)
            if node in ends:
                if repeat:
                    for k, nx in children[0].items():
                        if k in st:
                            raise ValueError(f"{name}: from_sequences(repeat=True): after a complete sequence the key "
                                             f"{cls._CLASS_NAMES.get(k, k)} both continues a longer sequence and starts a new one")
                        st[k] = nx
                st[cls.EOS] = term
            table.append(st)
        table.append({})
        # canonical numbering: breadth-first from the start state, edges in key order
        order, number = [0], {0: 0}
        for node in order:
            for k in sorted(table[node]):
                nx = table[node][k]
                if nx not in number:
                    number[nx] = len(order)
                    order.append(nx)
        return cls([[(k, number[nx]) for k, nx in table[node].items()] for node in order], start=0)

    def step(self, state, token, n_text, vrt_range, eos_ids):
        """The state after `token` in `state` (OFF stays OFF; a token without an edge leads to OFF)."""
        if state == self.OFF:
            return self.OFF
        token = int(token)
        st = dict(self.edges[state])
        lo, hi = int(n_text) + int(vrt_range[0]), int(n_text) + int(vrt_range[1])
        if 0 <= token < n_text and token in st:
            return st[token]
        if lo <= token < hi:
            return st.get(self.VRT, self.OFF)
        if 0 <= token < n_text:
            return st.get(self.EOS if token in {int(e) for e in eos_ids} else self.TEXT, self.OFF)
        return self.OFF

    def walk(self, tokens, n_text, vrt_range, eos_ids):
        """The state after the generated prefix `tokens`, from the start state."""
        state = self.start
        for tok in tokens:
            state = self.step(state, tok, n_text, vrt_range, eos_ids)
        return state

    def allowed_in(self, state, n_text, vrt_range, eos_ids):
        """The sorted table columns allowed in `state` for a row whose patches are columns n_text + vrt_range[0] .. n_text + vrt_range[1] - 1."""
        eos = sorted({int(e) for e in eos_ids if 0 <= int(e) < n_text})
        out = set()
        if state != self.OFF:
            st = dict(self.edges[state])
            if self.TEXT in st:
                out.update(range(int(n_text)))
                if self.EOS not in st:
                    out.difference_update(eos)
            if self.VRT in st:
                out.update(range(int(n_text) + int(vrt_range[0]), int(n_text) + int(vrt_range[1])))
            if self.EOS in st:
                out.update(eos)
            out.update(k for k in st if 0 <= k < n_text)
        return sorted(out) if out else eos

    def allowed(self, tokens, n_text, vrt_range, eos_ids):
        """The sorted list of allowed table columns after the generated prefix `tokens` — a plain Python walk: the specification the kernel
        is compared against.  n_text: the vocabulary size; vrt_range = (lo, hi): the row's patch offsets (vrt_off[row], vrt_off[row + 1]);
        eos_ids: the call's EOS ids."""
        return self.allowed_in(self.walk(tokens, n_text, vrt_range, eos_ids), n_text, vrt_range, eos_ids)

    def accepts(self, tokens, n_text, vrt_range, eos_ids):
        """True when every token of `tokens`, up to and including the first EOS id, was allowed where it stands."""
        state, eos = self.start, {int(e) for e in eos_ids}
        for tok in tokens:
            if int(tok) not in self.allowed_in(state, n_text, vrt_range, eos_ids):
                return False
            if int(tok) in eos:
                return True
            state = self.step(state, tok, n_text, vrt_range, eos_ids)
        return True


def check_token_automaton(token_automaton, vocab_size):
    """generate(token_automaton=A) → A, checked against the vocabulary; None stays None.  ValueError naming the argument for anything that
    is not a TokenAutomaton."""
    if token_automaton is None:
        return None
    if not isinstance(token_automaton, TokenAutomaton):
        raise ValueError(f"generate(token_automaton=...): a padt_amd.generation.TokenAutomaton is required, got {type(token_automaton).__name__} "
                         "(it is not HF's prefix_allowed_tokens_fn: a callable cannot run inside the captured step)")
    return token_automaton.check(vocab_size)


# ------------------------------------------------------------------------------------------------ generate(logit_bias=, patch_bias=, exponential_decay_length_penalty=)
# The three edits that ADD to a score.  The specification (score_bias_row below is its plain statement; the head kernel, padt_vrt_head_bias,
# is compared against it bit for bit), for a row's masked logit l of table column c at step t (tokens generated so far), in HF's processor
# order — SequenceBias, RepetitionPenalty, the bans, ExponentialDecayLengthPenalty:
#   1. x = l + bias[c]: one fp32 add; bias[c] is the call's logit_bias entry of a text column, the row's patch_bias entry of its own patch
#      column, 0 where nothing is listed; -inf is a legal bias and acts as a ban
#   2. the repetition penalty on x          3. logit mask, schedule, ban bitmap: -inf
#   4. c one of the call's EOS ids and t > start: v = v + |v| * a[t], a[t] = fp32(factor ** (t - start) - 1) computed in double and rounded
#      once (decay_table); the product and the sum round separately.  A column that is already -inf stays -inf (HF produces NaN there).
# NOT HF's sequence_bias (multi-token sequences), min_new_tokens, min_length or forced_eos_token_id: those stay refused by name.
def _bias_value(name, v, where):
    if isinstance(v, torch.Tensor) and v.numel() == 1:
        v = v.item()
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{name}: a bias is a real number, got {v!r} ({where})")
    v = float(v)
    if math.isnan(v) or v == math.inf or abs(v) > 3.4028234663852886e38 and v != -math.inf:
        raise ValueError(f"{name}: a bias must be a finite fp32 value or -inf (a ban), got {v!r} ({where})")
    return float(torch.tensor(v, dtype=torch.float32))               # what the device adds


def check_logit_bias(logit_bias, vocab_size):
    """generate(logit_bias=) → its normal form: a tuple of (id, bias) pairs sorted by id, the biases rounded to fp32, zero entries dropped
    (adding 0 is the call without the entry); None for None / nothing left.  Accepts a dict {id: bias} or a list of [id, bias] pairs (the
    OpenAI / vLLM shapes; string keys that spell integers included).  Text ids only: a VRT id raises NotImplementedError pointing to
    patch_bias, NaN / +inf / a repeated or malformed entry ValueError, all naming logit_bias."""
    name = "generate(logit_bias=...)"
    if logit_bias is None:
        return None
    if isinstance(logit_bias, dict):
        items = list(logit_bias.items())
    else:
        try:
            items = [tuple(e) for e in logit_bias]
        except TypeError:
            raise ValueError(f"{name}: a dict {{id: bias}} or a list of [id, bias] pairs is required, got {logit_bias!r}") from None
    out = {}
    for e in items:
        if len(e) != 2:
            raise ValueError(f"{name}: an entry is an [id, bias] pair, got {e!r}")
        k, v = e
        if isinstance(k, str) and k.strip().lstrip("+-").isdigit():
            k = int(k)
        if isinstance(k, torch.Tensor) and k.numel() == 1 and not (k.dtype.is_floating_point or k.dtype == torch.bool):
            k = int(k)
        if isinstance(k, bool) or not isinstance(k, numbers.Integral):
            raise ValueError(f"{name}: token ids must be integers, got {k!r}")
        k = int(k)
        if k < 0:
            raise ValueError(f"{name}: id {k} is outside the vocabulary")
        if k >= int(vocab_size):
            raise NotImplementedError(f"{name}: id {k} is not a text id (0 <= id < {int(vocab_size)}): a VRT id means another patch in every "
                                      "sample — bias a sample's own patches with patch_bias")
        if k in out:
            raise ValueError(f"{name}: id {k} is listed twice")
        out[k] = _bias_value(name, v, f"id {k}")
    key = tuple(sorted((k, v) for k, v in out.items() if v != 0.0))
    return key or None


def check_patch_bias(patch_bias, B, patches=None, grids=None):
    """generate(patch_bias=) → its normal form: a list of B entries, each None or an fp32 CPU tensor over that row's own patches in VRT-id
    order; None when every entry is None.  An entry may be a 1-D tensor / sequence of the row's patch count or a 2-D map (h/2, w/2) over the
    merged patch grid (flattened row-major: VRT-id order).  A map keeps its shape until `grids` is given, so that it can still be checked
    against the row's grid; with `grids` every entry comes back 1-D.  patches: the rows' patch counts, grids: their merged grids (h/2, w/2),
    once known (modeling._launch runs the check again with both).  ValueError naming patch_bias and the row for a wrong batch size, rank,
    length or map shape, NaN or +inf."""
    name = "generate(patch_bias=...)"
    if patch_bias is None:
        return None
    if isinstance(patch_bias, torch.Tensor):
        raise ValueError(f"{name}: a list of {int(B)} per-row entries (None, a 1-D tensor or a 2-D map) is required, got one tensor of shape "
                         f"{tuple(patch_bias.shape)}")
    try:
        rows = list(patch_bias)
    except TypeError:
        raise ValueError(f"{name}: a list of per-row entries is required, got {patch_bias!r}") from None
    if len(rows) != int(B):
        raise ValueError(f"{name}: {len(rows)} entries for a batch of {int(B)} samples")
    out = []
    for b, r in enumerate(rows):
        if r is None:
            out.append(None)
            continue
        try:
            t = torch.as_tensor(r).detach().cpu()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{name}: row {b}: a float tensor is required, got {type(r).__name__}") from None
        if t.dtype == torch.bool or t.dtype.is_complex or t.dim() not in (1, 2):
            raise ValueError(f"{name}: row {b}: a 1-D float tensor over the row's patches or a 2-D (h/2, w/2) map is required, got dtype "
                             f"{t.dtype}, shape {tuple(t.shape)}")
        t = t.to(torch.float64)
        if bool(torch.isnan(t).any()) or bool((t == math.inf).any()):
            raise ValueError(f"{name}: row {b}: NaN or +inf (a bias is finite or -inf, a ban)")
        t32 = t.to(torch.float32)
        if bool((torch.isinf(t32) & ~torch.isinf(t)).any()):
            raise ValueError(f"{name}: row {b}: a value beyond fp32's range")
        if t.dim() == 2 and grids is not None and tuple(t.shape) != tuple(int(x) for x in grids[b]):
            raise ValueError(f"{name}: row {b}: a {tuple(t.shape)} map for a merged patch grid of {tuple(int(x) for x in grids[b])}")
        if patches is not None and t.numel() != int(patches[b]):
            raise ValueError(f"{name}: row {b}: {t.numel()} values for {int(patches[b])} patches")
        out.append((t32.reshape(-1) if grids is not None else t32).contiguous())      # a map keeps its shape until it was checked against the grid
    return out if any(t is not None for t in out) else None


def check_decay_length_penalty(value, max_new_tokens=None):
    """generate(exponential_decay_length_penalty=(start, factor)) → (int start, float factor), None for None.  start: an integer >= 0, counted
    in generated tokens as HF counts it; factor: a positive real; factor ** max_new_tokens must be finite in fp32 (the largest entry of the
    device table).  ValueError naming the argument."""
    name = "generate(exponential_decay_length_penalty=...)"
    if value is None:
        return None
    try:
        start, factor = value
    except (TypeError, ValueError):
        raise ValueError(f"{name}: a (start_index, decay_factor) pair is required, got {value!r}") from None
    if isinstance(start, bool) or not isinstance(start, numbers.Integral) or int(start) < 0:
        raise ValueError(f"{name}: start_index must be an integer >= 0, got {start!r}")
    if isinstance(factor, bool) or not isinstance(factor, numbers.Real) or not (float(factor) > 0.0) or math.isinf(float(factor)):
        raise ValueError(f"{name}: decay_factor must be a positive real number, got {factor!r}")
    start, factor = int(start), float(factor)
    if max_new_tokens is not None:
        try:
            top = factor ** int(max_new_tokens)
        except OverflowError:
            top = math.inf
        if not top <= 3.4028234663852886e38:
            raise ValueError(f"{name}: decay_factor ** max_new_tokens = {factor!r} ** {int(max_new_tokens)} is not finite in fp32")
    return (start, factor)


def decay_table(decay, t_max, n_steps=None) -> torch.Tensor:
    """The device table of the decay (start, factor): fp32 (t_max,) with a[t] = fp32(factor ** (t - start) - 1) for start < t < n_steps —
    computed in double with Python's pow, as HF's ExponentialDecayLengthPenalty computes its scalar, and rounded once, as its tensor multiply
    rounds it — and 0 (no edit) everywhere else.  n_steps: the call's max_new_tokens, the range check_decay_length_penalty validated (a
    session's table may be longer than the call: the steps past n_steps are never run, and their powers may not even fit a double); None:
    t_max.  A power beyond the double range is +inf, never an exception.  None → all 0."""
    t_max = int(t_max)
    n = t_max if n_steps is None else max(0, min(t_max, int(n_steps)))
    vals = [0.0] * t_max
    if decay is not None:
        start, factor = decay
        for t in range(start + 1, n):
            try:
                vals[t] = factor ** (t - start) - 1
            except OverflowError:
                vals[t] = math.inf
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32)


def score_bias_row(logits, bias=None, penalty=1.0, seen=None, banned=None, eos_ids=(), a_t=0.0):
    """Steps 1-4 of the specification above on fp32 rows (..., n): logits — the masked logits (−inf outside the mask); bias (n,) or None; seen /
    banned — bool (..., n) masks or None; a_t — the decay table's entry of this step (0: no edit).  Plain torch, one rounding per step."""
    x = logits.to(torch.float32)
    if bias is not None:
        x = x + bias.to(torch.float32)
    if float(penalty) != 1.0 and seen is not None:
        pen = torch.tensor(float(penalty), dtype=torch.float32, device=x.device)
        x = torch.where(seen, torch.where(x < 0, x * pen, x / pen), x)
    if banned is not None:
        x = torch.where(banned, torch.full_like(x, -math.inf), x)
    a = torch.tensor(float(a_t), dtype=torch.float32, device=x.device)
    if float(a) != 0.0:
        x = x.clone()
        for e in dict.fromkeys(int(e) for e in eos_ids):
            v = x[..., e]
            x[..., e] = torch.where(torch.isinf(v) & (v < 0), v, v + v.abs() * a)
    return x


# ------------------------------------------------------------------------------------------------ generate(frequency_penalty=, presence_penalty=, patch_suppression=)
# The edits that GROW with what a row has already generated.  The specification (count_state / count_penalty_row below are its plain
# statement; padt_count_update and the COUNTS head kernels, padt_vrt_head_counts, are compared against them bit for bit), for row b at step t:
#   * count[c]: how often table column c — a text id or one of the row's own VRT columns — occurs among the row's GENERATED tokens 0 .. t - 1.
#     The prompt is never counted (vLLM's rule for these two penalties, unlike the repetition penalty's `seen`), forced tokens are, the pad
#     tokens behind a row's end are not.
#   * near[j]: over the VRT tokens of the row's COMPLETED runs — maximal runs of consecutive VRT tokens followed by a non-VRT token; a run
#     still open at step t suppresses nothing, so an object's own VRT tokens may sit next to each other — the number whose patch (y, x) on
#     the row-major merged grid (h/2, w/2) lies within max(|y - y_j|, |x - x_j|) <= radius of patch j.
#   * the edit, between the repetition penalty and the mask / schedule / ban filter (the order: bias, repetition penalty, token counts, patch
#     neighbourhood, bans, EOS decay), all in fp32: s = s - f * count; s = s - p * (count > 0) — vLLM's apply_penalties, two products and two
#     differences each rounded on its own — then, where near > 0: s = s - near * penalty (+inf: -inf, a ban; near == 0 is no operation, so
#     there is no 0 * inf).
# The device keeps the state of the tokens it selected FROM: the step whose token ends a row with an EOS id is not counted (nothing is selected
# after it, so no output can tell) — count_state(tokens, n) with n the tokens before that one is what the tables then hold.
COUNT_MAX_RADIUS = ops.COUNT_MAX_RADIUS


def _row_floats(name, value, B, lo, hi):
    """a float in [lo, hi], or one per row → list of B floats (rounded to fp32: what the device reads); None for None"""
    if value is None:
        return None
    if isinstance(value, torch.Tensor):
        if value.dtype == torch.bool or value.dtype.is_complex or value.dim() > 1:
            raise ValueError(f"generate({name}=...): a number or one number per row is required, got a {value.dtype} tensor of shape {tuple(value.shape)}")
        value = value.item() if value.dim() == 0 else value.tolist()
    if isinstance(value, numbers.Real) and not isinstance(value, bool):
        vals = [value] * int(B)
    else:
        if isinstance(value, (str, bytes)):
            raise ValueError(f"generate({name}=...): a number or one number per row is required, got {value!r}")
        try:
            vals = list(value)
        except TypeError:
            raise ValueError(f"generate({name}=...): a number or one number per row is required, got {value!r}") from None
        if len(vals) != int(B):
            raise ValueError(f"generate({name}=...): {len(vals)} entries for a batch of {int(B)} samples")
    out = []
    for b, v in enumerate(vals):
        if isinstance(v, torch.Tensor) and v.numel() == 1:
            v = v.item()
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError(f"generate({name}=...): row {b}: a real number is required, got {v!r}")
        v = float(v)
        if not math.isfinite(v) or not lo <= v <= hi:
            raise ValueError(f"generate({name}=...): row {b}: {v!r} is not a finite number in [{lo:g}, {hi:g}] (vLLM's rule)")
        out.append(float(torch.tensor(v, dtype=torch.float32)))
    return out


def check_count_penalties(frequency_penalty, presence_penalty, B):
    """generate(frequency_penalty=, presence_penalty=) → (f, p): two lists of B fp32-rounded floats, or (None, None) when both are off (None, 0
    or all zeros: the call without the arguments).  Each argument is a float or a sequence of B floats, finite and within [-2, 2]; anything
    else raises ValueError naming the argument."""
    f = _row_floats("frequency_penalty", frequency_penalty, B, -2.0, 2.0)
    p = _row_floats("presence_penalty", presence_penalty, B, -2.0, 2.0)
    if not any(f or ()) and not any(p or ()):
        return None, None
    return f or [0.0] * int(B), p or [0.0] * int(B)


def check_patch_suppression(patch_suppression, B):
    """generate(patch_suppression=) → a list of B entries, each None (the row is not suppressed) or (int radius, float penalty); None for None
    or a list of Nones.  One (radius, penalty) pair applies to every row.  radius: an integer in [0, COUNT_MAX_RADIUS] — above the cap
    NotImplementedError naming it, negative or not an integer ValueError; penalty: > 0, finite or +inf (a ban) — zero, negative or NaN
    ValueError.  All name the argument."""
    name = "generate(patch_suppression=...)"
    if patch_suppression is None:
        return None

    def pair(e, where):
        try:
            radius, penalty = e
        except (TypeError, ValueError):
            raise ValueError(f"{name}: a (radius, penalty) pair is required, got {e!r}{where}") from None
        if isinstance(radius, torch.Tensor) and radius.numel() == 1 and not (radius.dtype.is_floating_point or radius.dtype == torch.bool):
            radius = int(radius)
        if isinstance(radius, bool) or not isinstance(radius, numbers.Integral) or int(radius) < 0:
            raise ValueError(f"{name}: radius must be an integer >= 0, got {radius!r}{where}")
        if int(radius) > COUNT_MAX_RADIUS:
            raise NotImplementedError(f"{name}: radius {int(radius)}{where}; at most {COUNT_MAX_RADIUS} on the MI355X path")
        if isinstance(penalty, torch.Tensor) and penalty.numel() == 1:
            penalty = penalty.item()
        if isinstance(penalty, bool) or not isinstance(penalty, numbers.Real) or not float(penalty) > 0.0:
            raise ValueError(f"{name}: penalty must be a number > 0 (+inf bans), got {penalty!r}{where}")
        pen = float(torch.tensor(float(penalty), dtype=torch.float32))
        if pen == math.inf and float(penalty) != math.inf or pen == 0.0:
            raise ValueError(f"{name}: penalty {penalty!r} is not an fp32 value > 0{where}")
        return int(radius), pen

    # one pair for the call: two scalars, the first an integer (a tuple, or a list as a dict config spells it) — never a list of two rows
    ps = patch_suppression
    if (isinstance(ps, (tuple, list)) and len(ps) == 2 and isinstance(ps[0], numbers.Integral) and not isinstance(ps[0], bool)
            and isinstance(ps[1], numbers.Real)):
        return [pair(ps, "")] * int(B)
    if isinstance(ps, (str, bytes, numbers.Number, torch.Tensor)):
        raise ValueError(f"{name}: a (radius, penalty) pair or a list of per-row pairs / Nones is required, got {ps!r}")
    try:
        rows = list(ps)
    except TypeError:
        raise ValueError(f"{name}: a (radius, penalty) pair or a list of per-row pairs / Nones is required, got {ps!r}") from None
    if len(rows) != int(B):
        raise ValueError(f"{name}: {len(rows)} entries for a batch of {int(B)} samples")
    out = [None if r is None else pair(r, f" (row {b})") for b, r in enumerate(rows)]
    return out if any(r is not None for r in out) else None


def count_state(tokens, n, vocab, lo, hi, grid=None, radius=None):
    """The counts of a row after its first n generated tokens, by a plain walk → (count, near): count — a dict {table column: occurrences}
    over text ids and the row's own VRT columns vocab + lo .. vocab + hi - 1 (a VRT id outside that range counts nowhere, but is a VRT token
    of its run); near — a list of hi - lo ints over the row's patches, row-major on grid = (hp, wp): for every VRT token of a COMPLETED run
    (followed by a non-VRT token within the n tokens) on one of the row's own patches (y, x), + 1 on the window max(|dy|, |dx|) <= radius
    clipped at the grid's border.  radius None (or grid None): no suppression, near is all 0.  The caller chooses n: tokens behind a row's
    end are not generated tokens and must not be passed as such."""
    vocab, lo, hi = int(vocab), int(lo), int(hi)
    row = [int(x) for x in tokens[: int(n)]]
    count = {}
    near = [0] * (hi - lo)
    if radius is not None and grid is not None:
        hp, wp = int(grid[0]), int(grid[1])
        if hp * wp != hi - lo:
            raise ValueError(f"count_state: a {hp} x {wp} grid for {hi - lo} patches")
    run = []
    for tok in row:
        is_vrt = tok >= vocab
        own = is_vrt and lo <= tok - vocab < hi
        if (0 <= tok < vocab) or own:
            count[tok] = count.get(tok, 0) + 1
        if is_vrt:
            if own:
                run.append(tok - vocab - lo)
            continue
        if radius is not None and grid is not None:                   # a non-VRT token: the run before it, if any, is complete
            for j in run:
                y, x = divmod(j, wp)
                for yy in range(max(0, y - int(radius)), min(hp, y + int(radius) + 1)):
                    for xx in range(max(0, x - int(radius)), min(wp, x + int(radius) + 1)):
                        near[yy * wp + xx] += 1
        run = []
    return count, near


def count_penalty_row(logits, counts=None, frequency_penalty=0.0, presence_penalty=0.0, near=None, suppression_penalty=0.0, bias=None,
                      penalty=1.0, seen=None, banned=None, eos_ids=(), a_t=0.0):
    """score_bias_row with the count edits in their place — bias, repetition penalty, TOKEN COUNTS, PATCH NEIGHBOURHOOD, bans, EOS decay — on
    fp32 rows (..., n): counts / near — integer or float (..., n) tensors over the row's columns (near is 0 on text columns), None = all 0
    and no edit; frequency_penalty / presence_penalty / suppression_penalty — numbers, or (..., 1) tensors for per-row values.  Plain torch,
    one rounding per operation: x -= f * counts; x -= p * (counts > 0); where near > 0 (and the penalty > 0): x -= near * penalty."""
    x = score_bias_row(logits, bias=bias, penalty=penalty, seen=seen)
    as_t = lambda v: v.to(device=x.device, dtype=torch.float32) if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float32, device=x.device)
    if counts is not None:
        c = counts.to(device=x.device, dtype=torch.float32)
        x = x - as_t(frequency_penalty) * c
        x = x - as_t(presence_penalty) * (c > 0).to(torch.float32)
    if near is not None:
        nr = near.to(device=x.device, dtype=torch.float32)
        pen = as_t(suppression_penalty)
        on = (nr > 0) & (pen > 0)
        x = torch.where(on, x - torch.where(on, nr, torch.ones_like(nr)) * torch.where(pen > 0, pen, torch.ones_like(pen)), x)
    return score_bias_row(x, banned=banned, eos_ids=eos_ids, a_t=a_t)


# ------------------------------------------------------------------------------------------------ generate(stop_sequences=, min_tokens=, max_tokens=)
# How a row ENDS.  The specification (stop_ban_ids / stop_state below are its plain statement; padt_stop_ban and padt_stop_match are compared
# against them bit for bit), for a row that holds n generated tokens after a step:
#   * before the step's head, with t = n tokens so far: while t < min_tokens every EOS id (the config's and the call's list) is banned —
#     HF's MinNewTokensLengthLogitsProcessor(prompt_len, min_tokens, eos_ids); a pure ban, so its place among the processors does not matter;
#   * after the step: 1. token n - 1 is an EOS id → "eos" (a forced EOS still ends the row, whatever min_tokens says);  2. n >= min_tokens
#     and one of the sequences equals the row's last tokens → "stop", the lowest index among those completing (vLLM's rule: a sequence
#     completing below min_tokens is ignored, and not matched retroactively later);  3. n >= max_tokens → "length".
# The prompt is never matched; the sequence's tokens stay in the output, as an EOS does.
# NOT HF's min_new_tokens / min_length / stop_strings / max_time: those names stay refused exactly as they are.
STOP_MAX_SEQS, STOP_MAX_LEN = ops.STOP_RULES_MAX_SEQS, ops.STOP_RULES_MAX_LEN
NO_BUDGET = 2 ** 31 - 1          # max_tokens of a row without a budget: never reached


def check_stop_sequences(stop_sequences, vocab_size=None):
    """generate(stop_sequences=) → its normal form: a tuple of id tuples in the caller's order (``stop_index`` names a position in it; a
    repeated sequence keeps both places); None for None.  Text ids only: a VRT id raises NotImplementedError with the rule table's wording, an
    empty list, an empty sequence or a malformed id ValueError, more than STOP_MAX_SEQS sequences or STOP_MAX_LEN ids in one
    NotImplementedError naming the argument and the cap."""
    name = "stop_sequences"
    if stop_sequences is None:
        return None
    if isinstance(stop_sequences, (str, bytes, numbers.Integral)):
        raise ValueError(f"generate({name}=...): a list of token-id lists is required, got {stop_sequences!r} (strings need the tokenizer: "
                         "stop_strings stays refused)")
    try:
        seqs = [s.tolist() if isinstance(s, torch.Tensor) else s for s in stop_sequences]
        seqs = [list(s) for s in seqs]
    except TypeError:
        raise ValueError(f"generate({name}=...): a list of token-id lists is required, got {stop_sequences!r}") from None
    if not seqs:
        raise ValueError(f"generate({name}=[]): an empty list stops nothing — pass None")
    if len(seqs) > STOP_MAX_SEQS:
        raise NotImplementedError(f"generate({name}=...): {len(seqs)} sequences; at most {STOP_MAX_SEQS} on the MI355X path")
    out = []
    for i, s in enumerate(seqs):
        if not s:
            raise ValueError(f"generate({name}=...): sequence {i} is empty")
        if len(s) > STOP_MAX_LEN:
            raise NotImplementedError(f"generate({name}=...): sequence {i} has {len(s)} ids; at most {STOP_MAX_LEN} on the MI355X path")
        out.append(tuple(ops._rule_ids(name, s, vocab_size)))
    return tuple(out)


def stop_table(sequences) -> torch.Tensor:
    """The packed int32 CPU table padt_stop_match reads (ops.STOP_RULES_INTS ints, fixed size; layout in include/padt_hip.h) for stop
    sequences in check_stop_sequences' normal form; None / (): no sequence."""
    seqs = check_stop_sequences(sequences) if sequences else ()
    t = [ops.STOP_RULES_MAGIC, len(seqs)] + [len(s) for s in seqs] + [0] * (STOP_MAX_SEQS - len(seqs))
    for s in seqs:
        t += list(s) + [0] * (STOP_MAX_LEN - len(s))
    t += [0] * (ops.STOP_RULES_INTS - len(t))
    return torch.tensor(t, dtype=torch.int32)


def _row_counts(name, value, B):
    """an int, or one int per row → (is_scalar, list of B ints)"""
    if isinstance(value, torch.Tensor):
        if value.dtype.is_floating_point or value.dtype.is_complex or value.dtype == torch.bool or value.dim() > 1:
            raise ValueError(f"generate({name}=...): an integer or one integer per row is required, got a {value.dtype} tensor of shape {tuple(value.shape)}")
        value = int(value) if value.dim() == 0 else value.tolist()
    if isinstance(value, numbers.Integral) and not isinstance(value, bool):
        return True, [int(value)] * int(B)
    try:
        vals = list(value)
    except TypeError:
        raise ValueError(f"generate({name}=...): an integer or one integer per row is required, got {value!r}") from None
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"generate({name}=...): an integer or one integer per row is required, got {v!r}")
    if len(vals) != int(B):
        raise ValueError(f"generate({name}=...): {len(vals)} entries for a batch of {int(B)} samples")
    return False, [int(v) for v in vals]


def check_max_tokens(max_tokens, B, max_new_tokens):
    """generate(max_tokens=) → a list of B budgets (an int applies to every row), None for None.  ValueError naming the argument and the row
    unless 1 <= max_tokens[b] <= max_new_tokens."""
    if max_tokens is None:
        return None
    _, vals = _row_counts("max_tokens", max_tokens, B)
    for b, v in enumerate(vals):
        if not 1 <= v <= int(max_new_tokens):
            raise ValueError(f"generate(max_tokens=...): row {b}: {v} is outside [1, max_new_tokens={int(max_new_tokens)}]")
    return vals


def check_min_tokens(min_tokens, B, max_new_tokens, max_tokens=None):
    """generate(min_tokens=) → an int (one value for the call: part of GenOptions) or a list of B ints (per-batch data), None for None.
    max_tokens: check_max_tokens' list or None — a row's budget is its entry, or max_new_tokens.  ValueError naming the argument and the row
    for a negative value or one above the row's budget."""
    if min_tokens is None:
        return None
    scalar, vals = _row_counts("min_tokens", min_tokens, B)
    for b, v in enumerate(vals):
        budget = int(max_new_tokens) if max_tokens is None else int(max_tokens[b])
        if v < 0:
            raise ValueError(f"generate(min_tokens=...): row {b}: {v} is negative")
        if v > budget:
            raise ValueError(f"generate(min_tokens=...): row {b}: {v} tokens are more than the row's budget of {budget} "
                             f"({'max_new_tokens' if max_tokens is None else 'its max_tokens'})")
    return vals[0] if scalar and vals else (None if scalar else vals)


def stop_ban_ids(step, min_tokens, eos_ids):
    """The ids generate(min_tokens=) bans at the step that selects token `step` (the row holds `step` generated tokens): every id of eos_ids
    while step < min_tokens, nothing afterwards — sorted, without duplicates or negative (unused) entries."""
    return sorted({int(e) for e in eos_ids if int(e) >= 0}) if int(step) < int(min_tokens) else []


def stop_state(tokens, n, sequences, min_tokens, max_tokens, eos_ids):
    """Does the row's n-th generated token end it?  → (finished, reason, index): reason "eos" / "stop" / "length" (None: not finished), index
    the matched sequence or -1.  tokens: the row's generated tokens (the first n are read); sequences: check_stop_sequences' normal form or
    None; eos_ids: every id that ends a row.  Precedence: EOS, then the lowest-indexed sequence equal to tokens[n - m : n] (only when
    n >= min_tokens and m <= n), then the budget (n >= max_tokens; None: no budget).  The state of a row over a whole run is the FIRST n at
    which this holds (stop_scan): a row is not looked at again after it finished."""
    n = int(n)
    if n < 1:
        return False, None, -1
    row = [int(x) for x in tokens[:n]]
    if row[-1] in {int(e) for e in eos_ids}:
        return True, "eos", -1
    if n >= int(min_tokens):
        for i, s in enumerate(sequences or ()):
            m = len(s)
            if 1 <= m <= n and row[n - m:] == [int(x) for x in s]:
                return True, "stop", i
    if max_tokens is not None and n >= int(max_tokens):
        return True, "length", -1
    return False, None, -1


def stop_scan(tokens, sequences, min_tokens, max_tokens, eos_ids):
    """The first n at which stop_state(tokens, n, ...) finishes the row → (finish_step = n - 1, reason, index); (-1, "length", -1) for a
    row still running after all of `tokens`."""
    for n in range(1, len(tokens) + 1):
        fin, reason, index = stop_state(tokens, n, sequences, min_tokens, max_tokens, eos_ids)
        if fin:
            return n - 1, reason, index
    return -1, "length", -1


# ------------------------------------------------------------------------------------------------ generate(beam_width=, n_best=, beam_length_penalty=, beam_early_stopping=)
# Beam search: the K best hypotheses of every sample, kept and reordered on the device.  The specification (beam_step / beam_backtrace below are
# its plain statement; padt_beam_step and padt_beam_finalize are compared against them bit for bit) is HF 5.x's GenerationMixin._beam_search,
# spelled without its -1e9 arithmetic: an impossible score IS -inf, an empty store entry IS empty.  Two deliberate differences from HF: before
# step 0 the live scores are [0, -inf, ...] where HF holds [0, -1e9, ...] — the results differ only when beam 0 has fewer than `keep` finite
# columns at step 0 (HF then continues copies of beam 0 at -1e9; here those slots are dead) — and a step's score is the log-softmax of the
# PROCESSED row (logit_bias / patch_bias / the EOS decay applied first: the value token_logprobs defines), where HF normalises before its
# processors.  NOT HF's num_beams / num_return_sequences / length_penalty / early_stopping: those names stay refused exactly as they are.
BEAM_MAX_WIDTH = ops.BEAM_MAX_WIDTH
BEAM_EARLY = {False: 0, True: 1, "never": 2}          # the early-stopping code of the device's beam config
_NEG_INF = -math.inf


def check_beam(beam_width=None, n_best=None, beam_length_penalty=None, beam_early_stopping=None, n_eos=1):
    """generate(beam_width=K, n_best=n, beam_length_penalty=lp, beam_early_stopping=es) → the option's one normal form (K, n, lp, es) with
    n = 1, lp = 1.0, es = False where not given; None when beam_width is None.  K: an integer >= 1; keep = max(2, 1 + n_eos) * K (HF's
    beams_to_keep) must fit ops.TOPK_ROWS_MAX_K and K <= BEAM_MAX_WIDTH — above either cap NotImplementedError naming beam_width and the cap;
    1 <= n <= K; lp a finite float; es one of False / True / "never".  Anything else, or one of the other three without beam_width,
    ValueError naming the argument."""
    others = dict(n_best=n_best, beam_length_penalty=beam_length_penalty, beam_early_stopping=beam_early_stopping)
    if beam_width is None:
        for name, v in others.items():
            if v is not None:
                raise ValueError(f"generate({name}={v!r}) needs beam_width: it is a beam-search option")
        return None
    if isinstance(beam_width, bool) or not isinstance(beam_width, numbers.Integral) or int(beam_width) < 1:
        raise ValueError(f"generate(beam_width={beam_width!r}): an integer >= 1 is required")
    K = int(beam_width)
    keep = beam_keep(K, n_eos)
    if K > BEAM_MAX_WIDTH:
        raise NotImplementedError(f"generate(beam_width={K}): at most beam_width={BEAM_MAX_WIDTH} on the MI355X path")
    if keep > ops.TOPK_ROWS_MAX_K:
        raise NotImplementedError(f"generate(beam_width={K}) with {int(n_eos)} EOS ids keeps {keep} candidates per step; at most "
                                  f"{ops.TOPK_ROWS_MAX_K} are selected on the device — lower beam_width or shorten the eos_token_id list")
    n = 1 if n_best is None else n_best
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 1 <= int(n) <= K:
        raise ValueError(f"generate(n_best={n_best!r}): an integer in [1, beam_width={K}] is required")
    lp = 1.0 if beam_length_penalty is None else beam_length_penalty
    if isinstance(lp, bool) or not isinstance(lp, numbers.Real) or not math.isfinite(float(lp)):
        raise ValueError(f"generate(beam_length_penalty={beam_length_penalty!r}): a finite number is required")
    es = False if beam_early_stopping is None else beam_early_stopping
    if not (es is False or es is True or es == "never" and isinstance(es, str)):
        raise ValueError(f"generate(beam_early_stopping={beam_early_stopping!r}): False, True or \"never\" is required")
    return K, int(n), float(lp), es


def check_beam_compatible(opts, processors=False, criteria=False, reference=False, output_scores=False, output_logits=False):
    """What generate(beam_width=) refuses by name (NotImplementedError): everything that depends on a row's generated HISTORY — that state
    (seen, hist, counts, automaton state, stop matches) does not follow the beams yet — sampling, and the outputs that describe ONE
    hypothesis per row.  opts: the call's resolved options (the beam entry aside); the other arguments say what else the call carries."""
    bad = []
    if opts.sampling is not None:
        bad.append("do_sample")
    if opts.repetition_penalty != 1.0:
        bad.append("repetition_penalty")
    if opts.rules is not None:
        n_gram, static, begin, words = opts.rules
        bad += [nm for nm, on in (("no_repeat_ngram_size", n_gram), ("bad_words_ids", words), ("suppress_tokens", static),
                                  ("begin_suppress_tokens", begin)) if on] or ["suppress_tokens"]
    if opts.automaton is not None:
        bad.append("token_automaton")
    if opts.forced:
        bad.append("forced_tokens")
    if opts.stop:
        bad.append("stop_sequences / min_tokens / max_tokens")
    if opts.counts:
        bad.append("frequency_penalty / presence_penalty / patch_suppression")
    if opts.top_logprobs:
        bad.append("top_logprobs")
    if opts.patch_logprobs:
        bad.append("output_patch_logprobs")
    if output_logits or opts.keep_logits:
        bad.append("output_logits")
    if output_scores or (opts.keep_scores and not (output_logits or opts.keep_logits or processors or criteria)):
        bad.append("output_scores")
    if processors:
        bad.append("logits_processor")
    if criteria:
        bad.append("stopping_criteria")
    if reference:
        bad.append("precision=\"reference\"")
    if bad:
        raise NotImplementedError(f"generate(beam_width=...) with {', '.join(bad)} is not implemented on the MI355X path: a row's history state "
                                  "does not follow the beams yet, and scores / candidates describe one hypothesis per row — drop the argument "
                                  "or run without beam_width")


def check_beam_session(config, batch, K):
    """What a beam call needs of the model and of a decode session, before anything is launched: the packed KV caches
    (head_dim 128, at most 16 query heads per kv head — padt_beam_reorder_kv moves their tiles) and batch * K rows within
    ops.DECODE_ROWS_MAX, what one decode step takes.  NotImplementedError naming beam_width."""
    if not (int(config.head_dim) == 128 and int(config.num_attention_heads) // int(config.num_key_value_heads) <= 16):
        raise NotImplementedError("generate(beam_width=...) needs the packed KV caches (head_dim 128: PaDT_Pro_3B / 7B): "
                                  "padt_beam_reorder_kv moves their tiles")
    if int(batch) * int(K) > ops.DECODE_ROWS_MAX:
        raise NotImplementedError(f"generate(beam_width={int(K)}) on {int(batch)} queries needs {int(batch) * int(K)} rows; a decode session takes "
                                  f"at most {ops.DECODE_ROWS_MAX} — lower beam_width or split the batch")


def beam_keep(K, n_eos):
    """HF's beams_to_keep: the candidates a step keeps per sample, so that K of them remain live when every EOS id was among the best."""
    return max(2, 1 + int(n_eos)) * int(K)


def beam_len_table(length_penalty, t_max) -> torch.Tensor:
    """The device table of the length penalty: fp32 (t_max,) with entry t = (t + 1) ** length_penalty — the divisor of a hypothesis that ends
    with its (t + 1)-th token — computed in double with Python's pow and rounded once.  The kernel only ever divides by an entry, so one
    captured graph serves every penalty.  A power beyond the fp32 range is +inf (or 0), never an exception."""
    vals = []
    for t in range(int(t_max)):
        try:
            vals.append(float(t + 1) ** float(length_penalty))
        except OverflowError:
            vals.append(math.inf)
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32)


def _f32(x):
    """the double x rounded to fp32 (to nearest even; beyond the range: +-inf), as a Python float"""
    if math.isfinite(x) and abs(x) <= 3.4028234663852886e38:
        return struct.unpack("f", struct.pack("f", x))[0]
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def _f32_add(a, b):
    """fp32 a + b of two fp32 values: the double sum of two fp32 values rounds to the fp32 sum (no double rounding: 53 >= 2 * 24 + 2)."""
    return _f32(a + b)


def _f32_div(a, b):
    """fp32 a / b of two fp32 values (the double quotient rounds to the fp32 quotient for the same reason)."""
    if b == 0.0:
        return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    if math.isinf(a) and math.isinf(b):
        return math.nan
    return _f32(a / b)


def beam_new_state(K):
    """The state of one sample before step 0: live scores [0, -inf, ...], an empty finished store, the early-stop heuristic not yet
    satisfied (`open`), not done.  A store entry is (score, end step, parent beam, last token, last log-prob); empty: score -inf, end -1."""
    K = int(K)
    return dict(live=[0.0] + [_NEG_INF] * (K - 1), store=[(_NEG_INF, -1, -1, -1, 0.0)] * K, sent=[False] * K, open=True, done=False)


def beam_step(state, cand_val, cand_idx, t, keep, eos_ids, len_table, t_last, early=False, pad=0, length_penalty=None, cand_rep=None):
    """One sample, one step of the beam search → (tok, parent, lp, info): the K child rows' token, parent beam and step log-prob, and
    info = dict(order=, finishing=, merged=) for tests.  `state` (beam_new_state) is updated in place; a done sample returns pad rows with
    parent = the slot itself and changes nothing.

    cand_val[p][r] / cand_idx[p][r] (r < keep): live beam p's r-th best (log-prob, column) pair, descending (-inf / -1 once the finite
    columns run out); t: the step; len_table: beam_len_table's values for the call's penalty; t_last: the call's last step
    (max_new_tokens - 1); early: False / True / "never".  cand_rep[p][r] (optional): the log-prob REPORTED for the candidate — what the
    returned lp and the store's last log-prob hold — where it is not cand_val itself: generate() reports the value token_logprobs defines
    (the greedy step's fold of the head's partials), which differs from the top-k kernel's by a rounding; the values added are cand_val's.

      1. value = fp32(live[p] + cand_val[p][r]); a -inf value is no candidate (never live, never finishing).
      2. order by value descending, then lower beam, then lower rank; the first `keep` are the step's candidates.
      3. a candidate is FINISHING when its token is one of eos_ids or t == t_last.
      4. the first K non-finishing candidates become the live beams (in that order: live scores descend); a slot that cannot be filled is
         dead: score -inf, pad token, parent = itself.
      5. the finishing ones among the FIRST K candidates are merged into the finished store with score fp32(value / len_table[t]): store
         entries and new ones ordered by score descending, an old entry before a new one of equal score, new ones in candidate order; the K
         best stay.  No merge when early is True and the store is full, nor once the heuristic flag (`open`) is cleared.
      6. open &= fp32(live[0] / d) > min(store scores), d = len_table[t_last] when early == "never" and length_penalty > 0 (None: read
         off the table, which then ascends), else len_table[t]; an empty entry counts as -inf (HF: _check_early_stop_heuristic after
         cur_len += 1).
      7. done = not (open and not (early is True and store full) and not every candidate finishing)
         (HF: _beam_search_has_unfinished_sequences; no candidate at all: every one of none is finishing)."""
    K = len(state["live"])
    if state["done"]:
        return [int(pad)] * K, list(range(K)), [0.0] * K, dict(order=[], finishing=[], merged=[])
    eos = {int(e) for e in eos_ids}
    cands = []
    for p in range(K):
        if state["live"][p] == _NEG_INF:
            continue
        for r in range(int(keep)):
            lp, col = float(cand_val[p][r]), int(cand_idx[p][r])
            if col < 0 or lp == _NEG_INF or math.isnan(lp):
                continue
            v = _f32_add(state["live"][p], lp)
            if v == _NEG_INF:
                continue
            cands.append((-v, p, r, col, lp if cand_rep is None else float(cand_rep[p][r])))
    cands.sort(key=lambda c: c[:3])
    cands = cands[: int(keep)]
    finishing = [c[3] in eos or int(t) >= int(t_last) for c in cands]
    # 4. the live beams of the next step
    tok, parent, lps, live = [int(pad)] * K, list(range(K)), [0.0] * K, [_NEG_INF] * K
    n = 0
    for c, fin in zip(cands, finishing):
        if not fin and n < K:
            tok[n], parent[n], lps[n], live[n] = c[3], c[1], c[4], -c[0]
            n += 1
    # 5. the finished store
    full = all(state["sent"])
    merged = []
    if state["open"] and not (early is True and full):
        div = float(len_table[int(t)])
        new = [(_f32_div(-c[0], div), int(t), c[1], c[3], c[4]) for c, fin in list(zip(cands, finishing))[:K] if fin]
        new = [e for e in new if not math.isnan(e[0])]
        merged = new
        entries = [(e, s) for e, s in zip(state["store"], state["sent"])] + [(e, True) for e in new]
        entries.sort(key=lambda es: -es[0][0])                    # stable: old entries first, new ones in candidate order
        state["store"], state["sent"] = [e for e, _ in entries[:K]], [s for _, s in entries[:K]]
    state["live"] = live
    # 6. can a running beam still beat the worst finished one?
    asc = (len(len_table) > 1 and float(len_table[1]) > float(len_table[0])) if length_penalty is None else float(length_penalty) > 0.0
    d = float(len_table[int(t_last)]) if (isinstance(early, str) and early == "never" and asc) else float(len_table[int(t)])
    best = _f32_div(live[0], d)
    worst = min(e[0] for e in state["store"]) if all(state["sent"]) else _NEG_INF
    state["open"] = state["open"] and best > worst
    # 7. is the sample done?
    state["done"] = not (state["open"] and not (early is True and all(state["sent"])) and not all(finishing))
    return tok, parent, lps, dict(order=[(c[1], c[2]) for c in cands], finishing=finishing, merged=merged)


def beam_backtrace(store, beam_tok, beam_parent, beam_lp, n_best):
    """The n best store entries of ONE sample, walked back through the steps' records → a list of n hypotheses, each a dict(score=, length=,
    tokens=, logprobs=, rows=) — rows[t] = (t, beam): where the hidden row that produced token t lives (hidden_buf[t][sample * K + beam]).
    store: the state's store (best first); beam_tok / beam_parent / beam_lp [t][K]: what beam_step returned per step.  An empty store entry
    (nothing finished, possible only for a call that produced no candidate at all) gives an empty hypothesis with score -inf."""
    out = []
    for score, end, par, tok, lp in list(store)[: int(n_best)]:
        if end < 0:
            out.append(dict(score=_NEG_INF, length=0, tokens=[], logprobs=[], rows=[]))
            continue
        toks, lps, rows = [0] * (end + 1), [0.0] * (end + 1), [None] * (end + 1)
        toks[end], lps[end], rows[end] = int(tok), float(lp), (end, int(par))
        r = int(par)
        for t in range(end - 1, -1, -1):
            toks[t], lps[t] = int(beam_tok[t][r]), float(beam_lp[t][r])
            r = int(beam_parent[t][r])
            rows[t] = (t, r)
        out.append(dict(score=float(score), length=end + 1, tokens=toks, logprobs=lps, rows=rows))
    return out


# generate()'s named parameters a generation_config may carry: an explicit argument (not None) wins, as in HF (padt.py:436)
_GENERATE_CONFIG_NAMED = ("max_new_tokens", "max_length", "do_sample", "repetition_penalty", "eos_token_id", "pad_token_id", "temperature", "top_k",
                          "top_p", "no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "min_p", "typical_p",
                          "epsilon_cutoff", "eta_cutoff", "exponential_decay_length_penalty")
# ... and those whose value is this path's own default either way (hidden states and the dict output are what its callers consume)
_GENERATE_CONFIG_OWN = ("use_cache", "output_hidden_states", "return_dict_in_generate")


def generation_config_fields(generation_config) -> dict:
    """generate(generation_config=): the fields a ``transformers.GenerationConfig`` sets to something other than its default (to_diff_dict),
    or the entries of a dict; bookkeeping entries (``transformers_version``, ``_from_model_config`` …) are dropped.  Anything else is not a
    generation config: NotImplementedError naming the argument."""
    if generation_config is None:
        return {}
    if isinstance(generation_config, dict):
        d = dict(generation_config)
    else:
        try:
            from transformers import GenerationConfig
        except ImportError:                                           # no transformers: only dicts can be configs
            GenerationConfig = ()
        if not (GenerationConfig and isinstance(generation_config, GenerationConfig)):
            raise NotImplementedError(f"generate(generation_config={generation_config!r}) is not implemented on the MI355X path: pass a "
                                      "transformers.GenerationConfig or a dict of its fields")
        d = generation_config.to_diff_dict()
    return {k: v for k, v in d.items() if not k.startswith("_") and k != "transformers_version" and v is not None}


# ------------------------------------------------------------------------------------------------ what a generate() resolved to
class Sampling(NamedTuple):
    """do_sample=True: HF's Temperature → TopK → TopP → MinP → Typical → Epsilon → Eta warpers and the key of the device's counter-based
    generator.  The last four hold their "off" value unless HF would build the warper (resolve_options), so equal behaviour is equal options."""
    temperature: float
    top_k: int
    top_p: float
    seed: int
    min_p: float = 0.0               # MinPLogitsWarper: 0 < min_p <= 1
    typical_p: float = 1.0           # TypicalLogitsWarper: 0 < typical_p < 1
    epsilon_cutoff: float = 0.0      # EpsilonLogitsWarper: 0 < epsilon_cutoff < 1
    eta_cutoff: float = 0.0          # EtaLogitsWarper: 0 < eta_cutoff < 1

    @property
    def warpers(self) -> bool:
        """One of the four warpers after top-p is active: padt_warp_sample_rows_f32 runs after the sampling kernel."""
        return self.min_p > 0.0 or self.typical_p < 1.0 or self.epsilon_cutoff > 0.0 or self.eta_cutoff > 0.0


DECAY_OFF = (0, 1.0)     # exponential_decay_length_penalty spelled as off: HF's processor with factor 1 adds |v| * 0; here it IS no decay
_SAMPLING_OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
WARPER_NAMES = tuple(_SAMPLING_OFF)


class _ConfigOverlay:
    """A generation config whose listed fields are a call's own values (with_warpers)."""

    def __init__(self, base, over):
        self.__dict__.update(_base=base, _over=over)

    def __getattr__(self, name):
        over = self.__dict__["_over"]
        return over[name] if name in over else getattr(self.__dict__["_base"], name)


def with_warpers(gc, values):
    """The generation config `gc` with the call's min_p / typical_p / epsilon_cutoff / eta_cutoff in front of its own: `values` maps the names
    to what the caller passed, None = not passed.  resolve_options reads the four from the config it is given — that is how a call's values
    reach it from generate(), PipelinedRunner.submit and rec_batch."""
    over = {k: v for k, v in (values or {}).items() if v is not None}
    unknown = set(over) - set(WARPER_NAMES)
    if unknown:
        raise ValueError(f"not a sampling warper: {sorted(unknown)}")
    return _ConfigOverlay(gc, over) if over else gc


class StepMode(NamedTuple):
    """What selects the decode step's kernel sequence and output buffers (DecodeSession.head_and_select): run_steps keeps one captured graph
    per value.  Penalty, EOS ids, warper settings, seed and the rules' contents are not part of it: the captured step reads them from device memory."""
    sampling: bool = False           # the sampling kernel instead of the arg-max over the head's partials
    keep_scores: bool = False        # every step's processed fp32 rows are filed in `scores`
    keep_logits: bool = False        # ... and the rows before the warpers in `raw_scores`
    rules: bool = False              # the ban-bitmap kernel runs and the head writes -inf where it says
    token_logprobs: bool = False     # the LSE head + padt_greedy_step_lp, or the row kernel when the token is not the head's arg-max
    top_k: int = 0                   # padt_topk_logprob_rows_f32 over the step's row: k candidates ...
    patches: bool = False            # ... and / or the sample's own patch columns
    processors: bool = False         # the caller's logits_processor rewrites the rows (hooked loop: never captured)
    reference: bool = False          # precision="reference": reference.ReferencePath.step instead of step_kernels
    warpers: bool = False            # min_p / typical_p / epsilon_cutoff / eta_cutoff: padt_warp_sample_rows_f32 warps the row and draws
    forced: bool = False             # generate(forced_tokens=): the probe head / padt_forced_step / padt_forced_override read the session's table
    automaton: bool = False          # generate(token_automaton=): padt_token_automaton writes the bitmap the head reads (the union with the rules')
    bias: bool = False               # logit_bias / patch_bias / exponential_decay_length_penalty: padt_vrt_head_bias reads the session's bias vector and decay table
    stop: bool = False               # stop_sequences / min_tokens / max_tokens: padt_stop_ban in front of the head, padt_stop_match behind the bookkeeping kernel
    counts: bool = False             # frequency_penalty / presence_penalty / patch_suppression: padt_vrt_head_counts reads the session's count tables, padt_count_update keeps them
    beam: int = 0                    # generate(beam_width=K): the width; padt_beam_step in the place of padt_greedy_step over top_k = keep candidates per row, then padt_beam_reorder_kv


@dataclass(frozen=True)
class GenOptions:
    """What one generate() resolved to (resolve_options).  Equality is decode-group compatibility: batches share a session only when equal."""
    repetition_penalty: float = 1.0
    eos_ids: tuple = ()
    sampling: Optional[Sampling] = None          # None: greedy
    rules: Optional[tuple] = None                # the four pure bans as ops.gen_rules_key returns them; None: nothing banned
    keep_scores: bool = False                    # output_scores, output_logits or a hooked loop: the processed rows of every step are kept
    keep_logits: bool = False                    # output_logits under sampling only: there the scores are the warped rows, so the raw ones get a stash of their own
    token_logprobs: bool = False
    top_logprobs: int = 0                        # k; 0: off
    patch_logprobs: bool = False
    # generate(forced_tokens=): the batch forces tokens.  The table itself is per-batch data like the prompt history; this only says that the
    # step reads one.  Set with dataclasses.replace after resolve_options; part of equality (batches share a decode group only when both force
    # or neither does) but deliberately NOT a dataclass field: the fields are the options generate_kwargs() spells as generate() arguments for a
    # re-run, and the table travels with its batch instead (modeling._non_finite_batch).
    forced: InitVar[bool] = False
    # generate(token_automaton=A): A.key, or None.  Like `forced` an init-only attribute — part of equality, hash and repr (batches share a
    # decode group only when their automata are equal: a session holds ONE packed table), not a dataclass field and not in generate_kwargs():
    # the automaton object travels with its batch to a re-run.
    automaton: InitVar[Optional[tuple]] = None
    # generate(logit_bias=) in check_logit_bias' normal form, generate(exponential_decay_length_penalty=) as (start, factor), and "this batch
    # carries a patch_bias" (the tensors travel with their batch like the forced table).  Init-only attributes like the two above — part of
    # equality, hash and repr; spelled for a re-run by bias_kwargs(), not by generate_kwargs().
    logit_bias: InitVar[Optional[tuple]] = None
    decay: InitVar[Optional[tuple]] = None
    patch_bias: InitVar[bool] = False
    # generate(stop_sequences=) in check_stop_sequences' normal form, generate(min_tokens=) when it is ONE value for the call, and "this batch
    # carries per-row min_tokens / max_tokens" (the lists travel with their batch like the forced table).  Init-only attributes like those
    # above — part of equality, hash and repr; spelled for a re-run by stop_kwargs().
    stop_sequences: InitVar[Optional[tuple]] = None
    min_tokens: InitVar[Optional[int]] = None
    row_limits: InitVar[bool] = False
    # generate(frequency_penalty= / presence_penalty=) and generate(patch_suppression=): only WHETHER each mechanism is on — the per-row
    # values travel with their batch like the forced table, so batches with different values share a decode group (each writes its own rows
    # of the session's arrays) and a batch with the feature never shares one with a batch without.  Init-only attributes like those above.
    count_penalties: InitVar[bool] = False
    patch_suppression: InitVar[bool] = False
    # generate(beam_width=, n_best=, beam_length_penalty=, beam_early_stopping=) in check_beam's normal form (K, n_best, penalty, early
    # stopping), or None.  An init-only attribute like those above — part of equality, hash and repr; spelled for a re-run by beam_kwargs().
    beam: InitVar[Optional[tuple]] = None

    def __post_init__(self, forced, automaton, logit_bias, decay, patch_bias, stop_sequences, min_tokens, row_limits, count_penalties,
                      patch_suppression, beam):
        object.__setattr__(self, "beam", None if beam is None else (int(beam[0]), int(beam[1]), float(beam[2]), beam[3]))
        object.__setattr__(self, "count_penalties", bool(count_penalties))
        object.__setattr__(self, "patch_suppression", bool(patch_suppression))
        object.__setattr__(self, "stop_sequences", None if stop_sequences is None else tuple(tuple(int(i) for i in q) for q in stop_sequences))
        object.__setattr__(self, "min_tokens", None if min_tokens is None else int(min_tokens))
        object.__setattr__(self, "row_limits", bool(row_limits))
        object.__setattr__(self, "forced", bool(forced))
        object.__setattr__(self, "automaton", automaton)
        object.__setattr__(self, "logit_bias", logit_bias or None)
        object.__setattr__(self, "decay", None if decay is None else (int(decay[0]), float(decay[1])))
        object.__setattr__(self, "patch_bias", bool(patch_bias))

    def _key(self):
        # every field, whatever is added later, and the init-only attributes
        return tuple(getattr(self, f.name) for f in fields(self)) + (self.forced, self.automaton, self.logit_bias, self.decay, self.patch_bias,
                                                                          self.stop_sequences, self.min_tokens, self.row_limits,
                                                                          self.count_penalties, self.patch_suppression, self.beam)

    def __eq__(self, other):
        return self._key() == other._key() if isinstance(other, GenOptions) else NotImplemented

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        a = self.automaton                                        # the key of a large table is long: its size and hash stand for it
        auto = "None" if a is None else f"<{len(a[1])} states, {sum(len(e) for e in a[1])} edges, start {a[0]}, #{hash(a) & 0xffffffff:08x}>"
        args = [f"{f.name}={getattr(self, f.name)!r}" for f in fields(self)] + [f"forced={self.forced!r}", f"automaton={auto}"]
        lb = self.logit_bias
        args += [f"logit_bias={lb!r}" if lb is None or len(lb) <= 8 else f"logit_bias=<{len(lb)} ids, #{hash(lb) & 0xffffffff:08x}>",
                 f"decay={self.decay!r}", f"patch_bias={self.patch_bias!r}"]
        sq = self.stop_sequences
        args += [f"stop_sequences={sq!r}" if sq is None or sum(len(q) for q in sq) <= 16 else f"stop_sequences=<{len(sq)} sequences, #{hash(sq) & 0xffffffff:08x}>",
                 f"min_tokens={self.min_tokens!r}", f"row_limits={self.row_limits!r}", f"count_penalties={self.count_penalties!r}",
                 f"patch_suppression={self.patch_suppression!r}", f"beam={self.beam!r}"]
        return f"GenOptions({', '.join(args)})"

    @property
    def want_rows(self) -> bool:
        """top_logprobs / output_patch_logprobs select from the whole processed row."""
        return bool(self.top_logprobs or self.patch_logprobs)

    @property
    def write_back(self) -> bool:
        """The sampling kernel overwrites its rows with the warped scores: whoever reads the row after it must see what was sampled from."""
        return self.sampling is not None and bool(self.keep_scores or self.token_logprobs or self.want_rows or self.sampling.warpers)

    @property
    def score_bias(self) -> bool:
        """One of the three additive edits is on: the head is padt_vrt_head_bias with the session's bias vector and decay table."""
        return self.logit_bias is not None or self.decay is not None or self.patch_bias

    @property
    def stop(self) -> bool:
        """One of stop_sequences / min_tokens / max_tokens was given: the step runs padt_stop_ban and padt_stop_match, and the output
        object carries finish_reason / stop_index / finish_step."""
        return self.stop_sequences is not None or self.min_tokens is not None or self.row_limits

    @property
    def counts(self) -> bool:
        """frequency_penalty / presence_penalty or patch_suppression is on: the head is padt_vrt_head_counts over the session's count
        tables, which padt_count_update keeps behind the bookkeeping kernel."""
        return self.count_penalties or self.patch_suppression

    @property
    def beam_keep(self) -> int:
        """The candidates a beam step keeps per sample and asks of every row (HF's beams_to_keep over the call's EOS ids); 0 without beams."""
        return 0 if self.beam is None else beam_keep(self.beam[0], len(set(self.eos_ids)) or 1)

    @property
    def reads_prompt(self) -> bool:
        """A ban or the repetition penalty is active: the built-in processors see the caller's full (B, L) input_ids."""
        return self.repetition_penalty != 1.0 or self.rules is not None

    def gen_cfg(self) -> torch.Tensor:
        """The generation-config slots the head / selection kernels read (ops.gen_cfg_tensor), on the host."""
        s = self.sampling or Sampling(1.0, 0, 1.0, 0)
        return ops.gen_cfg_tensor(self.repetition_penalty, self.eos_ids, "cpu", do_sample=self.sampling is not None, seed=s.seed,
                                  temperature=s.temperature, top_k=s.top_k, top_p=s.top_p, write_back=self.write_back, min_p=s.min_p,
                                  typical_p=s.typical_p, epsilon_cutoff=s.epsilon_cutoff, eta_cutoff=s.eta_cutoff)

    def step_mode(self, processors: bool = False, reference: bool = False) -> StepMode:
        return StepMode(sampling=self.sampling is not None, keep_scores=self.keep_scores, keep_logits=self.keep_logits, rules=self.rules is not None,
                        token_logprobs=self.token_logprobs, top_k=self.beam_keep or self.top_logprobs, patches=self.patch_logprobs,
                        processors=bool(processors), reference=bool(reference), warpers=self.sampling is not None and self.sampling.warpers,
                        forced=self.forced, automaton=self.automaton is not None, bias=self.score_bias, stop=self.stop, counts=self.counts,
                        beam=0 if self.beam is None else self.beam[0])

    def warper_kwargs(self) -> dict:
        """min_p / typical_p / epsilon_cutoff / eta_cutoff as explicit generate() keywords (with_warpers values), next to generate_kwargs():
        off is spelled 0.0 / 1.0, never None, so that no generation_config can switch a warper back on."""
        s = self.sampling
        return dict(_SAMPLING_OFF) if s is None else {name: getattr(s, name) for name in WARPER_NAMES}

    def bias_kwargs(self) -> dict:
        """logit_bias / exponential_decay_length_penalty as explicit generate() keywords, next to generate_kwargs() and warper_kwargs().
        Off is spelled as off ({} / (0, 1.0): no entry, a factor whose table is all 0), never None, so that no generation_config can switch
        the decay back on.  The patch_bias tensors travel with their batch."""
        return dict(logit_bias=dict(self.logit_bias or ()), exponential_decay_length_penalty=self.decay or DECAY_OFF)

    def stop_kwargs(self) -> dict:
        """stop_sequences / min_tokens as explicit generate() keywords, next to generate_kwargs(), warper_kwargs() and bias_kwargs().  No
        generation_config carries either, so off is None.  Per-row min_tokens / max_tokens travel with their batch."""
        sq = self.stop_sequences
        return dict(stop_sequences=None if sq is None else [list(q) for q in sq], min_tokens=self.min_tokens)

    def beam_kwargs(self) -> dict:
        """beam_width / n_best / beam_length_penalty / beam_early_stopping as explicit generate() keywords, next to generate_kwargs() and the
        other *_kwargs().  No generation_config carries them, so off is None."""
        K, n, lp, es = self.beam or (None, None, None, None)
        return dict(beam_width=K, n_best=n, beam_length_penalty=lp, beam_early_stopping=es)

    def generate_kwargs(self) -> dict:
        """Explicit generate() arguments that resolve back to these options under ANY generation_config: what is off is spelled as off (0, [],
        False), never as None, so that a checkpoint default cannot switch it back on; the 1-token bad words travel as suppress_tokens.
        output_scores / output_logits are the caller's to pass: they also decide what is returned, which the options do not record."""
        n_gram, static, begin, words = self.rules or (0, (), (), ())
        kw = dict(do_sample=False) if self.sampling is None else dict(do_sample=True, **self.sampling._asdict())
        for name in WARPER_NAMES:                                 # not arguments of generate_launch: warper_kwargs()
            kw.pop(name, None)
        return dict(kw, repetition_penalty=self.repetition_penalty, eos_token_id=list(self.eos_ids), no_repeat_ngram_size=n_gram,
                    bad_words_ids=[list(wd) for wd in words], suppress_tokens=list(static), begin_suppress_tokens=list(begin),
                    output_token_logprobs=self.token_logprobs, top_logprobs=self.top_logprobs, output_patch_logprobs=self.patch_logprobs)


def resolve_options(gc, config_eos_id, vocab_size, do_sample=None, repetition_penalty=None, eos_token_id=None, temperature=None, top_k=None,
                    top_p=None, seed=None, keep_scores=False, keep_logits=False, no_repeat_ngram_size=None, bad_words_ids=None,
                    suppress_tokens=None, begin_suppress_tokens=None, output_token_logprobs=False, top_logprobs=None,
                    output_patch_logprobs=False) -> GenOptions:
    """generate_launch's arguments (same names) → GenOptions.  gc: the model's generation_config, whose field applies where the argument is
    None (HF: padt.py:436) — and, through with_warpers, the call's min_p / typical_p / epsilon_cutoff / eta_cutoff; config_eos_id / vocab_size: the model config's.  Pure but for the seed, which is drawn from torch's global
    generator when sampling without one (so torch.manual_seed makes runs repeatable) — and only then."""
    top_logprobs = check_top_logprobs(top_logprobs)
    dflt = lambda name, v: getattr(gc, name, None) if v is None else v
    do_sample = dflt("do_sample", do_sample)
    temperature, top_k, top_p = float(dflt("temperature", temperature)), int(dflt("top_k", top_k)), float(dflt("top_p", top_p))
    # the four warpers after top-p come from gc alone (a call's own values: with_warpers): validated as HF's classes validate them, whatever
    # the mode; a gc without the attribute means off
    warp = {}
    for name, (lo, hi, lo_open, hi_open) in (("min_p", (0.0, 1.0, False, False)), ("typical_p", (0.0, 1.0, True, False)),
                                             ("epsilon_cutoff", (0.0, 1.0, False, True)), ("eta_cutoff", (0.0, 1.0, False, True))):
        v = getattr(gc, name, None)
        v = _SAMPLING_OFF[name] if v is None else v
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not ((lo < v or (not lo_open and v == lo)) and (v < hi or (not hi_open and v == hi))):
            raise ValueError(f"generate({name}={v!r}): a number in {'(' if lo_open else '['}{lo:g}, {hi:g}{')' if hi_open else ']'} is required "
                             f"(HF's {name} warper)")
        warp[name] = float(v)
    if do_sample and top_k == 1:
        do_sample = False                                         # sampling among the single best token IS the arg-max
    samp = None
    if do_sample:
        if temperature <= 0:
            raise ValueError("temperature must be strictly positive (HF TemperatureLogitsWarper)")
        if top_p < 1.0 and not (0 < top_k <= 1024):
            raise NotImplementedError("top_p < 1 is supported together with 0 < top_k <= 1024 (the nucleus is taken over the top-k survivors)")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        samp = Sampling(temperature, top_k, top_p, int(seed), **warp)      # a value HF builds no warper for IS its off value (0 / 1 / 0 / 0)
    eos = dflt("eos_token_id", eos_token_id)
    eos = (int(eos),) if isinstance(eos, int) else tuple(int(e) for e in eos)
    if config_eos_id not in eos or len(eos) > 4:
        raise NotImplementedError("eos_token_id must contain config.eos_token_id and hold at most 4 ids")
    # the four pure bans in canonical form (None: nothing banned — then no kernel is added and the head gets no bitmap)
    rules = ops.gen_rules_key(dflt("no_repeat_ngram_size", no_repeat_ngram_size), dflt("bad_words_ids", bad_words_ids),
                              dflt("suppress_tokens", suppress_tokens), dflt("begin_suppress_tokens", begin_suppress_tokens),
                              eos_ids=eos, vocab_size=vocab_size)
    if keep_logits and rules is not None and samp is None:
        raise NotImplementedError("generate(output_logits=True) with a logits processor active (no_repeat_ngram_size, bad_words_ids, suppress_tokens "
                                  "or begin_suppress_tokens): only the processed rows are kept on this path — ask for output_scores=True")
    return GenOptions(repetition_penalty=float(dflt("repetition_penalty", repetition_penalty)), eos_ids=eos, sampling=samp, rules=rules,
                      keep_scores=bool(keep_scores), keep_logits=bool(keep_logits) and samp is not None, token_logprobs=bool(output_token_logprobs),
                      top_logprobs=top_logprobs, patch_logprobs=bool(output_patch_logprobs))
