"""LLM side of the hot loop: dynamic VRT embedding, prefill, hipGraph-replayed decode steps, VRT head, greedy loop.

Host work here is integer bookkeeping (packing, position ids, cache slots) and kernel sequencing; all arithmetic runs in
libpadt_hip.so.  Differences from the reference's control flow that do not change results:
  * prompts are PACKED (left-padding is dropped instead of masked) — attention is per-sample varlen, so padded and
    packed runs see identical keys; rope positions follow transformers==4.50 ``get_rope_index`` and are
    padding-independent (position of step t = max prompt position + 1 + t);
  * the [embed_tokens ‖ prototypes] table is never concatenated (padt.py:194,228 rebuild it every forward);
  * only the last prompt position goes through the VRT head (padt.py:294 computes all L positions, :713 keeps one);
  * a decode step is ONE captured hipGraph replayed per token; argmax, EOS/pad bookkeeping, token append and the
    per-step hidden-state stash all happen on device, the host syncs once per `sync_every` steps.
"""
import gc
from dataclasses import dataclass
from typing import List, Optional


import torch

from . import ops
from .config import PaDTConfig
from .generation import BEAM_EARLY, NO_BUDGET, GenOptions, StepMode, beam_len_table, decay_table, stop_table

I32 = torch.int32


# ------------------------------------------------------------------------------------------------ host integer prep
def rope_index_packed(cfg: PaDTConfig, rows: List[List[int]], grids: List[List[int]]):
    """transformers==4.50.0 ``get_rope_index`` on unpadded token lists (called at padt.py:263).

    Returns (pos [3][T_total] list-of-lists per sample, next_pos per sample = max+1).
    text run: running index on all 3 axes; image: t = start, h = start+row, w = start+col over the merged grid;
    next run starts at previous max + 1.
    """
    m = cfg.vision_config.spatial_merge_size
    out, nxt = [], []
    gi = 0
    for toks in rows:
        chunks: List[torch.Tensor] = []
        st = 0
        n_img = sum(1 for i in range(len(toks) - 1)
                    if toks[i] == cfg.vision_start_token_id and toks[i + 1] == cfg.image_token_id)
        for _ in range(n_img):
            ed = toks.index(cfg.image_token_id, st)
            t, h, w = grids[gi]
            gi += 1
            lt, lh, lw = t, h // m, w // m
            text_len = ed - st
            st_idx = int(chunks[-1].max()) + 1 if chunks else 0
            chunks.append(torch.arange(text_len).view(1, -1).expand(3, -1) + st_idx)
            ti = torch.zeros(lt * lh * lw, dtype=torch.long)
            hi = torch.arange(lh).view(1, -1, 1).expand(lt, -1, lw).flatten()
            wi = torch.arange(lw).view(1, 1, -1).expand(lt, lh, -1).flatten()
            chunks.append(torch.stack([ti, hi, wi]) + text_len + st_idx)
            st = ed + lt * lh * lw
        if st < len(toks):
            st_idx = int(chunks[-1].max()) + 1 if chunks else 0
            chunks.append(torch.arange(len(toks) - st).view(1, -1).expand(3, -1) + st_idx)
        pos = torch.cat(chunks, dim=1).reshape(3, -1)
        out.append(pos)
        nxt.append(int(pos.max()) + 1)
    return out, nxt


@dataclass
class PromptPlan:
    B: int
    L_pad: int                       # padded prompt length of the caller's (B, L) input
    lens: List[int]                  # valid tokens per sample
    ids: torch.Tensor                # (T,) int64 packed global ids
    img_index: torch.Tensor          # (T,) int32: index into image_embeds or -1
    pos3: torch.Tensor               # (3, T) int32
    sample: torch.Tensor             # (T,) int32
    slot: torch.Tensor               # (T,) int32
    cu: torch.Tensor                 # (B+1,) int32
    last_idx: torch.Tensor           # (B,) int32 index of each sample's last token
    next_pos: List[int]
    rope_deltas: torch.Tensor        # (B,1) int64, 4.50 convention: max+1 - L_pad
    vrt_off: List[int]               # (B+1) prototype row offsets
    first_row: int = 0               # decode-session row of this batch's first sample (merged decode groups)
    shared: Optional["SharedPrompt"] = None   # generate(image_index=): the smaller token set the prompt pass computes (plan_prompt_shared)


def plan_prompt(cfg: PaDTConfig, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor],
                grid_thw: torch.Tensor, device, row0: int = 0, proto_row0: int = 0) -> PromptPlan:
    """``row0`` / ``proto_row0``: first decode-session row and first prototype-table row of this batch when several
    batches share one session (merged decode, modeling.generate_launch): KV rows and VRT ids are shifted accordingly."""
    ids_cpu = input_ids.detach().cpu()
    B, L = ids_cpu.shape
    am = attention_mask.detach().cpu() if attention_mask is not None else torch.ones_like(ids_cpu)
    grids = [[int(x) for x in r] for r in grid_thw.tolist()]
    if len(grids) != B:
        raise ValueError("one image per sample is required (padt.py:301 indexes the logit mask by image)")
    rows = [ids_cpu[b][am[b] == 1].tolist() for b in range(B)]
    n_img_tok = sum(r.count(cfg.image_token_id) for r in rows)
    merged = [g[0] * g[1] * g[2] // cfg.merge_unit for g in grids]
    if n_img_tok != sum(merged):
        raise ValueError(f"Image features and image tokens do not match: tokens: {n_img_tok}, features {sum(merged)}")
    pos, nxt = rope_index_packed(cfg, rows, grids)
    lens = [len(r) for r in rows]
    ids = torch.tensor([t for r in rows for t in r], dtype=torch.int64)
    if proto_row0:
        ids = torch.where(ids >= cfg.vocab_size, ids + proto_row0, ids)
    is_img = ids == cfg.image_token_id
    img_index = torch.where(is_img, torch.cumsum(is_img.to(torch.int64), 0) - 1, torch.full_like(ids, -1)).to(I32)
    cu = [0]
    for l in lens:
        cu.append(cu[-1] + l)
    sample = torch.cat([torch.full((l,), b + row0, dtype=I32) for b, l in enumerate(lens)])
    slot = torch.cat([torch.arange(l, dtype=I32) for l in lens])
    off = [0]
    for n in merged:
        off.append(off[-1] + n)
    return PromptPlan(
        B=B, L_pad=L, lens=lens, ids=ids.to(device), img_index=img_index.to(device),
        pos3=torch.cat(pos, dim=1).to(I32).contiguous().to(device), sample=sample.to(device), slot=slot.to(device),
        cu=torch.tensor(cu, dtype=I32, device=device), last_idx=torch.tensor([c - 1 for c in cu[1:]], dtype=I32, device=device),
        next_pos=nxt, rope_deltas=torch.tensor([[n - L] for n in nxt], dtype=torch.int64), vrt_off=off, first_row=row0)


@dataclass
class SharedPrompt:
    """The token set a prompt pass with ``image_index`` computes (plan_prompt_shared): every share group's prefix ONCE, then every
    sample's own tokens.  Segment s < G is the prefix of group s, segment G + b the own tokens of sample b."""
    n_images: int
    groups: List[tuple]              # (prefix length P, member samples) per share group, in order of the first member
    prefix_of: List[int]             # per sample: its group's index, or -1 (no shared prefix: every token is its own)
    ids: torch.Tensor                # (Ts,) int64 global ids
    img_index: torch.Tensor          # (Ts,) int32 row of the per-SAMPLE merged embeddings (a prefix reads its first member's), or -1
    pos3: torch.Tensor               # (3, Ts) int32: slices of the full rows' mRoPE positions
    dst_off: torch.Tensor            # (Ts+1,) int32 CSR offsets into the destination lists
    dst_sample: torch.Tensor         # session row whose K / V^T cache images get the token, or -1: a join row only
    dst_slot: torch.Tensor           # ... at this slot
    dst_row: torch.Tensor            # row of the attention's key / value join buffers
    n_join: int
    cu_q: torch.Tensor               # (G+B+1,) int32 query segments (the token set itself)
    cu_k: torch.Tensor               # (G+B+1,) int32 key segments of the join buffers: [prefix] / [group prefix | own tokens]
    max_q: int
    unshare: torch.Tensor            # (T,) int32: row of the token set behind each row of the unshared packed order (PromptPlan.ids)
    low_rows: torch.Tensor           # (sum merged per sample,) int32: the image's merged row behind each per-sample merged row
    patch_rows: torch.Tensor         # (sum patches per sample,) int32: the same for the patch-level rows (high_res, visual_pe)
    grid_x: torch.Tensor             # (B, 3) image_grid_thw[image_index]
    dst_host: tuple = ()             # host copies of (dst_sample, dst_slot, dst_row) for check_shared_destinations
    # generate(prefix=) (plan_prompt_prefix): no prefix segment is computed — the token set is the own tokens, and the handle's cached rows
    # are put where the shared pass would have fanned them out (ops.kv_prefix_fanout), its hidden rows behind the token set's
    prefix: Optional["PromptPrefix"] = None
    prefix_len: tuple = ()           # per sample: the length P of its image's cached prefix
    members: tuple = ()              # device int32 (mem_image, mem_row, mem_join): per sample its image, session row, first row of its key segment
    max_p: int = 0


@dataclass
class PromptPrefix:
    """What model.encode_prefix keeps of N images and the prompt rows in front of each query on them, for generate(prefix=) in later
    calls: the ViT outputs every consumer downstream reads and, per LLM layer, the roped K rows and V rows of the prefix tokens — what the
    join buffers of the shared prompt pass hold.  Image u's prefix has P = len(ids[u]) tokens, rows [off[u], off[u+1]) of ``hidden`` /
    ``k[layer]`` / ``v[layer]``.  The handle owns its tensors and belongs to no session; nothing in a generate call writes to it."""
    ids: List[List[int]]             # per image: the unpadded prefix ids, VRT ids in image-LOCAL numbering
    grid: torch.Tensor               # (N, 3) int64, host
    pos3: Optional[List[torch.Tensor]] = None      # per image (3, P) int32, host: mRoPE positions of the prefix
    next_pos: Optional[List[int]] = None           # ... and the position after it
    dtype: Optional[torch.dtype] = None            # the 16-bit operand type it was built with
    low: Optional[torch.Tensor] = None             # (sum merged, D) merged rows
    high: Optional[torch.Tensor] = None            # (sum patches, vh) fp32 patch-level rows
    pe: Optional[tuple] = None                     # (cos, sin) (sum patches, hd): visual PE
    proto: Optional[torch.Tensor] = None           # (sum merged, D) prototype rows
    hidden: Optional[torch.Tensor] = None          # (sum P, D) last-layer post-norm rows of the prefix tokens
    k: Optional[torch.Tensor] = None               # (layers, sum P, Hkv * hd) roped K rows
    v: Optional[torch.Tensor] = None               # (layers, sum P, Hkv * hd) V rows
    pre_off: Optional[torch.Tensor] = None         # (N + 1,) int32 on the device: ``off``
    ready: object = None                           # event after which the tensors may be read
    inputs: tuple = ()                             # (input_ids, attention_mask, pixel_values, image_grid_thw) it was built from
    twin: Optional["PromptPrefix"] = None          # the bf16 build of an fp16 handle, made once when a call needs it (operands="auto")

    @property
    def n_images(self) -> int:
        return len(self.ids)

    @property
    def lens(self) -> List[int]:
        return [len(r) for r in self.ids]

    @property
    def off(self) -> List[int]:
        o = [0]
        for r in self.ids:
            o.append(o[-1] + len(r))
        return o

    @property
    def nbytes(self) -> int:
        ts = [self.low, self.high, self.proto, self.hidden, self.k, self.v] + list(self.pe or ())
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def image_k(self, u: int) -> torch.Tensor:
        """[layer][P][Hkv * hd] roped K rows of image u's prefix (a view)."""
        return self.k[:, self.off[u]: self.off[u + 1]]

    def image_v(self, u: int) -> torch.Tensor:
        return self.v[:, self.off[u]: self.off[u + 1]]


def unpadded_rows(input_ids, attention_mask):
    ids_cpu = input_ids.detach().cpu()
    am = attention_mask.detach().cpu() if attention_mask is not None else torch.ones_like(ids_cpu)
    return [ids_cpu[b][am[b] == 1].tolist() for b in range(ids_cpu.shape[0])]


def plan_prefix_build(cfg: PaDTConfig, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], grid_thw: torch.Tensor,
                      device) -> PromptPlan:
    """The prompt pass model.encode_prefix runs: plan_prompt of the N prefix rows (row u = image u's prefix) with a token set whose every
    destination is a join row only (dst_sample = -1) — ops.llm_qkv_post_shared then leaves the roped K rows and V rows in the handle's
    layer slices, in packed row order, and touches no cache image."""
    rows = unpadded_rows(input_ids, attention_mask)
    grids = [[int(x) for x in r] for r in torch.as_tensor(grid_thw).tolist()]
    if len(grids) != len(rows):
        raise ValueError(f"encode_prefix takes one row per image: {len(rows)} rows, {len(grids)} images")
    for u, (r, g) in enumerate(zip(rows, grids)):
        n_tok, n_feat = r.count(cfg.image_token_id), g[0] * g[1] * g[2] // cfg.merge_unit
        if n_tok != n_feat:
            raise ValueError(f"encode_prefix: row {u} must contain the image tokens of image {u} completely: {n_tok} image tokens, "
                             f"{n_feat} features")
    plan = plan_prompt(cfg, input_ids, attention_mask, torch.tensor(grids, dtype=torch.long), device)
    T = sum(plan.lens)
    ar = torch.arange(T, dtype=I32)
    none = torch.full((T,), -1, dtype=I32)
    plan.shared = SharedPrompt(
        n_images=len(grids), groups=[], prefix_of=[-1] * len(rows), ids=plan.ids, img_index=plan.img_index, pos3=plan.pos3,
        dst_off=torch.arange(T + 1, dtype=I32).to(device), dst_sample=none.to(device), dst_slot=plan.slot, dst_row=ar.to(device), n_join=T,
        cu_q=plan.cu, cu_k=plan.cu, max_q=max(plan.lens), unshare=ar.to(device), low_rows=None, patch_rows=None,
        grid_x=torch.tensor(grids, dtype=torch.long), dst_host=(none, plan.slot.cpu(), ar))
    return plan


def check_prefix_rows(cfg: PaDTConfig, prefix: PromptPrefix, image_index, rows: List[List[int]]) -> List[int]:
    """generate(prefix=): → the index as a list, after the host-side validation of the rows against the handle (ValueError)."""
    B, N = len(rows), prefix.n_images
    if image_index is None:
        if B != N:
            raise ValueError(f"generate(prefix=...) without image_index needs one row per image of the prefix: {B} rows, {N} images")
        idx = list(range(B))
    else:
        idx = [int(i) for i in (image_index.detach().cpu().reshape(-1).tolist() if isinstance(image_index, torch.Tensor) else list(image_index))]
    if len(idx) != B:
        raise ValueError(f"image_index has {len(idx)} entries for a batch of {B} samples")
    for b, u in enumerate(idx):
        if not 0 <= u < N:
            raise ValueError(f"image_index[{b}] = {u} is outside [0, {N}): the prefix holds {N} images")
    merged = [int(g[0] * g[1] * g[2]) // cfg.merge_unit for g in prefix.grid.tolist()]
    off = 0
    for b, u in enumerate(idx):                                   # compared in image-local VRT numbering: the row's ids count the batch's patches
        pre, V = prefix.ids[u], cfg.vocab_size
        r = [t - off if t >= V else t for t in rows[b]]
        n = 0
        while n < min(len(r), len(pre)) and r[n] == pre[n]:
            n += 1
        if n < min(len(r), len(pre)):
            raise ValueError(f"generate(prefix=...): row {b} does not start with the prefix of image {u}: first difference at position {n} "
                             f"(id {r[n]}, the prefix has {pre[n]})")
        if len(r) <= len(pre):
            raise ValueError(f"generate(prefix=...): row {b} has no token of its own: it ends at position {len(r)}, the prefix of image {u} "
                             f"has {len(pre)} tokens")
        off += merged[u]
    return idx


def plan_prompt_prefix(cfg: PaDTConfig, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], prefix: PromptPrefix,
                       image_index, device, row0: int = 0, proto_row0: int = 0) -> PromptPlan:
    """plan_prompt_shared for rows whose prefixes are CACHED (generate(prefix=)): → the PromptPlan of the expanded inputs with ``shared``
    describing the token set the pass computes — every sample's own tokens (those behind its image's prefix) and nothing else.  Sample b's
    key segment is [prefix of its image | own tokens]; the prefix part of it, and slots [0, P) of its cache images, are filled from the
    handle (``members``, ops.kv_prefix_fanout), so no destination of the token set names them.  ``unshare`` reads the prefix rows of the
    unshared packed order behind the token set's rows: row Ts + off[u] + j is row j of image u's cached hidden rows."""
    rows = unpadded_rows(input_ids, attention_mask)
    B = len(rows)
    idx = check_prefix_rows(cfg, prefix, image_index, rows)
    grids = [[int(x) for x in r] for r in prefix.grid.tolist()]
    base = plan_prompt(cfg, input_ids, attention_mask, torch.tensor([grids[u] for u in idx], dtype=torch.long), "cpu", row0=row0,
                       proto_row0=proto_row0)
    lens, cu = base.lens, base.cu.tolist()
    P, p_off = [prefix.lens[u] for u in idx], prefix.off
    merged = [g[0] * g[1] * g[2] // cfg.merge_unit for g in grids]
    low_off, patch_off = [0], [0]
    for g, n in zip(grids, merged):
        low_off.append(low_off[-1] + n)
        patch_off.append(patch_off[-1] + g[0] * g[1] * g[2])
    low_rows = torch.cat([torch.arange(low_off[u], low_off[u + 1], dtype=I32) for u in idx])
    patch_rows = torch.cat([torch.arange(patch_off[u], patch_off[u + 1], dtype=I32) for u in idx])
    own = [lens[b] - P[b] for b in range(B)]
    cu_q, cu_k = [0], [0]
    for b in range(B):
        cu_q.append(cu_q[-1] + own[b])
        cu_k.append(cu_k[-1] + lens[b])
    Ts = cu_q[-1]
    src = torch.cat([torch.arange(cu[b] + P[b], cu[b] + lens[b], dtype=torch.int64) for b in range(B)])
    dst_off, d_sample, d_slot, d_row = [0], [], [], []
    unshare = torch.empty((cu[-1],), dtype=I32)
    for b in range(B):
        for j in range(own[b]):
            d_sample.append(row0 + b), d_slot.append(P[b] + j), d_row.append(cu_k[b] + P[b] + j)
            dst_off.append(len(d_sample))
        unshare[cu[b]: cu[b] + P[b]] = torch.arange(Ts + p_off[idx[b]], Ts + p_off[idx[b]] + P[b], dtype=I32)
        unshare[cu[b] + P[b]: cu[b] + lens[b]] = torch.arange(cu_q[b], cu_q[b + 1], dtype=I32)
    t32 = lambda v: torch.tensor(v, dtype=I32).to(device)
    base.shared = SharedPrompt(
        n_images=len(grids), groups=[], prefix_of=[-1] * B, ids=base.ids[src].to(device), img_index=base.img_index[src].to(device),
        pos3=base.pos3[:, src].contiguous().to(device), dst_off=t32(dst_off), dst_sample=t32(d_sample), dst_slot=t32(d_slot), dst_row=t32(d_row),
        n_join=cu_k[-1], cu_q=t32(cu_q), cu_k=t32(cu_k), max_q=max(own), unshare=unshare.to(device), low_rows=low_rows.to(device),
        patch_rows=patch_rows.to(device), grid_x=torch.tensor([grids[u] for u in idx], dtype=torch.long),
        dst_host=tuple(torch.tensor(v, dtype=I32) for v in (d_sample, d_slot, d_row)), prefix=prefix, prefix_len=tuple(P),
        members=(t32(idx), t32([row0 + b for b in range(B)]), t32(cu_k[:-1])), max_p=max(P))
    for f in ("ids", "img_index", "pos3", "sample", "slot", "cu", "last_idx"):
        setattr(base, f, getattr(base, f).to(device))
    return base


def check_image_index(cfg: PaDTConfig, image_index, B: int, rows: List[List[int]], grids: List[List[int]]) -> List[int]:
    """generate(image_index=): → the index as a list, after the host-side validation of the argument (ValueError)."""
    idx = [int(i) for i in (image_index.detach().cpu().reshape(-1).tolist() if isinstance(image_index, torch.Tensor) else list(image_index))]
    N = len(grids)
    if len(idx) != B:
        raise ValueError(f"image_index has {len(idx)} entries for a batch of {B} samples")
    for b, u in enumerate(idx):
        if not 0 <= u < N:
            raise ValueError(f"image_index[{b}] = {u} is outside [0, {N}): pixel_values / image_grid_thw hold {N} images")
    unused = sorted(set(range(N)) - set(idx))
    if unused:
        raise ValueError(f"image_index uses no sample for image(s) {unused}: every image of pixel_values must belong to a sample")
    for b, u in enumerate(idx):
        n_tok, n_feat = rows[b].count(cfg.image_token_id), grids[u][0] * grids[u][1] * grids[u][2] // cfg.merge_unit
        if n_tok != n_feat:
            raise ValueError(f"Image features and image tokens do not match: tokens: {n_tok}, features {n_feat} (sample {b}, image {u})")
    return idx


def plan_prompt_shared(cfg: PaDTConfig, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], grid_thw: torch.Tensor,
                       image_index, device, row0: int = 0, proto_row0: int = 0) -> PromptPlan:
    """plan_prompt for B samples over N <= B images (sample b uses image image_index[b]): → the PromptPlan of the EXPANDED inputs
    (image_grid_thw[image_index], one image per sample — lens, cu, last_idx, positions, VRT ranges are what every consumer downstream of
    the prompt pass reads) with ``shared`` set to the smaller token set the pass computes.

    Share group: the samples of one image whose unpadded rows agree up to and including the last image token.  Its prefix length is
    P = min(longest common prefix of the rows, shortest row - 1) — every sample keeps a token of its own, its last hidden row is needed.
    One member, or a P that does not cover the image tokens: no prefix.  The prompt is causal, so the hidden rows and K / V rows of a
    prefix token are the same in every member's full row: they are computed once and fanned out (ops.llm_qkv_post_shared)."""
    ids_cpu = input_ids.detach().cpu()
    B, L = ids_cpu.shape
    am = attention_mask.detach().cpu() if attention_mask is not None else torch.ones_like(ids_cpu)
    grids = [[int(x) for x in r] for r in torch.as_tensor(grid_thw).tolist()]
    rows = [ids_cpu[b][am[b] == 1].tolist() for b in range(B)]
    idx = check_image_index(cfg, image_index, B, rows, grids)
    base = plan_prompt(cfg, input_ids, attention_mask, torch.tensor([grids[u] for u in idx], dtype=torch.long), "cpu", row0=row0,
                       proto_row0=proto_row0)
    lens, cu = base.lens, base.cu.tolist()
    # ---- share groups
    by_key = {}
    for b, r in enumerate(rows):
        last_img = len(r) - 1 - r[::-1].index(cfg.image_token_id)
        by_key.setdefault((idx[b], tuple(r[: last_img + 1])), []).append(b)
    groups, prefix_of = [], [-1] * B
    for (u, key), members in by_key.items():
        if len(members) < 2:
            continue
        P = min(lens[b] for b in members) - 1
        first = rows[members[0]]
        for b in members[1:]:
            r, n = rows[b], 0
            while n < P and r[n] == first[n]:
                n += 1
            P = n
        if P < len(key):                                         # by definition the GROUP has no prefix then (a member's row ends at the image:
            continue                                             # shortest row - 1 stops inside it) — its other members lose theirs too
        for b in members:
            prefix_of[b] = len(groups)
        groups.append((P, members))
    # ---- unique-image row tables: merged rows (embeddings, prototypes) and patch rows (high_res, visual_pe) per sample
    merged = [g[0] * g[1] * g[2] // cfg.merge_unit for g in grids]
    low_off, patch_off = [0], [0]
    for g, n in zip(grids, merged):
        low_off.append(low_off[-1] + n)
        patch_off.append(patch_off[-1] + g[0] * g[1] * g[2])
    low_rows = torch.cat([torch.arange(low_off[u], low_off[u + 1], dtype=I32) for u in idx])
    patch_rows = torch.cat([torch.arange(patch_off[u], patch_off[u + 1], dtype=I32) for u in idx])
    # ---- the token set: (sample whose full row the token is read from, first position, count) per segment
    segs = [(members[0], 0, P) for P, members in groups]
    segs += [(b, groups[prefix_of[b]][0] if prefix_of[b] >= 0 else 0, None) for b in range(B)]
    segs = [(b, a, (lens[b] - a) if n is None else n) for b, a, n in segs]
    G = len(groups)
    cu_q = [0]
    for _, _, n in segs:
        cu_q.append(cu_q[-1] + n)
    cu_k = [0]
    for s, (b, a, n) in enumerate(segs):
        cu_k.append(cu_k[-1] + (n if s < G else a + n))
    src = torch.cat([torch.arange(cu[b] + a, cu[b] + a + n, dtype=torch.int64) for b, a, n in segs])     # rows of the unshared packed order
    ids_s, pos_s, img_s = base.ids[src], base.pos3[:, src].contiguous(), base.img_index[src]
    # ---- destinations and the rows of the unshared order
    dst_off, d_sample, d_slot, d_row = [0], [], [], []
    unshare = torch.empty((cu[-1],), dtype=I32)
    for s, (P, members) in enumerate(groups):
        for j in range(P):
            d_sample.append(-1), d_slot.append(j), d_row.append(cu_k[s] + j)           # the prefix's own key segment
            for b in members:
                d_sample.append(row0 + b), d_slot.append(j), d_row.append(cu_k[G + b] + j)
            dst_off.append(len(d_sample))
        for b in members:
            unshare[cu[b]: cu[b] + P] = torch.arange(cu_q[s], cu_q[s] + P, dtype=I32)
    for b in range(B):
        _, a, n = segs[G + b]
        for j in range(n):
            d_sample.append(row0 + b), d_slot.append(a + j), d_row.append(cu_k[G + b] + a + j)
            dst_off.append(len(d_sample))
        unshare[cu[b] + a: cu[b] + a + n] = torch.arange(cu_q[G + b], cu_q[G + b] + n, dtype=I32)
    t32 = lambda v: torch.tensor(v, dtype=I32).to(device)
    base.shared = SharedPrompt(
        n_images=len(grids), groups=groups, prefix_of=prefix_of, ids=ids_s.to(device), img_index=img_s.to(device), pos3=pos_s.to(device),
        dst_off=t32(dst_off), dst_sample=t32(d_sample), dst_slot=t32(d_slot), dst_row=t32(d_row), n_join=cu_k[-1], cu_q=t32(cu_q),
        cu_k=t32(cu_k), max_q=max(n for _, _, n in segs), unshare=unshare.to(device), low_rows=low_rows.to(device),
        patch_rows=patch_rows.to(device), grid_x=torch.tensor([grids[u] for u in idx], dtype=torch.long), dst_host=tuple(torch.tensor(v, dtype=I32) for v in (d_sample, d_slot, d_row)))
    for f in ("ids", "img_index", "pos3", "sample", "slot", "cu", "last_idx"):
        setattr(base, f, getattr(base, f).to(device))
    return base


def check_shared_destinations(sh: SharedPrompt, n_rows: int, s_max: int):
    """Host check of a shared plan against the session it is about to write: every cache destination inside [0, n_rows) x [0, s_max), no
    (row, slot) written twice, every join row inside the join buffers."""
    sample, slot, row = sh.dst_host
    if bool(((row < 0) | (row >= sh.n_join)).any()):
        raise ValueError("shared prompt plan: a join row is outside the join buffers")
    keep = sample >= 0
    sample, slot = sample[keep].long(), slot[keep].long()
    if bool(((sample >= n_rows) | (slot < 0) | (slot >= s_max)).any()):
        raise ValueError(f"shared prompt plan: a KV destination is outside the session's {n_rows} rows x {s_max} slots")
    if torch.unique(sample * s_max + slot).numel() != sample.numel():
        raise ValueError("shared prompt plan: a (row, slot) of the KV cache is written twice")


# ------------------------------------------------------------------------------------------------ decode session
MODE = {"f": 0, None: 0, "t": 1, "v": 2, "e": 3}


def _call_hooks(hooks, input_ids, scores, chain: bool):
    """HF's LogitsProcessorList / StoppingCriteriaList are callables over (input_ids, scores); a plain list / tuple of callables is walked here:
    processors chain (each sees its predecessor's scores), criteria are OR-ed."""
    if callable(hooks):
        return hooks(input_ids, scores)
    out = scores if chain else None
    for h in hooks:
        if chain:
            out = h(input_ids, out)
        else:
            r = h(input_ids, scores)
            out = r if out is None else (out | r)
    return out


class DecodeSession:
    """Persistent device state for one (batch, S_max, max prototypes, T_max) shape: KV caches, per-step state, the
    prototype table and the captured decode-step hipGraph.  Pointers are stable across generate() calls so the graph
    is captured once."""

    def __init__(self, cfg: PaDTConfig, W, B: int, s_max: int, np_max: int, t_max: int, device):
        self.cfg, self.W, self.B, self.s_max, self.np_max, self.t_max = cfg, W, B, s_max, np_max, t_max
        D, hd, Hkv, nl = cfg.hidden_size, cfg.head_dim, cfg.num_key_value_heads, cfg.num_hidden_layers
        bf = W.op16                                         # 16-bit operand type of the model (fp16 by default, bf16: weights.prepare_weights)
        z = lambda *s, dt=bf: torch.zeros(*s, device=device, dtype=dt)
        # KV caches, one pair per layer.  head_dim 128 (PaDT_Pro_3B / 7B): the FRAGMENT-PACKED images of padt_decode_attn_rope (K
        # [S/16][D/32][64 lanes][8], V^T [D/16][S/32][64 lanes][8]: 1 KiB contiguous per wave-wide load) read by the one-launch decode
        # attention and written in place by the prompt pass (llm_qkv_post) and the decode step's append; otherwise row-major K / transposed V
        # with the two-launch split attention.
        self.cache_packed = hd == 128 and cfg.num_attention_heads // Hkv <= 16
        self.kc = [z(B, Hkv, s_max, hd) for _ in range(nl)]
        self.vtc = [z(B, Hkv, hd, s_max) for _ in range(nl)]
        self.proto = z(np_max, D)
        self.vrt_off = z(B + 1, dt=I32)
        self.batch_row0 = z(B, dt=I32)     # per row: the first row of its batch in a merged decode group (the sampling kernels' generator key)
        self.mode_table = z(t_max + 1, dt=I32)
        self.step = z(1, dt=I32)
        self.unfinished = z(B, dt=I32)
        self.tokens = z(B, t_max, dt=torch.int64)
        self.cur_tok = z(B, dt=torch.int64)
        self.slot = z(B, dt=I32)
        self.lens = z(B, dt=I32)
        self.pos3 = z(3, B, dt=I32)
        self.hidden_buf = z(t_max, B, D)
        self.nblk = ops.vrt_head_nblk(cfg.vocab_size, np_max)
        self.part_val = z(self.nblk * B, dt=torch.float32)
        self.part_idx = z(self.nblk * B, dt=I32)
        self.attn_ws = ops.new_decode_workspace(B, Hkv, hd, s_max, device)
        # down_proj has only D/16 column blocks (128 for D = 2048): split K over 2 blocks each to occupy every CU
        self.down_split, self.o_split = 2, 1                # (o with split 2: 7.6 → 10.9 us at 64 rows, profiles/r03_decode_experiments.md §7)
        self.splitk_ws = ops.new_splitk_workspace(cfg.hidden_size, max(self.down_split, self.o_split, 1), device)
        half = hd // 2
        self.inv_freq = (1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))).to(device)
        assert self.inv_freq.numel() == half
        # decode-step activations (static addresses → graph-replayable)
        # x / att / h are in the 16-row fragment-packed activation layout (include/padt_hip.h): every projection reads its
        # input fragments as 1 KiB contiguous wave loads; x_rm is the row-major copy the step's token embeddings land in
        I = W.llm_ipad
        B16 = (B + 15) // 16 * 16
        self.x = z(B16, D)
        self.x_rm = z(B, D)
        self.x32 = z(B, D, dt=torch.float32)     # fp32 residual stream of the decode step (x is its packed 16-bit mirror)
        self.n = z(B, D)
        self.qkv = z(B, (cfg.num_attention_heads + 2 * Hkv) * hd)
        self.q = z(B, cfg.num_attention_heads * hd)
        self.att = z(B16, cfg.num_attention_heads * hd)
        self.h = z(B16, I)
        self.hn = z(B, D)
        self.hn_first = z(B, D)          # last prompt token's post-norm hidden state per row (first-token selection)
        self.hn_pk = z(B16, D)           # packed copy of the head's input rows
        # generation-config slots (device memory, so the captured graph does not bake them in) + per-row seen-token bitmap
        self.gen_cfg = ops.gen_cfg_tensor(1.0, (), device)
        self.seen = z(B, (cfg.vocab_size + np_max + 31) // 32, dt=I32)
        # HF's pure-ban processors (no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens): the packed rule table, each
        # row's prompt ids as the caller passed them (padding included: what HF's processors see) and the per-step ban bitmap ops.gen_rules
        # rebuilds from them and `tokens` — all device memory at fixed addresses, read by the captured step
        self.rules = z(ops.GEN_RULES_INTS, dt=I32)
        self.hist = z(B, s_max, dt=I32)
        self.hist_len = z(B, dt=I32)
        self.ban = z(B, self.seen.shape[1], dt=I32)
        self.err = z(1, dt=I32)
        self.nf = z(B, dt=I32)           # per row: a decode step produced a non-finite hidden row (fp16 operand overflow; ops.check_finite)
        self.nf_batch = z(B, dt=I32)     # per batch of the decode group (slot k): ViT rows / prototypes / prompt-pass rows not finite
        # read_summary's ONE read-back per chunk (ops.collect_summary): [err, any unfinished, nf rows, nf batches, first EOS step per row]
        self.summary = z(2 + 3 * B, dt=I32)
        self.summary_host = torch.zeros(2 + 3 * B, dtype=I32).pin_memory() if torch.device(device).type == "cuda" else torch.zeros(2 + 3 * B, dtype=I32)
        # what this generate's step launches and keeps (generation.StepMode, set by begin()); the buffers below are allocated on first use
        self.mode = StepMode()
        self.eos_ids = (int(cfg.eos_token_id),)   # the ids that finish a row in this generate: the config's and the resolved options' (begin())
        self.scores = None               # mode.keep_scores (output_scores=True): every step's masked fp32 logit rows [t_max][B][W]
        self.raw_scores = None           # mode.keep_logits (output_logits=True under sampling): the rows before the warpers [t_max][B][W]
        self.part_sum = None             # mode.token_logprobs: the head's per-block Σ exp(logit - block max) [nblk][B] (fused path) ...
        self.logprobs = None             # ... and log p of every selected token [B][t_max], no logit row kept
        self.top_idx = self.top_val = None   # mode.top_k (top_logprobs=k): the k best columns of every step's score row [B][t_max][k] ...
        self.top_flat = None             # ... views of ONE flat pair sized for k = 32
        self.p_cap = 0                   # mode.patches (output_patch_logprobs=True): every sample's own patch columns in `patch_lp` [B][t_max][p_cap]
        self.patch_lp = None
        self.topk_ws = None              # padt_topk_logprob_rows_f32's chunk workspace, sized for k = 32
        self.forced = None               # mode.forced (generate(forced_tokens=)): [B][t_max] int32 table columns in session numbering, -1 = free ...
        self.probe_val = None            # ... and the probe head's processed logit of each row's forced column [B]
        self.atab = None                 # mode.automaton (generate(token_automaton=)): the packed table, ops.TOKEN_AUTOMATON_INTS int32 (fixed size) ...
        self.astate = None               # ... each row's (state, valid_for_step) [B][2] ...
        self.aban = None                 # ... and the bitmap padt_token_automaton writes for the head (with rules: its union with `ban`) [B][words]
        self.bias = None                 # mode.bias (generate(logit_bias=, patch_bias=)): fp32 [V + np_max] added to the raw logit of its column ...
        self.decay = None                # ... and exponential_decay_length_penalty's a[t] fp32 [t_max], read at the device step counter (generation.decay_table)
        self.stab = None                 # mode.stop (generate(stop_sequences=, min_tokens=, max_tokens=)): the packed sequences, ops.STOP_RULES_INTS int32 (fixed size) ...
        self.min_tok = self.max_tok = None       # ... each row's minimum and budget [B] ...
        self.finish_step = self.finish_reason = self.stop_index = None      # ... what padt_stop_match records per row [B] (-1 / 0 / -1: no finish yet) ...
        self.sban = None                 # ... the bitmap padt_stop_ban writes for the head (the rules' / the automaton's plus the EOS ids below min_tokens) [B][words] ...
        self.summary_stop = self.summary_stop_host = None      # ... and read_summary's read-back with the three finish arrays behind it
        self.cnt_text = None             # mode.counts (generate(frequency_penalty=, presence_penalty=, patch_suppression=)): how often each row generated a text column, uint16 [B][V padded to 4] ...
        self.cnt_patch = self.near = None        # ... how often a patch column was generated by its row, and the completed-run VRT tokens around each patch, uint16 [np_max] ...
        self.cpen = None                 # ... each row's f, p and suppression penalty fp32 [3][B] (0: off) ...
        self.cgrid = self.cradius = None         # ... and its merged patch grid (hp, wp) [B][2] and radius [B] (-1: no suppression), int32: what padt_count_update reads
        self.beam = None                 # mode.beam (generate(beam_width=K)): this generate's ops.BeamState — live scores, finished store, step records — over the buffers below ...
        for nm in ops.BEAM_STATE_F32 + ops.BEAM_STATE_I32 + ("flags", "beam_tok", "beam_parent", "beam_lp", "perm", "p0", "cfg", "len_table"):
            setattr(self, "beam_" + nm, None)      # ... flat, allocated on first use, one set for every width
        self.beam_rep = None             # ... the log-probs a step reports for its candidates (mode.token_logprobs: padt_beam_cand_lp) [B][32] ...
        self.beam_kv = None              # ... and the device table of the layers' cache image pointers padt_beam_reorder_kv reads, built once
        self.rope_cs = z(B, hd // 2, 2, dt=torch.float32)
        self.n_qkv = (cfg.num_attention_heads + 2 * Hkv) * hd
        self.graphs = {}                 # captured decode-step graph per mode (different kernel sequences and output buffers)
        self.logits = None               # fp32 [B][V + np_max] rows for the sampling kernel, allocated on first use
        self.np_cur = np_max
        self.step_fn = None              # precision="reference": the eager split-precision decode step (reference.ReferencePath.step) instead of step_kernels
        self.hooks = None                # caller-supplied logits_processor / stopping_criteria of this generate (modeling.generate): the HOOKED, eager loop
        self.hid32 = None                # ... and its fp32 per-step hidden rows [t_max][B][D]

    # one decode step, all on the current stream (eager or under capture)
    def step_kernels(self):
        cfg, W = self.cfg, self.W
        Hq, Hkv, hd, D = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.hidden_size
        B = self.B
        ops.embed_tokens(self.cur_tok, None, W["llm.embed"], self.proto, None, out=self.x_rm, err_flag=self.err)
        sc = ops.stream_scale(W.op16)
        eps_n = W.eps_m(cfg.rms_norm_eps)                                    # the fused norms read the (scaled) stream mirror
        ops.cast_x16_f32(self.x_rm, out=self.x32)
        if sc != 1.0:                                                         # first mirror of the step's stream: X(scale * x32)
            ops.cast_f32_x16(self.x32, out=self.x_rm, scale=sc)
        ops.pack_rows(self.x_rm, self.x, B, to_packed=True)
        ops.rope_table(self.pos3, self.inv_freq, self.rope_cs, hd, cfg.mrope_section)
        fp8 = W.llm_weights == "fp8"                              # fp8 weight images (+ per-row scales): half the bytes per step
        wk = ".wq" if fp8 else ".wp"
        ws = (lambda m: W[m + ".ws"]) if fp8 else (lambda m: None)
        we = lambda m: None
        if W.llm_weights == "fp4":                                # MXFP4 images (+ block exponents): the same launches over 4.25 bits per weight
            wk, we = ".w4", (lambda m: W[m + ".we"])
        for i in range(cfg.num_hidden_layers):
            p = f"llm.{i}."
            # 6 launches per layer: [norm+qkv] [rope+append+split attention] [merge] [o+resid] [norm+gate/up+SwiGLU] [down+resid]
            ops.gemm_packed(self.x, W[p + "qkv" + wk], self.n_qkv, W[p + "qkv.b"], out=self.qkv, norm_eps=eps_n, a_packed=True, rows=B,
                            scales=ws(p + "qkv"), exps=we(p + "qkv"))
            ops.decode_attn_rope(self.qkv, self.rope_cs, self.slot, self.kc[i], self.vtc[i], self.att, self.attn_ws, Hq, Hkv,
                                 hd, self.s_max, self.s_max, out_packed=True, cache_packed=self.cache_packed)
            ops.gemm_packed_resid32(self.att, W[p + "o" + wk], D, self.x32, self.x, scales=ws(p + "o"), exps=we(p + "o"), split_k=self.o_split,
                                    workspace=self.splitk_ws, rows=B)
            ops.gemm_packed(self.x, W[p + "gu" + wk], 2 * W.llm_ipad, out=self.h, epilogue=ops.EPI_SWIGLU, norm_eps=eps_n,
                            a_packed=True, c_packed=True, rows=B, scales=ws(p + "gu"), exps=we(p + "gu"))
            ops.gemm_packed_resid32(self.h, W[p + "down" + wk], D, self.x32, self.x, scales=ws(p + "down"), exps=we(p + "down"),
                                    split_k=self.down_split, workspace=self.splitk_ws, rows=B)
        ops.rmsnorm_f32(self.x32, W["llm.norm"], out=self.hn, eps=cfg.rms_norm_eps)
        ops.check_finite(self.hn, self.nf, rows_per_flag=1, rows=B)      # sticky per-row flag, read once per generate (modeling.generate_collect)
        self.head_and_select(self.hn, advance=True)

    def _own(self, name: str, shape, dtype, fill=0, reset: bool = True):
        """The buffer `name` of an option that is on: allocated on first use (nothing is held for an option that is off) holding `fill`, and
        at that address ever after — the captured graphs hold it.  Every later generate that asks starts from `fill` again; reset=False:
        what a kernel or begin() writes in full before anything reads it keeps what it holds."""
        t = getattr(self, name)
        if t is None:
            dev, shape = self.part_val.device, (shape,) if isinstance(shape, int) else tuple(shape)
            t = torch.zeros(shape, device=dev, dtype=dtype) if fill == 0 else torch.full(shape, fill, device=dev, dtype=dtype)
            setattr(self, name, t)
        elif reset:
            t.zero_() if fill == 0 else t.fill_(fill)
        return t

    def begin(self, opts: GenOptions, p_max: int = 0, processors: bool = False, step_fn=None, automaton=None, n_steps=None, schedule=None):
        """Start of a generate — of a new decode group — with these options (p_max: the largest patch count of one sample; n_steps: the call's
        max_new_tokens, None = the session's t_max — the mode table and the decay table are filled up to there; processors: the caller's
        logits_processor runs in the hooked loop; step_fn: precision="reference"'s step; schedule: the forced token class per step, None =
        every step free).  Sets the gen_cfg slots and the rule table the captured step reads and the step mode, puts every row into the
        neutral state — finished, empty, no VRT range — that the group's batches overwrite for their own rows (add_batch), and sets the
        buffers of the options that are on (_own) to their finished-row values (0 / -1 / -inf).
        top_logprobs uses the leading B * t_max * k elements of ONE flat (ids, values) pair sized for k = 32 as [B][t_max][k], so a captured
        step keeps its addresses and memory does not grow with the k values asked; the patch buffer grows, and the graphs captured over the
        smaller one go with it."""
        dev = self.part_val.device
        B, t_max, F32 = self.B, self.t_max, torch.float32
        T = t_max if n_steps is None else int(n_steps)
        self.gen_cfg.copy_(opts.gen_cfg().to(dev, non_blocking=True))
        self.mode, self.step_fn, self.hooks = opts.step_mode(processors, step_fn is not None), step_fn, None
        self.eos_ids = tuple(dict.fromkeys((int(self.cfg.eos_token_id),) + tuple(opts.eos_ids)))      # every id that finishes a row on the device
        if opts.repetition_penalty != 1.0:
            self.seen.zero_()
        # neutral state for every row; the batches overwrite their own rows (unused rows stay finished / empty)
        st = torch.zeros(T + 1, dtype=I32)
        if schedule is not None:
            for i, mm in enumerate(schedule[:T]):
                st[i] = MODE[mm]
        self.mode_table[: T + 1].copy_(st.to(dev, non_blocking=True))
        for t in (self.step, self.err, self.unfinished, self.slot, self.pos3, self.vrt_off):
            t.zero_()
        self.lens.fill_(1)                                       # slot + 1, as for a filled row (add_batch): the keys visible to the next token of an empty prompt
        self.cur_tok.fill_(self.cfg.pad_token_id)
        if opts.sampling is not None:
            self.batch_row0.zero_()                              # read by the sampling kernels alone
        if step_fn is not None and (self.hid32 is None or self.hid32.shape[0] < T):      # reference precision keeps fp32 hidden rows per step
            self.hid32 = torch.zeros((t_max, B, self.cfg.hidden_size), device=dev, dtype=F32)
        if opts.token_logprobs:
            self._own("part_sum", self.nblk * B, F32)
            self._own("logprobs", (B, t_max), F32)
        self.top_idx = self.top_val = None
        if (opts.want_rows or opts.beam is not None) and self.topk_ws is None:
            nbytes = ops.topk_rows_workspace(self.cfg.vocab_size + self.np_max, ops.TOPK_ROWS_MAX_K, B)
            self.topk_ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        k_top = opts.top_logprobs or opts.beam_keep              # a beam step reads its rows' `keep` best candidates from the same pair
        if k_top:
            if self.top_flat is None:
                n = B * t_max * ops.TOPK_ROWS_MAX_K
                self.top_flat = (torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=F32))
            n = B * t_max * k_top
            self.top_idx, self.top_val = (f[:n].view(B, t_max, k_top) for f in self.top_flat)
            self.top_idx.fill_(-1)
            self.top_val.fill_(float("-inf"))
        if opts.patch_logprobs:
            if self.patch_lp is None or self.p_cap < p_max:
                self.graphs = {m: g for m, g in self.graphs.items() if not m.patches}      # their launches hold the old buffer's address
                self.p_cap, self.patch_lp = max(int(p_max), 1), None
            self._own("patch_lp", (B, t_max, self.p_cap), F32, float("-inf"))
        if opts.forced:                                          # every row free; each batch of the group fills its own rows (add_batch)
            self._own("forced", (B, t_max), I32, -1)
            self._own("probe_val", B, F32, reset=False)
        if opts.automaton is not None:                           # `automaton`: the generation.TokenAutomaton whose key the options carry
            tab = ops.token_automaton_tensor(automaton, key=None if automaton is not None else opts.automaton)
            self._own("atab", ops.TOKEN_AUTOMATON_INTS, I32, reset=False)[: tab.numel()].copy_(tab.to(dev, non_blocking=True))
            self._own("astate", (B, 2), I32, -1)                 # no row's state is valid: the first launch starts every row at the start state
            self._own("aban", self.ban.shape, I32, reset=False)
        if opts.score_bias:                                      # text columns and the decay now; each batch of the group adds its patch segment (add_batch)
            self._own("bias", self.cfg.vocab_size + self.np_max, F32)
            self._own("decay", t_max, F32, reset=False)
            if opts.logit_bias is not None:
                ids = torch.tensor([k for k, _ in opts.logit_bias], dtype=torch.long)
                val = torch.tensor([v for _, v in opts.logit_bias], dtype=torch.float32)
                self.bias.index_copy_(0, ids.to(dev), val.to(dev))
            self.decay.copy_(decay_table(opts.decay, self.t_max, n_steps).to(dev, non_blocking=True))
        if opts.stop:                                            # rows no batch of the group fills: min 0 (or the call's one value), budget t_max
            if self.summary_stop_host is None:
                host = torch.zeros(2 + 6 * B, dtype=I32)
                self.summary_stop_host = host.pin_memory() if torch.device(dev).type == "cuda" else host
            self._own("summary_stop", 2 + 6 * B, I32, reset=False)
            self._own("stab", ops.STOP_RULES_INTS, I32, reset=False).copy_(stop_table(opts.stop_sequences).to(dev, non_blocking=True))
            self._own("sban", self.ban.shape, I32, reset=False)
            self._own("min_tok", B, I32, opts.min_tokens or 0)
            self._own("max_tok", B, I32, t_max)
            self._own("finish_step", B, I32, -1)
            self._own("finish_reason", B, I32)
            self._own("stop_index", B, I32, -1)
        if opts.counts:                                          # nothing generated yet; rows no batch of the group fills: no penalty, no suppression
            self._own("cnt_text", (B, (self.cfg.vocab_size + 3) // 4 * 4), ops.COUNT_DTYPE)
            self._own("cnt_patch", self.np_max, ops.COUNT_DTYPE)
            self._own("near", self.np_max, ops.COUNT_DTYPE)
            self._own("cpen", (3, B), F32)
            self._own("cgrid", (B, 2), I32)
            self._own("cradius", B, I32, -1)
        if opts.rules is not None:
            self.rules.copy_(ops.gen_rules_tensor(key=opts.rules).to(dev, non_blocking=True))
            self.hist_len.zero_()                                # rows no batch of the group fills: an empty prompt
        self.beam = None
        if opts.beam is not None:
            # live scores [0, -inf, ...], empty stores, every sample open; the length table and the config in device memory, so that one
            # captured graph per width (and candidate count) serves every penalty, early-stopping mode and max_new_tokens
            K, _, penalty, early = opts.beam
            if not self.cache_packed:
                raise NotImplementedError("generate(beam_width=...) needs the packed KV caches (head_dim 128): padt_beam_reorder_kv moves their tiles")
            if B % K:
                raise ValueError(f"generate(beam_width={K}): the session holds {B} rows, not a multiple of the width")
            self.beam = ops.BeamState(B // K, K, t_max, dev, own=lambda nm, n, dt: self._own("beam_" + nm, n, dt, reset=False))
            self.beam.len_table.copy_(beam_len_table(penalty, t_max).to(dev, non_blocking=True))
            self.beam.cfg.copy_(ops.beam_cfg_tensor(K, opts.beam_keep, BEAM_EARLY[early], T - 1, early == "never" and penalty > 0.0).to(dev, non_blocking=True))
            if opts.token_logprobs:
                self._own("beam_rep", B * ops.TOPK_ROWS_MAX_K, F32, reset=False)
            if self.beam_kv is None:
                self.beam_kv = ops.beam_kv_table(self.kc, self.vtc)

    def add_batch(self, opts: GenOptions, row0: int, proto_row0: int, vrt_off, lens, next_pos, prompt_ids=None, forced=None, stop=None,
                  counts=None, count_grids=None, patch_bias=None):
        """The per-generate device state of one batch's rows, after begin(): rows [row0, row0 + B) for B = len(lens), whose prototype rows
        start at proto_row0 of the session's table.  All values are the batch's own and already validated (modeling._launch): vrt_off —
        its B + 1 patch offsets from 0; lens / next_pos — each row's prompt length and next rope position; prompt_ids (opts.reads_prompt) —
        the caller's padded (B, L) ids on the session's device; forced — its int table (B, n <= t_max), -1 = free; stop — dict(min_tokens=,
        max_tokens=) of per-row lists or None; counts — dict(frequency_penalty=, presence_penalty=, patch_suppression=) of per-row lists or
        None, with count_grids, each row's merged patch grid (hp, wp); patch_bias — per row a tensor over its patches or None.  VRT ids of
        the batch's own numbering (>= vocab) become session columns: + proto_row0."""
        cfg, dev = self.cfg, self.part_val.device
        B, V, n_proto = len(lens), cfg.vocab_size, vrt_off[-1]
        rows = slice(row0, row0 + B)
        up = lambda v, dt=I32: torch.tensor(v, dtype=dt).to(dev, non_blocking=True)
        shift = lambda ids: torch.where(ids >= V, ids + proto_row0, ids) if proto_row0 else ids
        self.vrt_off[row0: row0 + B + 1].copy_(up([proto_row0 + o for o in vrt_off]))
        if row0 + B + 1 < self.vrt_off.numel():
            self.vrt_off[row0 + B + 1:].fill_(proto_row0 + n_proto)     # rows not (yet) in use: empty VRT range
        if opts.sampling is not None:
            self.batch_row0[rows].fill_(row0)
        self.unfinished[rows].fill_(1)
        lens_t = torch.tensor(lens, dtype=I32)
        self.slot[rows].copy_(lens_t.to(dev, non_blocking=True))        # next append index
        self.lens[rows].copy_((lens_t + 1).to(dev, non_blocking=True))  # keys visible to the next token
        self.pos3[:, rows].copy_(up([next_pos] * 3))
        if opts.reads_prompt:
            ids_full = shift(prompt_ids)                          # HF's logits processors see the caller's full (B, L) input_ids, padding included
        if opts.repetition_penalty != 1.0:
            rws = (torch.arange(B, device=dev, dtype=I32) + row0)[:, None].expand(B, ids_full.shape[1]).contiguous()
            ops.seen_init(ids_full.reshape(-1).contiguous(), rws.reshape(-1), self.seen)
        if opts.rules is not None:
            self.hist[rows, : ids_full.shape[1]].copy_(ids_full)  # int64 → int32 (ids are table rows)
            self.hist_len[rows].fill_(ids_full.shape[1])
        if opts.beam is not None:                              # where the rows' generated slots begin: what padt_beam_reorder_kv moves
            self.beam.p0[rows].copy_(lens_t.to(dev, non_blocking=True))
        if forced is not None:
            # this batch's rows of the session's table, in session numbering like the prompt history; the steps past n stay free (-1: begin())
            self.forced[rows, : forced.shape[1]].copy_(shift(forced).to(dev, non_blocking=True))
        if opts.stop:
            # this batch's rows of the session's minima and budgets (begin() set every row to the call's one minimum and to the budget of a
            # row no batch fills): its own lists, or no budget at all — such a row ends on EOS, a stop sequence or the call's max_new_tokens
            lim = stop or {}
            if lim.get("min_tokens") is not None:
                self.min_tok[rows].copy_(up(lim["min_tokens"]))
            if lim.get("max_tokens") is not None:
                self.max_tok[rows].copy_(up(lim["max_tokens"]))
            else:
                self.max_tok[rows].fill_(NO_BUDGET)
        if opts.counts:
            # this batch's rows of the session's penalties, grids and radii (begin() zeroed the tables and switched every row off)
            cv = counts or {}
            supp = cv.get("patch_suppression") or [None] * B
            self.cpen[:, rows].copy_(up([cv.get("frequency_penalty") or [0.0] * B, cv.get("presence_penalty") or [0.0] * B,
                                         [0.0 if e is None else e[1] for e in supp]], torch.float32))
            self.cgrid[rows].copy_(up(count_grids))
            self.cradius[rows].copy_(up([-1 if e is None else e[0] for e in supp]))
        if patch_bias is not None:
            # this batch's segment of the session's bias vector: its own prototype rows (begin() zero-filled the vector; a row without an entry adds 0)
            seg = torch.zeros(n_proto, dtype=torch.float32)
            for b, pb in enumerate(patch_bias):
                if pb is not None:
                    seg[vrt_off[b]: vrt_off[b + 1]] = pb.reshape(-1)
            c0 = V + proto_row0
            self.bias[c0: c0 + n_proto].copy_(seg.to(dev, non_blocking=True))

    def read_summary(self, done: int, n_batches: int) -> dict:
        """Everything the host needs from the device after `done` steps of a group of n_batches — ONE launch (ops.collect_summary, with stop
        rules ops.collect_summary_stop: the same record with the rows' finish arrays behind it), ONE pinned device-to-host copy, ONE
        synchronise — by name: err (the table-range flag), unfinished (any row), nf_rows [B] / nf_batch [n_batches] (the range guard's
        flags), first_eos [B] (each row's first EOS step, -1: none) and, with stop rules, finish_step / finish_reason / stop_index [B]."""
        B, eos = self.B, self.cfg.eos_token_id
        if self.mode.stop:
            ops.collect_summary_stop(self.err, self.unfinished, self.nf, self.nf_batch, n_batches, self.tokens, done, eos, self.gen_cfg,
                                     self.finish_step, self.finish_reason, self.stop_index, self.summary_stop)
            dst, host = self.summary_stop, self.summary_stop_host
        else:
            ops.collect_summary(self.err, self.unfinished, self.nf, self.nf_batch, n_batches, self.tokens, done, eos, self.gen_cfg, self.summary)
            dst, host = self.summary, self.summary_host
        host.copy_(dst, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        rec = host.tolist()
        # the record's words: [err, any unfinished, nf rows [B], nf batches [n_batches], first EOS [B]] (+ the three finish arrays [B] each)
        o = 2 + B + n_batches
        out = dict(err=rec[0], unfinished=rec[1], nf_rows=rec[2: 2 + B], nf_batch=rec[2 + B: o], first_eos=rec[o: o + B])
        if self.mode.stop:
            names = ("finish_step", "finish_reason", "stop_index")
            out.update({nm: rec[o + (i + 1) * B: o + (i + 2) * B] for i, nm in enumerate(names)})
        return out

    def head_and_select(self, hn, advance: bool):
        cfg, W = self.cfg, self.W
        hp = W.get("llm.head.wp")
        lg = None
        hk, m = self.hooks, self.mode
        # token log-probs: from the head's partials (the LSE head + padt_greedy_step_lp, no logit row) when the token is their arg-max; from
        # the fp32 row the selection kernel read when it is not (sampling, caller processors rewrote the row)
        lp_rows = m.token_logprobs and (m.sampling or m.processors)
        psum, lp_out = (self.part_sum, self.logprobs) if (m.token_logprobs and not lp_rows) else (None, None)
        top_on = bool(m.top_k or m.patches)                  # top_logprobs / output_patch_logprobs read the whole processed row too
        if m.sampling or m.keep_scores or top_on:            # the sampling kernel / output_scores need the whole masked / penalised logit row
            if self.logits is None:
                self.logits = torch.empty((self.B, (cfg.vocab_size + self.np_max + 3) // 4 * 4), device=hn.device, dtype=torch.float32)
            lg = self.logits
        ban = None
        if m.rules:                                          # this step's ban bitmap from the rows' histories; the head then writes -inf there
            ban = ops.gen_rules(self.rules, self.hist, self.hist_len, self.tokens, self.step, self.ban, cfg.vocab_size + self.np_max)
        if m.automaton:                                      # the columns the rows' automaton states allow; with rules the union of both bitmaps
            ban = ops.token_automaton(self.atab, self.gen_cfg, self.vrt_off, self.tokens, self.step, self.unfinished, self.astate, self.aban,
                                      cfg.vocab_size + self.np_max, cfg.vocab_size, rules_ban=ban)
        if m.stop:                                           # min_tokens: the EOS ids of a row still below its minimum, on top of whatever is banned already
            ban = ops.stop_ban(self.gen_cfg, cfg.eos_token_id, self.step, self.min_tok, self.sban, cfg.vocab_size + self.np_max, ban_in=ban)
        # forced tokens (generate(forced_tokens=)): the caller's table decides the token of a forced row.  Fused log-probs: the probe head leaves
        # the processed logit of the forced column next to the LSE partials; without log-probs the plain head runs and only the bookkeeping differs
        fc = self.forced if m.forced else None
        probe = self.probe_val if (fc is not None and psum is not None) else None
        head_in, head_kw = hn, dict(mode_table=self.mode_table, step=self.step, gen_cfg=self.gen_cfg, seen=self.seen, logits=lg, ban=ban)
        if hp is not None:                                   # packed table + packed hidden rows: 1 KiB contiguous wave loads
            ops.pack_rows(hn, self.hn_pk, self.B, to_packed=True)
            head_in, head_kw = self.hn_pk, dict(head_kw, table_packed=hp, rows=self.B)
        if m.counts:                                         # the count edits (and, with mode.bias, the additive ones): the same heads over the session's count tables
            ops.vrt_head_counts(head_in, W["llm.head"], self.proto, self.vrt_off, self.part_val, self.part_idx, cfg.eos_token_id, self.cnt_text,
                                self.cnt_patch, self.near, self.cpen, bias=self.bias if m.bias else None, decay=self.decay if m.bias else None,
                                part_sum=psum, forced=fc if probe is not None else None, probe_val=probe, **head_kw)
        elif m.bias:                                         # the additive edits: the same heads, reading the session's bias vector and decay table
            ops.vrt_head_bias(head_in, W["llm.head"], self.proto, self.vrt_off, self.part_val, self.part_idx, cfg.eos_token_id, bias=self.bias,
                              decay=self.decay, part_sum=psum, forced=fc if probe is not None else None, probe_val=probe, **head_kw)
        elif probe is not None:
            ops.vrt_head_probe(head_in, W["llm.head"], self.proto, self.vrt_off, self.part_val, self.part_idx, cfg.eos_token_id, psum, fc, probe,
                               **head_kw)
        else:
            ops.vrt_head(head_in, W["llm.head"], self.proto, self.vrt_off, self.part_val, self.part_idx, cfg.eos_token_id, part_sum=psum, **head_kw)
        if m.processors:
            # padt.py:717 `next_token_scores = logits_processor(input_ids, next_token_logits)` with the CALLER's processors: they see the rows the head
            # wrote (logit mask + the built-in processors applied) and the sequences so far, and what they return is what is scored / selected / kept
            view = lg[: hk["B"], : hk["table_rows"]]
            new = _call_hooks(hk["processors"], hk["sequences"](), view, chain=True)
            if new is not view:
                view.copy_(new.to(torch.float32))
        if m.keep_scores and self.scores is None:
            self.scores = torch.zeros((self.t_max,) + tuple(self.logits.shape), device=hn.device, dtype=torch.float32)
        if m.keep_logits:                                    # padt.py:721-722: raw_logits += (next_token_logits,) — differ from the scores under sampling
            if self.raw_scores is None:
                self.raw_scores = torch.zeros((self.t_max,) + tuple(self.logits.shape), device=hn.device, dtype=torch.float32)
            ops.stash_step_f32(lg, self.step, self.raw_scores)
        if m.keep_scores and not m.sampling:                 # padt.py:719-720: scores += (next_token_scores,) — filed under the device step counter
            ops.stash_step_f32(lg, self.step, self.scores)
        nblk = self.nblk
        if m.sampling:                                       # padt.py:740-743: multinomial over softmax of the warped scores
            # with keep_scores (or token_logprobs) the session's gen_cfg has write_back set: lg then holds the warped rows (l / T, -inf outside top-k / top-p),
            # HF's next_token_scores — the warpers are part of its logits_processor (padt.py:717)
            # keyed by each row's place in its own batch (batch_row0), so a batch of a merged decode group draws what it draws alone
            ops.sample_token(lg, cfg.vocab_size + self.np_max, self.gen_cfg, self.step, self.part_val, self.part_idx, self.B,
                             vocab=cfg.vocab_size, vrt_off=self.vrt_off, row_base=self.batch_row0)
            if m.warpers:
                # min_p / typical_p / epsilon_cutoff / eta_cutoff (HF's warpers after top-p): write_back is set, so lg holds the row after
                # temperature / top-k / top-p; the kernel warps it further in place and draws from what stays, replacing sample_token's draw —
                # every reader below (scores stash, token / top-k log-probs, the caller's criteria) then sees HF's next_token_scores
                ops.warp_sample_rows(lg, cfg.vocab_size + self.np_max, self.gen_cfg, self.step, self.part_val, self.part_idx, self.B,
                                     vocab=cfg.vocab_size, vrt_off=self.vrt_off, row_base=self.batch_row0)
            if m.keep_scores:
                ops.stash_step_f32(lg, self.step, self.scores)
            nblk = 1
        elif m.processors:                                   # the head's fused arg-max partials describe the rows BEFORE the caller's processors
            ops.argmax_rows(lg, cfg.vocab_size + self.np_max, self.part_val, self.part_idx, self.B)
            nblk = 1
        if fc is not None and (m.sampling or m.processors):                   # the draw / arg-max of a forced row gives way to the caller's token: scored and appended below
            ops.forced_override(self.part_idx, fc, self.step, self.unfinished, cfg.vocab_size + self.np_max, self.B)
        if lp_rows:                                          # before greedy_step clears `unfinished` and bumps the step counter
            ops.token_logprob_rows(lg, cfg.vocab_size + self.np_max, self.part_idx, self.unfinished, self.step, self.logprobs, self.B)
        if top_on:                                           # the row as selected from (warped under sampling: write_back), `unfinished` as on entry
            ops.topk_logprob_rows(lg, cfg.vocab_size + self.np_max, self.unfinished, self.step, self.topk_ws, self.B, top_idx=self.top_idx,
                                  top_val=self.top_val, vrt_off=self.vrt_off if m.patches else None, vocab=cfg.vocab_size,
                                  patch_lp=self.patch_lp if m.patches else None)
        if m.beam:
            # the K rows of a sample are its beams: their `keep` best candidates of this step are merged, the next live beams and the finished
            # hypotheses selected (generation.beam_step), and the caches of every layer follow the beams' parents
            bs = self.beam
            rep_lp = None
            if psum is not None:
                # the log-probs REPORTED for the candidates are the values token_logprobs defines: the greedy step's fold of the LSE head's
                # partials, so a hypothesis' token_logprobs are the bits the greedy call and score_completions report; the scores add the top-k's
                rep_lp = ops.beam_cand_lp(self.part_val, self.part_idx, psum, nblk, lg, cfg.vocab_size + self.np_max, self.top_idx, self.step,
                                          self.beam_rep[: self.B * m.top_k].view(self.B, m.top_k))
            ops.beam_step(bs, self.top_idx, self.top_val, hn, self.hidden_buf, self.unfinished, self.cur_tok, self.step, self.slot, self.lens,
                          self.pos3, self.vrt_off, cfg.eos_token_id, cfg.pad_token_id, cfg.vocab_size, cfg.vocab_size + self.np_max,
                          advance=advance, gen_cfg=self.gen_cfg, err=self.err, rep_lp=rep_lp)
            ops.beam_reorder_kv(self.beam_kv, bs.perm, bs.p0, self.slot, bs.B, bs.K, cfg.num_key_value_heads, cfg.head_dim, self.s_max,
                                self.t_max, rows=self.B)
        elif fc is not None:
            ops.forced_step(self.part_val, self.part_idx, nblk, hn, self.hidden_buf, self.unfinished, self.tokens,
                            self.cur_tok, self.step, self.slot, self.lens, self.pos3, cfg.eos_token_id, cfg.pad_token_id, fc,
                            cfg.vocab_size + self.np_max, advance=advance, gen_cfg=self.gen_cfg, seen=self.seen, part_sum=psum, logprobs=lp_out,
                            probe_val=probe)
        else:
            ops.greedy_step(self.part_val, self.part_idx, nblk, hn, self.hidden_buf, self.unfinished, self.tokens,
                            self.cur_tok, self.step, self.slot, self.lens, self.pos3, cfg.eos_token_id, cfg.pad_token_id,
                            advance=advance, gen_cfg=self.gen_cfg, seen=self.seen, part_sum=psum, logprobs=lp_out)
        if m.counts:                                         # the step counter is bumped: every row still unfinished counts the token it just generated
            ops.count_update(self.tokens, self.step, self.unfinished, self.vrt_off, self.cgrid, self.cradius, self.cnt_text, self.cnt_patch,
                             self.near, cfg.vocab_size, self.np_max)
        if m.stop:                                           # the step counter is bumped: the rows hold *step tokens.  EOS, stop sequence, budget
            ops.stop_match(self.stab, self.gen_cfg, cfg.eos_token_id, self.tokens, self.step, self.min_tok, self.max_tok, self.unfinished,
                           self.finish_step, self.finish_reason, self.stop_index)
        if hk is not None:
            hk["t"] += 1
            if hk["criteria"]:
                # padt.py:752 `unfinished_sequences = unfinished_sequences & ~stopping_criteria(input_ids, scores)` for the caller's criteria (EOS and
                # the length limit are the loop's own: padt_greedy_step / max_new_tokens)
                kept = tuple(self.scores[i, : hk["B"], : hk["table_rows"]] for i in range(hk["t"])) if hk["pass_scores"] else None
                stop = _call_hooks(hk["criteria"], hk["sequences"](), kept, chain=False)
                if not isinstance(stop, torch.Tensor):       # criteria of the old API answer one bool for the whole batch
                    stop = torch.full((hk["B"],), bool(stop), device=hn.device)
                if m.stop:                                   # a row the caller's criteria end: recorded here, reason "criteria" — padt_stop_match then leaves it alone
                    nb = hk["B"]
                    new = stop.to(device=hn.device, dtype=torch.bool) & (self.unfinished[:nb] != 0) & (self.finish_reason[:nb] == 0)
                    self.finish_step[:nb].copy_(torch.where(new, torch.full_like(self.finish_step[:nb], hk["t"] - 1), self.finish_step[:nb]))
                    self.finish_reason[:nb].copy_(torch.where(new, torch.full_like(self.finish_reason[:nb], ops.STOP_REASONS.index("criteria")),
                                                              self.finish_reason[:nb]))
                self.unfinished[: hk["B"]].mul_((~stop.to(device=hn.device, dtype=torch.bool)).to(self.unfinished.dtype))

    def run_steps(self, n: int, use_graph: bool = True):
        if n <= 0:
            return
        one_step = self.step_kernels if self.step_fn is None else (lambda: self.step_fn(self))    # reference precision: reference.ReferencePath.step
        if not use_graph:
            for _ in range(n):
                one_step()
            return
        gkey = self.mode                                     # different kernel sequences (and output buffers) → one captured graph per mode
        if gkey not in self.graphs:
            one_step()                                       # real step; also pays every one-time kernel attribute call
            n -= 1
            g = torch.cuda.CUDAGraph()
            # No garbage collection inside the capture: a dead reference cycle that still owns GPU objects (a released model's sessions with
            # their graphs, events and cached blocks) would be finalised on this thread in the middle of the capture, which aborts the process.
            gc_on = gc.isenabled()
            gc.disable()
            try:
                # thread_local: only THIS thread's calls are checked during capture.  With world > 1 the process group's watchdog thread polls
                # the events of an in-flight result gather (pipeline.ResultExchange) while a later lane captures its graph; under the default
                # global mode such a query from another thread invalidates the capture.
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    one_step()
            finally:
                if gc_on:
                    gc.enable()
            self.graphs[gkey] = g
        t = ops.STEP_TIMER
        ev = t.begin() if t is not None else None
        for _ in range(n):
            self.graphs[gkey].replay()
        if ev is not None:
            t.end(ev, (n, self.B))


class LanguageModel:
    def __init__(self, cfg: PaDTConfig, W, device):
        self.cfg, self.W, self.device = cfg, W, device
        self._sessions = {}

    def prototypes(self, image_embeds: torch.Tensor, out: Optional[torch.Tensor] = None, nf=None) -> torch.Tensor:
        """padt.py:187-191: LayerNorm then + W2(W1 x).  nf: int32 device flag set when a prototype row is not finite."""
        W = self.W
        if not self.cfg.use_visual_prototype_projection:
            if out is None:
                out = image_embeds.clone()
            else:
                out.copy_(image_embeds)
        else:
            p = ops.layernorm(image_embeds, W["proto.norm.w"], W["proto.norm.b"], eps=1e-5)
            t = ops.gemm(p, W["proto.0.w"])
            out = ops.gemm(t, W["proto.1.w"], out=out, epilogue=ops.EPI_RESID, residual=p)
        if nf is not None:
            ops.check_finite(out, nf)
        return out

    def session(self, B: int, need_s: int, need_np: int, need_t: int, lane: int = 0, grow: bool = True) -> Optional[DecodeSession]:
        """The lane's session for B rows, (re)allocated when too small; with grow=False returns None instead (a session
        that already holds other batches' KV rows must not be replaced)."""
        s_max = (need_s + 63) // 64 * 64
        key = (B, lane)
        s = self._sessions.get(key)
        if not grow:
            return s if (s is not None and s.s_max >= s_max and s.np_max >= need_np and s.t_max >= need_t) else None
        if s is None or s.s_max < s_max or s.np_max < need_np or s.t_max < need_t:
            s = DecodeSession(self.cfg, self.W, B, max(s_max, s.s_max if s else 0), max(need_np, s.np_max if s else 0),
                              max(need_t, s.t_max if s else 0), self.device)
            self._sessions[key] = s
        return s

    def prefill(self, plan: PromptPlan, image_embeds: torch.Tensor, sess: DecodeSession, nf=None, kv_out=None):
        """Packed prefill; fills the session's KV caches; returns the post-norm hidden states of all prompt tokens (T,D).
        nf: int32 device flag set when a post-norm row is not finite (the residual stream absorbs every upstream inf / NaN).
        kv_out = (K, V), each (layers, n_join, Hkv * hd), with a shared plan: the join buffers of layer i ARE K[i] / V[i] (encode_prefix:
        the prompt pass writes the handle's rows itself)."""
        cfg, W = self.cfg, self.W
        Hq, Hkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        sh = plan.shared                                         # generate(image_index=): the smaller token set (plan_prompt_shared);
        src = plan if sh is None else sh
        T = src.ids.numel()
        dev = image_embeds.device
        bf = W.op16
        x = ops.embed_tokens(src.ids, src.img_index, W["llm.embed"], sess.proto, image_embeds, err_flag=sess.err)
        x32 = ops.cast_x16_f32(x)                                # fp32 residual stream; x stays its 16-bit mirror
        eps_n = W.eps_m(cfg.rms_norm_eps)
        if ops.stream_scale(bf) != 1.0:
            ops.cast_f32_x16(x32, out=x, scale=ops.stream_scale(bf))           # mirrors hold X(scale * x32) (fp16: 2^-4, see ops.stream_scale)
        n = torch.empty_like(x)
        rstd = torch.empty((T,), device=dev, dtype=torch.float32)
        qkv = torch.empty((T, (Hq + 2 * Hkv) * hd), device=dev, dtype=bf)
        q = torch.empty((T, Hq * hd), device=dev, dtype=bf)
        if sh is None:
            kp = torch.empty((T, Hkv * hd), device=dev, dtype=bf)
        elif kv_out is None:                                     # roped K / V rows of every key segment: [prefix] / [group prefix | own tokens]
            kj = torch.empty((sh.n_join, Hkv * hd), device=dev, dtype=bf)
            vj = torch.empty((sh.n_join, Hkv * hd), device=dev, dtype=bf)
        pre = sh.prefix if sh is not None else None              # generate(prefix=): cached prefix rows instead of prefix segments
        att = torch.empty((T, Hq * hd), device=dev, dtype=bf)
        h = torch.empty((T, W.llm_ipad), device=dev, dtype=bf)
        mx = max(plan.lens)
        f8 = W.fp8_prefill
        if f8:                                                       # e4m3 images of the three GEMM inputs of a layer + their row scales
            x8 = torch.empty((T, cfg.hidden_size), device=dev, dtype=torch.uint8)
            a8 = torch.empty((T, Hq * hd), device=dev, dtype=torch.uint8)
            h8 = torch.empty((T, W.llm_ipad), device=dev, dtype=torch.uint8)
            rs8 = torch.empty((T,), device=dev, dtype=torch.float32)
        for i in range(cfg.num_hidden_layers):
            p = f"llm.{i}."
            # fp8 x fp8 MFMA path (llm_weights="fp8"): the GEMM input rows are quantised to e4m3 (power-of-two row scale x the folded norm's
            # rstd) and multiplied with the e4m3 weight image; a projection whose shape the fp8 kernel does not take keeps the bf16 GEMM
            if f8 and (p + "qkv.w8") in W:
                ops.quant_rows_fp8(x, norm_eps=eps_n, out=x8, rs=rs8)
                ops.gemm_fp8(x8, W[p + "qkv.w8"], W[p + "qkv.ws"], rs8, bias=W[p + "qkv.b"], out=qkv)
            else:
                ops.row_rstd(x, eps=eps_n, out=rstd)                       # norm weight is folded into qkv.w
                ops.gemm(x, W[p + "qkv.w"], W[p + "qkv.b"], out=qkv, row_scale=rstd)
            if sh is None:
                ops.llm_qkv_post(qkv, plan.pos3, sess.inv_freq, q, sess.kc[i], sess.vtc[i], Hq, Hkv, hd, sess.s_max,
                                 cfg.mrope_section, sample=plan.sample, slot=plan.slot, k_pack=kp, cache_packed=sess.cache_packed)
                ops.attn_varlen(q, kp, qkv[:, (Hq + Hkv) * hd:], att, plan.cu, plan.cu, mx, Hq, Hkv, hd, causal=True)
            else:
                # a token is rotated once and fanned out to every member's cache images and key segment; a suffix's queries then see
                # [group prefix | own tokens] under the bottom-right aligned causal mask (Lk > Lq), exactly the keys of its full row
                if kv_out is not None:
                    kj, vj = kv_out[0][i], kv_out[1][i]
                if pre is not None:                              # the cached rows go where the shared pass would have fanned them out
                    ops.kv_prefix_fanout(pre.k[i], pre.v[i], pre.pre_off, *sh.members, sh.max_p, sess.kc[i], sess.vtc[i], kj, vj, Hkv, hd,
                                         sess.s_max, cache_packed=sess.cache_packed)
                ops.llm_qkv_post_shared(qkv, sh.pos3, sess.inv_freq, q, sess.kc[i], sess.vtc[i], kj, vj, sh.dst_off, sh.dst_sample,
                                        sh.dst_slot, sh.dst_row, Hq, Hkv, hd, sess.s_max, cfg.mrope_section,
                                        cache_packed=sess.cache_packed)
                ops.attn_varlen(q, kj, vj, att, sh.cu_q, sh.cu_k, sh.max_q, Hq, Hkv, hd, causal=True)
            if f8 and (p + "o.w8") in W:
                ops.quant_rows_fp8(att, out=a8, rs=rs8)
                ops.gemm_fp8(a8, W[p + "o.w8"], W[p + "o.ws"], rs8, epilogue=ops.EPI_RESID, x32=x32, xb=x)
            else:
                ops.gemm_resid32(att, W[p + "o.w"], None, x32, x)
            if f8 and (p + "gu.w8") in W:
                ops.quant_rows_fp8(x, norm_eps=eps_n, out=x8, rs=rs8)
                ops.gemm_fp8(x8, W[p + "gu.w8"], W[p + "gu.ws"], rs8, out=h, epilogue=ops.EPI_SWIGLU)
            else:
                ops.row_rstd(x, eps=eps_n, out=rstd)                       # norm weight is folded into gu.w
                ops.gemm(x, W[p + "gu.w"], out=h, epilogue=ops.EPI_SWIGLU, row_scale=rstd)
            if f8 and (p + "down.w8") in W:
                ops.quant_rows_fp8(h, out=h8, rs=rs8)
                ops.gemm_fp8(h8, W[p + "down.w8"], W[p + "down.ws"], rs8, epilogue=ops.EPI_RESID, x32=x32, xb=x)
            else:
                ops.gemm_resid32(h, W[p + "down.w"], None, x32, x)
        ops.rmsnorm_f32(x32, W["llm.norm"], out=n, eps=cfg.rms_norm_eps)
        if nf is not None:
            ops.check_finite(n, nf)
        if sh is not None:                                       # back to the unshared packed per-sample order every consumer reads
            if pre is not None:                                  # the prefix rows of that order are the handle's
                n = torch.cat([n, pre.hidden])
            n = ops.gather_rows(n, sh.unshare)
        return n
