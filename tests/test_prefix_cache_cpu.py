"""encode_prefix / generate(prefix=) — host side: the prefix plan against plan_prompt_shared on the same rows, the argument policy by message,
and the new entry point's argument validation (no device needed)."""
import inspect
from types import SimpleNamespace

import pytest
import torch

import padt_amd
from padt_amd import _lib
from padt_amd.llm import (PromptPrefix, check_shared_destinations, plan_prefix_build, plan_prompt, plan_prompt_prefix, plan_prompt_shared)
from prefix_cache_util import prefix_case


@pytest.fixture(scope="module")
def case():
    cfg = padt_amd.small_test_config()
    return cfg, prefix_case(cfg)


def handle(c, rows=None):
    """The metadata half of a handle: what the planner reads."""
    return PromptPrefix(ids=[list(r) for r in (rows or c["pre_rows"])], grid=c["grid"].clone())


@pytest.mark.parametrize("row0,proto_row0", [(0, 0), (5, 61)])
def test_prefix_plan_is_the_shared_plan_minus_the_prefix_segments(case, row0, proto_row0):
    cfg, c = case
    B, idx = 6, c["q_index"]
    ids = c["q_ids"].clone()
    if proto_row0:                                                # a prompt VRT id among sample 3's own tokens: shifted with the batch's prototype rows
        ids[3, -2] = cfg.vocab_size + sum(c["n_merged"][u] for u in idx[:3]) + 3
    shared = plan_prompt_shared(cfg, ids, c["q_am"], c["grid"], idx, "cpu", row0=row0, proto_row0=proto_row0)
    plan = plan_prompt_prefix(cfg, ids, c["q_am"], handle(c), idx, "cpu", row0=row0, proto_row0=proto_row0)
    ss, sp = shared.shared, plan.shared
    # everything downstream of the prompt pass reads the expanded plan: the same one
    assert plan.next_pos == shared.next_pos and plan.lens == shared.lens and plan.vrt_off == shared.vrt_off and plan.L_pad == shared.L_pad
    assert plan.first_row == shared.first_row == row0
    for f in ("rope_deltas", "cu", "last_idx", "ids", "pos3", "img_index", "sample", "slot"):
        assert torch.equal(getattr(plan, f), getattr(shared, f)), f
    for f in ("low_rows", "patch_rows", "grid_x"):
        assert torch.equal(getattr(sp, f), getattr(ss, f)), f
    assert sp.n_images == ss.n_images == 3
    # the token set: the own tokens and no prefix token
    P, own = c["q_prefix"], c["q_own"]
    assert list(sp.prefix_len) == P and sp.max_p == max(P) and sp.groups == []
    Ts = sum(own)
    assert sp.ids.numel() == sp.pos3.shape[1] == sp.img_index.numel() == Ts == sum(plan.lens) - sum(P) and sp.max_q == max(own)
    assert (sp.img_index < 0).all()                               # every image token lies in a prefix
    G = len(ss.groups)
    assert G == 2
    cu = plan.cu.tolist()
    cq_p, ck_p, cq_s, ck_s = (t.tolist() for t in (sp.cu_q, sp.cu_k, ss.cu_q, ss.cu_k))
    assert [cq_p[b + 1] - cq_p[b] for b in range(B)] == own
    dp = [t.tolist() for t in (sp.dst_off, sp.dst_sample, sp.dst_slot, sp.dst_row)]
    ds = [t.tolist() for t in (ss.dst_off, ss.dst_sample, ss.dst_slot, ss.dst_row)]
    p_off = [0, c["P"][0], c["P"][0] + c["P"][1], sum(c["P"])]
    for b in range(B):
        a = c["prefix"][b]                                        # what the shared plan shares of this row (0 for sample 3: it has no group)
        assert ck_p[b + 1] - ck_p[b] == ck_s[G + b + 1] - ck_s[G + b] == P[b] + own[b]      # key segment [prefix | own]
        for j in range(own[b]):
            r = cu[b] + P[b] + j                                  # row of the unshared packed order
            tp, ts = int(sp.unshare[r]), int(ss.unshare[r])
            assert tp - cq_p[b] == j == ts - cq_s[G + b] - (P[b] - a)
            assert sp.ids[tp] == ss.ids[ts] == plan.ids[r] and torch.equal(sp.pos3[:, tp], ss.pos3[:, ts])
            assert sp.img_index[tp] == ss.img_index[ts]
            # one destination: the row's cache image at slot P + j, and the same place of its key segment
            assert dp[0][tp + 1] - dp[0][tp] == 1 == ds[0][ts + 1] - ds[0][ts]
            n_p, n_s = dp[0][tp], ds[0][ts]
            assert dp[1][n_p] == ds[1][n_s] == row0 + b and dp[2][n_p] == ds[2][n_s] == P[b] + j
            assert dp[3][n_p] - ck_p[b] == ds[3][n_s] - ck_s[G + b] == P[b] + j
        # the prefix rows of the unshared order are the handle's hidden rows, behind the token set
        assert sp.unshare[cu[b]: cu[b] + P[b]].tolist() == list(range(Ts + p_off[idx[b]], Ts + p_off[idx[b]] + P[b]))
    assert [t.tolist() for t in sp.members] == [idx, [row0 + b for b in range(B)], ck_p[:-1]]
    # the host check of the destinations: no prefix slot in the list, no (row, slot) twice, the session's bounds
    check_shared_destinations(sp, row0 + B, max(plan.lens))
    assert all(slot >= P[s - row0] for s, slot in zip(dp[1], dp[2]))
    assert len(set(zip(dp[1], dp[2]))) == len(dp[1]) == Ts and sorted(dp[3]) == sorted(
        r for b in range(B) for r in range(ck_p[b] + P[b], ck_p[b + 1]))
    with pytest.raises(ValueError, match="outside the session"):
        check_shared_destinations(sp, row0 + B, max(plan.lens) - 1)
    with pytest.raises(ValueError, match="outside the session"):
        check_shared_destinations(sp, row0 + B - 1, max(plan.lens))


def test_default_index_and_vrt_ids_in_image_local_numbering(case):
    """B == N rows without an index; a VRT id INSIDE a prefix is compared in image-local numbering (the row counts the batch's patches)."""
    cfg, c = case
    V, n_m = cfg.vocab_size, c["n_merged"]
    pre = [list(r) + [V + 3] for r in c["pre_rows"]]              # local patch 3 of each image closes its prefix
    rows = [pre[0][:-1] + [V + 3, 7], pre[1][:-1] + [V + n_m[0] + 3, 8, 9], pre[2][:-1] + [V + n_m[0] + n_m[1] + 3, 5]]
    L = max(len(r) for r in rows)
    ids, am = torch.full((3, L), cfg.pad_token_id, dtype=torch.long), torch.zeros((3, L), dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, L - len(r):], am[b, L - len(r):] = torch.tensor(r), 1
    plan = plan_prompt_prefix(cfg, ids, am, handle(c, pre), None, "cpu")
    assert [t.tolist() for t in plan.shared.members[:2]] == [[0, 1, 2], [0, 1, 2]] and list(plan.shared.prefix_len) == [len(r) for r in pre]
    assert plan.shared.ids.tolist() == [7, 8, 9, 5]
    ids[1, L - 3] = V + 3                                         # image 0's numbering in row 1: another patch of image 1's table
    with pytest.raises(ValueError, match=rf"row 1 does not start with the prefix of image 1: first difference at position {len(pre[1]) - 1} "):
        plan_prompt_prefix(cfg, ids, am, handle(c, pre), None, "cpu")


def test_prefix_validation_messages(case):
    cfg, c = case
    h = handle(c)
    # sample 6 of the case asks about image 1 behind ANOTHER text: rejected by name, with the first differing position
    first = next(j for j, (x, y) in enumerate(zip(c["rows"][6], c["pre_rows"][1])) if x != y)
    with pytest.raises(ValueError, match=rf"row 6 does not start with the prefix of image 1: first difference at position {first} "):
        plan_prompt_prefix(cfg, c["ids"], c["am"], h, c["image_index"], "cpu")
    # a row that equals its prefix, and one that ends inside it: no token of its own
    whole = handle(c, [c["pre_rows"][0], c["rows"][4], c["pre_rows"][2]])
    with pytest.raises(ValueError, match=rf"row 4 has no token of its own: it ends at position {len(c['rows'][4])}, the prefix of image 1 has {len(c['rows'][4])}"):
        plan_prompt_prefix(cfg, c["q_ids"], c["q_am"], whole, c["q_index"], "cpu")
    longer = handle(c, [c["pre_rows"][0], c["rows"][1][:-1], c["pre_rows"][2]])
    with pytest.raises(ValueError, match=r"row 4 has no token of its own"):
        plan_prompt_prefix(cfg, c["q_ids"], c["q_am"], longer, c["q_index"], "cpu")
    with pytest.raises(ValueError, match=r"image_index\[3\] = 3 is outside \[0, 3\): the prefix holds 3 images"):
        plan_prompt_prefix(cfg, c["q_ids"], c["q_am"], h, [0, 1, 0, 3, 1, 0], "cpu")
    with pytest.raises(ValueError, match=r"image_index\[0\] = -1 is outside"):
        plan_prompt_prefix(cfg, c["q_ids"], c["q_am"], h, torch.tensor([-1, 1, 0, 2, 1, 0]), "cpu")
    with pytest.raises(ValueError, match="image_index has 5 entries for a batch of 6"):
        plan_prompt_prefix(cfg, c["q_ids"], c["q_am"], h, c["q_index"][:5], "cpu")
    with pytest.raises(ValueError, match="without image_index needs one row per image of the prefix: 6 rows, 3 images"):
        plan_prompt_prefix(cfg, c["q_ids"], c["q_am"], h, None, "cpu")
    # an image of the handle that no row asks about is no error: the handle outlives the call
    plan = plan_prompt_prefix(cfg, c["q_ids"][:3], c["q_am"][:3], h, [0, 1, 0], "cpu")
    assert plan.shared.n_images == 3 and plan.shared.max_p == max(c["P"][:2])


def test_the_builders_plan_writes_join_rows_only(case):
    cfg, c = case
    plan = plan_prefix_build(cfg, c["pre_ids"], c["pre_am"], c["grid"], "cpu")
    full = plan_prompt(cfg, c["pre_ids"], c["pre_am"], c["grid"], "cpu")
    sh = plan.shared
    T = sum(c["P"])
    assert plan.lens == c["P"] and torch.equal(plan.ids, full.ids) and torch.equal(plan.pos3, full.pos3)
    assert sh.ids is plan.ids and (sh.dst_sample == -1).all() and sh.dst_row.tolist() == list(range(T)) == sh.unshare.tolist()
    assert sh.dst_off.tolist() == list(range(T + 1)) and sh.n_join == T and torch.equal(sh.cu_q, full.cu) and torch.equal(sh.cu_k, full.cu)
    check_shared_destinations(sh, 1, 1)                           # no cache destination at all
    # a row that does not hold its image's tokens completely
    cut = c["pre_ids"].clone()
    cut[2, -(3 + 2)] = 5                                          # one image token of image 2 replaced by text
    with pytest.raises(ValueError, match=r"row 2 must contain the image tokens of image 2 completely: 14 image tokens, 15 features"):
        plan_prefix_build(cfg, cut, c["pre_am"], c["grid"], "cpu")
    with pytest.raises(ValueError, match="one row per image: 3 rows, 2 images"):
        plan_prefix_build(cfg, c["pre_ids"], c["pre_am"], c["grid"][:2], "cpu")


def test_handle_metadata_without_a_device(case):
    cfg, c = case
    h = handle(c)
    assert h.n_images == 3 and h.lens == c["P"] and h.off == [0, c["P"][0], c["P"][0] + c["P"][1], sum(c["P"])] and h.nbytes == 0
    h.k = torch.zeros((2, sum(c["P"]), 8), dtype=torch.float16)
    h.v = torch.zeros_like(h.k)
    h.pe = (torch.zeros(4, 2), torch.zeros(4, 2))
    assert h.nbytes == 2 * h.k.numel() * 2 + 2 * 8 * 4
    assert h.image_k(1).shape == (2, c["P"][1], 8) and h.image_k(1).data_ptr() == h.k[0, c["P"][0]].data_ptr()


# ------------------------------------------------------------------------------------------------------------ the argument policy
def _model(**attrs):
    """An uninitialised instance: generate() reaches generate_launch's argument checks without a device (the pattern of test_shared_prefix_cpu.py)."""
    from padt_amd.modeling import PaDTForConditionalGeneration
    m = PaDTForConditionalGeneration.__new__(PaDTForConditionalGeneration)
    m.generation_config = SimpleNamespace(pad_token_id=0, repetition_penalty=1.0)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_generate_argument_policy_by_message(case):
    cfg, c = case
    h = handle(c)
    ids = torch.zeros((2, 4), dtype=torch.long)
    with pytest.raises(ValueError, match=r"generate\(prefix=\.\.\.\): the handle holds the images — pixel_values and image_grid_thw must be None"):
        _model().generate(input_ids=ids, max_new_tokens=3, prefix=h, pixel_values=torch.zeros(4, 4), image_grid_thw=c["grid"])
    with pytest.raises(ValueError, match="pixel_values and image_grid_thw must be None"):
        _model().generate(input_ids=ids, max_new_tokens=3, prefix=h, image_grid_thw=c["grid"])
    with pytest.raises(NotImplementedError, match=r"generate\(prefix=\.\.\.\) is not implemented with precision='reference'"):
        _model(precision="reference").generate(input_ids=ids, max_new_tokens=3, prefix=h)
    with pytest.raises(NotImplementedError, match=r"encode_prefix.*precision='reference'"):
        _model(precision="reference").encode_prefix(ids, None, torch.zeros(4, 4), c["grid"])
    with pytest.raises(TypeError, match="takes the handle encode_prefix returns"):
        _model().generate(input_ids=ids, max_new_tokens=3, prefix=object())
    with pytest.raises(NotImplementedError, match="past_key_values"):          # HF's argument stays rejected by name
        _model().generate(input_ids=ids, max_new_tokens=3, past_key_values=h)


def test_prefix_is_forwarded_where_image_index_is():
    from padt_amd import harness
    from padt_amd.modeling import PaDTForConditionalGeneration as M
    from padt_amd.pipeline import PipelinedRunner, rec_batch
    for fn in (rec_batch, PipelinedRunner.submit):
        assert inspect.signature(fn).parameters["prefix"].default is None
    assert inspect.signature(M._launch).parameters["prefix"].default is None
    assert "prefix" not in inspect.signature(M.generate).parameters and "prefix" not in inspect.signature(M.generate_launch).parameters
    assert 'extra["prefix"] = b["prefix"]' in inspect.getsource(harness.infer_dataset)
    assert "prefix=sub[\"prefix\"]" in inspect.getsource(M._non_finite_batch)      # what the bf16 re-run keeps
    got = {}

    class Fake:
        def generate(self, **kw):
            got.update(kw)
            raise KeyboardInterrupt
    h = PromptPrefix(ids=[[1, 2]], grid=torch.tensor([[1, 4, 4]]))
    proc = SimpleNamespace(assign_to_global_vrt_id=lambda ids, grid: (got.setdefault("grid", grid), ids)[1])
    with pytest.raises(KeyboardInterrupt):
        rec_batch(Fake(), proc, torch.zeros((2, 3), dtype=torch.long), None, None, None, max_new_tokens=2, prefix=h, image_index=[0, 0])
    assert got["prefix"] is h and got["pixel_values"] is None and got["image_grid_thw"] is None and got["image_index"] == [0, 0]
    assert got["grid"].tolist() == [[1, 4, 4]] * 2                # the handle's grids, per sample


# ------------------------------------------------------------------------------------------------------------ the entry point
def test_fanout_entry_point_is_declared_exported_and_validates():
    lib = _lib.load()
    decl = _lib.parse_header()["padt_kv_prefix_fanout"]
    assert "padt_kv_prefix_fanout_f16" in _lib.parse_header(_lib.HEADER_F16)
    assert len(decl[1]) == 24
    ok = dict(k_pre=16, v_pre=16, ld_pre=256, n_pre=50, pre_off=16, n_images=2, mem_image=16, mem_row=16, mem_join=16, n_members=3, max_p=40,
              k_cache=16, vt_cache=16, k_join=16, ld_kj=256, v_join=16, ld_vj=256, n_join=200, n_kv_heads=2, head_dim=128, s_max=64, batch=5,
              cache_packed=1)
    for name in ("padt_kv_prefix_fanout", "padt_kv_prefix_fanout_f16"):
        fn = getattr(lib, name)
        for bad, msg in ((dict(k_pre=None), b"null pointer"), (dict(mem_join=None), b"null pointer"), (dict(v_join=None), b"null pointer"),
                         (dict(n_pre=0), b"bad dimensions"), (dict(n_members=65536), b"bad dimensions"), (dict(n_images=0), b"bad dimensions"),
                         (dict(batch=0), b"bad dimensions"), (dict(head_dim=258), b"head_dim must be even"), (dict(head_dim=63), b"head_dim must be even"),
                         (dict(ld_pre=255), b"row stride is shorter"), (dict(ld_vj=128), b"row stride is shorter"),
                         (dict(head_dim=80, ld_pre=160, ld_kj=160, ld_vj=160), b"packed caches need"), (dict(s_max=72), b"packed caches need")):
            a = dict(ok, **bad)
            assert fn(None, *a.values()) == -1 and msg in lib.padt_last_error(), (name, bad)
        assert fn(None, *dict(ok, n_members=0).values()) == 0      # nothing to do: no launch
        assert fn(None, *dict(ok, max_p=0).values()) == 0
