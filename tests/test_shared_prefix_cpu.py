"""generate(image_index=) — host side: the shared prompt plan against plan_prompt of the expanded inputs, the argument policy, and the
new entry point's argument validation (no device needed)."""
import os
from types import SimpleNamespace

import pytest
import torch

import padt_amd
from padt_amd import _lib
from padt_amd.llm import check_shared_destinations, plan_prompt, plan_prompt_shared
from shared_prefix_util import shared_case


@pytest.fixture(scope="module")
def case():
    cfg = padt_amd.small_test_config()
    return cfg, shared_case(cfg)


@pytest.mark.parametrize("row0,proto_row0", [(0, 0), (7, 61)])
def test_shared_plan_reproduces_the_expanded_plan(case, row0, proto_row0):
    cfg, c = case
    B = 7
    ids = c["ids"].clone()
    if proto_row0:                                                # a prompt VRT id: shifted with the batch's prototype rows, as plan_prompt does
        ids[3, -2] = cfg.vocab_size + 3
    full = plan_prompt(cfg, ids, c["am"], c["grid_x"], "cpu", row0=row0, proto_row0=proto_row0)
    plan = plan_prompt_shared(cfg, ids, c["am"], c["grid"], c["image_index"], "cpu", row0=row0, proto_row0=proto_row0)
    sh = plan.shared
    # everything downstream of the prompt pass reads the expanded plan
    assert plan.next_pos == full.next_pos and plan.lens == full.lens and plan.vrt_off == full.vrt_off and plan.L_pad == full.L_pad
    assert torch.equal(plan.rope_deltas, full.rope_deltas) and torch.equal(plan.cu, full.cu) and torch.equal(plan.last_idx, full.last_idx)
    assert torch.equal(plan.ids, full.ids) and torch.equal(plan.pos3, full.pos3)
    # the groups the case was built for
    assert [P for P, _ in sh.groups] == [c["prefix"][0], c["prefix"][1]] and [m for _, m in sh.groups] == [[0, 2, 5], [1, 4]]
    assert sh.prefix_of == [0, 1, 0, -1, 1, 0, -1]
    G = len(sh.groups)
    cu_q, cu_k, cu = sh.cu_q.tolist(), sh.cu_k.tolist(), full.cu.tolist()
    own = [cu_q[G + b + 1] - cu_q[G + b] for b in range(B)]
    assert own == c["own"] and {1, 2, 33} <= set(own)
    assert sh.ids.numel() == cu_q[-1] == sum(P for P, _ in sh.groups) + sum(own) < full.ids.numel()
    assert sh.max_q == max(max(own), max(P for P, _ in sh.groups))
    # merged-embedding rows of the UNIQUE images, as the expanded plan's img_index sees them through low_rows
    off_u = [0]
    for n in c["n_merged"]:
        off_u.append(off_u[-1] + n)
    d_off, d_sample, d_slot, d_row = (t.tolist() for t in (sh.dst_off, sh.dst_sample, sh.dst_slot, sh.dst_row))
    written = {}
    for t in range(sh.ids.numel()):
        for n in range(d_off[t], d_off[t + 1]):
            if d_sample[n] >= 0:
                assert (d_sample[n], d_slot[n]) not in written
                written[(d_sample[n], d_slot[n])] = t
    for b in range(B):
        g = sh.prefix_of[b]
        P = sh.groups[g][0] if g >= 0 else 0
        toks = list(range(cu_q[g], cu_q[g] + P)) if g >= 0 else []
        toks += list(range(cu_q[G + b], cu_q[G + b + 1]))
        lo, hi = cu[b], cu[b + 1]
        assert len(toks) == hi - lo == full.lens[b]
        t_idx = torch.tensor(toks)
        assert torch.equal(sh.ids[t_idx], full.ids[lo:hi])
        assert torch.equal(sh.pos3[:, t_idx], full.pos3[:, lo:hi])
        assert torch.equal(sh.unshare[lo:hi].long(), t_idx)
        # image rows: the same embedding row of the same image — the sample's own, or (a prefix) the first member's copy of it
        exp_img = full.img_index[lo:hi]
        got_img = sh.img_index[t_idx]
        assert torch.equal(got_img < 0, exp_img < 0)
        on = exp_img >= 0
        assert torch.equal(sh.low_rows[exp_img[on].long()], sh.low_rows[got_img[on].long()])
        if g < 0:
            assert torch.equal(exp_img, got_img)
        # every slot below len written exactly once, by the token that holds that position of the full row — and seen by the attention
        # at the same place of the sample's key segment [group prefix | own tokens]
        assert cu_k[G + b + 1] - cu_k[G + b] == full.lens[b]
        for j, t in enumerate(toks):
            assert written[(row0 + b, j)] == t
            assert any(d_sample[n] == row0 + b and d_slot[n] == j and d_row[n] == cu_k[G + b] + j for n in range(d_off[t], d_off[t + 1]))
    assert len(written) == sum(full.lens)
    # a prefix has a key segment of its own (causal self-attention of the prefix rows): join rows only, no cache destination
    for g, (P, members) in enumerate(sh.groups):
        assert cu_k[g + 1] - cu_k[g] == P
        for j in range(P):
            t = cu_q[g] + j
            dests = [(d_sample[n], d_slot[n], d_row[n]) for n in range(d_off[t], d_off[t + 1])]
            assert dests[0] == (-1, j, cu_k[g] + j) and [d[0] for d in dests[1:]] == [row0 + m for m in members]
    assert sorted(d_row) == list(range(sh.n_join))                # every join row written exactly once
    # per-sample expansion tables
    assert sh.low_rows.tolist() == [r for u in c["image_index"] for r in range(off_u[u], off_u[u + 1])]
    assert sh.patch_rows.numel() == c["pix_x"].shape[0] and torch.equal(c["pix"][sh.patch_rows.long()], c["pix_x"])
    check_shared_destinations(sh, row0 + B, max(full.lens))
    with pytest.raises(ValueError, match="outside the session"):
        check_shared_destinations(sh, row0 + B, max(full.lens) - 1)
    with pytest.raises(ValueError, match="outside the session"):
        check_shared_destinations(sh, row0 + B - 1, max(full.lens))
    sh.dst_host[1][1] = sh.dst_host[1][2]
    sh.dst_host[0][1] = sh.dst_host[0][2]
    with pytest.raises(ValueError, match="written twice"):
        check_shared_destinations(sh, row0 + B, max(full.lens))


def test_no_prefix_when_it_would_not_cover_the_image(case):
    """Two queries whose rows END with the image: the shortest row minus one stops inside the image tokens, so nothing is shared but the ViT."""
    cfg, c = case
    n = c["n_merged"][0]
    row = [5, 6, cfg.vision_start_token_id] + [cfg.image_token_id] * n
    ids = torch.tensor([row, row])
    plan = plan_prompt_shared(cfg, ids, None, c["grid"][:1], [0, 0], "cpu")
    assert plan.shared.groups == [] and plan.shared.ids.numel() == 2 * len(row) and plan.shared.low_rows.tolist() == list(range(n)) * 2
    assert plan.shared.grid_x.tolist() == [c["grid"][0].tolist()] * 2


def test_image_index_validation_messages(case):
    cfg, c = case
    args = (cfg, c["ids"], c["am"], c["grid"])
    with pytest.raises(ValueError, match="image_index has 6 entries for a batch of 7"):
        plan_prompt_shared(*args, c["image_index"][:6], "cpu")
    with pytest.raises(ValueError, match=r"image_index\[2\] = 3 is outside \[0, 3\)"):
        plan_prompt_shared(*args, [0, 1, 3, 2, 1, 0, 1], "cpu")
    with pytest.raises(ValueError, match=r"image_index\[0\] = -1 is outside"):
        plan_prompt_shared(*args, torch.tensor([-1, 1, 0, 2, 1, 0, 1]), "cpu")
    with pytest.raises(ValueError, match=r"no sample for image\(s\) \[2\]"):
        plan_prompt_shared(cfg, c["ids"][[0, 1, 2]], c["am"][[0, 1, 2]], c["grid"], [0, 1, 0], "cpu")
    with pytest.raises(ValueError, match="Image features and image tokens do not match"):
        plan_prompt_shared(*args, [0, 1, 0, 2, 1, 1, 1], "cpu")          # sample 5 carries image 0's 16 tokens, image 1 has 30
    plan = plan_prompt_shared(*args, torch.tensor(c["image_index"], dtype=torch.int32), "cpu")       # an int tensor is an index too
    assert plan.shared.n_images == 3


class _Launched(Exception):
    pass


def _model():
    """An uninitialised instance whose generate_launch reports what generate() resolved (the pattern of test_gen_rules_cpu.py)."""
    from padt_amd.modeling import PaDTForConditionalGeneration
    m = PaDTForConditionalGeneration.__new__(PaDTForConditionalGeneration)
    m.generation_config = SimpleNamespace(pad_token_id=0, repetition_penalty=1.0)

    def launch(input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens, do_sample, *a, **kw):
        raise _Launched(dict(kw, max_new_tokens=max_new_tokens, do_sample=do_sample))
    m.generate_launch = launch
    return m


def test_image_index_is_a_named_parameter_and_reaches_the_launch():
    for kw, want in ((dict(image_index=[0, 0]), [0, 0]), ({}, None)):
        with pytest.raises(_Launched) as e:
            _model().generate(input_ids=torch.zeros((2, 4), dtype=torch.long), max_new_tokens=3, **kw)
        assert e.value.args[0]["image_index"] == want


def test_reference_precision_rejects_image_index_by_name():
    from padt_amd.modeling import PaDTForConditionalGeneration
    m = PaDTForConditionalGeneration.__new__(PaDTForConditionalGeneration)
    m.generation_config = SimpleNamespace(pad_token_id=0, repetition_penalty=1.0)
    m.precision = "reference"
    with pytest.raises(NotImplementedError, match=r"image_index.*precision='reference'"):
        m.generate(input_ids=torch.zeros((2, 4), dtype=torch.long), max_new_tokens=3, image_index=[0, 0])


def test_runner_and_rec_batch_take_image_index():
    import inspect
    from padt_amd.pipeline import PipelinedRunner, rec_batch, sample_grids
    for fn in (PipelinedRunner.submit, rec_batch, padt_amd.modeling.PaDTForConditionalGeneration.generate_launch):
        p = inspect.signature(fn).parameters["image_index"]
        assert p.default is None
    g = torch.tensor([[1, 8, 8], [1, 6, 10]])
    assert sample_grids(g, [1, 0, 1]).tolist() == [[1, 6, 10], [1, 8, 8], [1, 6, 10]]
    assert sample_grids(g, torch.tensor([0, 0], dtype=torch.int32)).tolist() == [[1, 8, 8], [1, 8, 8]]


def test_entry_point_validates_without_device():
    if not os.path.exists(_lib.LIB_PATH):
        from padt_amd.build import build
        build()
    lib = _lib.load()
    assert lib.padt_abi_version() == 4                            # the ABI only grew
    for name in ("padt_llm_qkv_post_shared", "padt_llm_qkv_post_shared_f16"):
        fn = getattr(lib, name)
        # (stream, qkv, ld, pos3, inv_freq, q, ld_q, k_join, ld_kj, v_join, ld_vj, n_join, kc, vtc, off, sample, slot, row, T, Hq, Hkv, hd, s_max, batch, s0, s1, packed)
        ok = [None, 16, 768, 16, 16, 16, 512, 16, 128, 16, 128, 4, 16, 16, 16, 16, 16, 16, 0, 4, 1, 128, 96, 2, 16, 24, 1]
        assert fn(*ok) == 0                                       # no tokens: success, nothing launched

        def bad(**kw):
            a = list(ok)
            names = _lib.parse_header()["padt_llm_qkv_post_shared"][2]
            for k, v in kw.items():
                a[names.index(k)] = v
            return fn(*a)
        assert bad(qkv=None) == -1 and b"null pointer" in lib.padt_last_error()
        for ptr in ("pos3", "inv_freq", "q_out", "k_join", "v_join", "k_cache", "vt_cache", "dst_off", "dst_sample", "dst_slot", "dst_row"):
            assert bad(**{ptr: None}) == -1, ptr
        assert bad(head_dim=130, T=1) == -1                       # packed caches need head_dim % 32 == 0
        assert bad(head_dim=127) == -1 and b"head_dim" in lib.padt_last_error()
        assert bad(s_max=100, T=1) == -1 and b"packed" in lib.padt_last_error()
        assert bad(T=-1) == -1 and b"bad dimensions" in lib.padt_last_error()
        for k in ("n_join", "batch", "n_heads", "n_kv_heads", "s_max"):
            assert bad(**{k: 0}) == -1, k
        assert bad(sec0=40, sec1=30) == -1                        # sections past head_dim / 2
        assert bad(ld_qkv=512) == -1 and b"stride" in lib.padt_last_error()
        assert bad(ld_kj=64) == -1 and bad(ld_vj=64) == -1 and bad(ld_q=256) == -1
