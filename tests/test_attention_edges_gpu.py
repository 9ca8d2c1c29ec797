"""Attention kernels where attention kernels usually break, against fp64 statements of the same operation on the exact operands the kernel reads.

The parity tests of test_kernels_gpu.py / test_kernels_f16_gpu.py / test_decoder_hp_gpu.py draw q, k, v from randn: near-uniform scores, and the
keys just outside every visibility boundary hold ordinary values.  Here, for every attention entry point (attn_varlen, decode_attn,
decode_attn_rope row-major and on fragment-packed caches at DS = 1 / 2, attn_f32 VALU / MFMA), in both 16-bit operand types:
  * score distributions (shape_scores): an attention sink 30 nats above every other key, a dominant key in the last, partial 64-key tile (and,
    for the packed decode kernel, in the range of its last wave), two tied maxima in different tiles / splits / waves, temperatures 0 (the
    output is the fp64 mean of v), 8 and 30, and q[0] = k[0] = 1000 at one key (a score around 1e5: the scale_log2 / exp2 path);
  * visibility boundaries: the keys just outside the visible set score 60 nats above every visible key and carry V rows of 1e4 — the causal
    diagonal, the neighbouring segments of cu_k, the next ViT window of the fused-RoPE path, the stale rows of a decode cache past len; at
    visible-key counts 64k - 1, 64k, 64k + 1, 512k + 1 and 1;
  * non-finite values outside the visible set (+inf / NaN, in K and, separately, in V): the outputs are bit-identical to a run with clean values;
  * a NaN inside the visible set (one q row; one K or V row): every (row, head) that sees it is non-finite and every other output of the launch
    is bit-identical to the clean run.  Exception, by construction of a shared-operand MFMA: a non-finite V row under a CAUSAL mask also reaches
    the queries of its own sample / segment and kv-head group that share its key tile without seeing it (0 x inf in O^T = V^T P^T, with one V^T
    fragment for all query columns).  Those rows are not asserted; every other row is ("Attention: what a key outside the visible
    set can do").

Tolerances are the suite's, unchanged: ulps = 6 of close_bf16 / close_f16 for the 16-bit kernels, split_close with its noise for attn_f32 —
except attn_f32 at temperatures 8 and 30, whose noise term gets the fp32 score-rounding term derived in test_attn_f32_score_distributions.
"""
import math

import pytest
import torch

from edge_util import same_bits
from test_decoder_hp_gpu import join, split_close
from test_kernels_f16_gpu import close_f16
from test_kernels_gpu import close_bf16, ref_attn

pytestmark = pytest.mark.gpu

BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
X16 = pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
DISTS = ["sink", "late", "tie", "t0", "t8", "t30", "huge"]
A = 4.0                    # q's planted coordinate (d = 0); a key with k[0] = gap * sqrt(D) / A scores `gap` nats above its randn score
POISON_GAP, POISON_V = 60.0, 1e4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------ helpers
def close16(out, ref, what):
    (close_bf16 if out.dtype == BF else close_f16)(out, ref, what, ulps=6)


def cum(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def late_key(n):
    """a key in the last, partial 64-key tile of n keys (the middle of it)"""
    return 64 * ((n - 1) // 64) + (n - 1) % 64 // 2


def last_wave_key(n):
    """the last key <= n - 1 with key = 7 * 64 (mod 512): the range of wave 7 of the packed decode kernel (NW = 8); else late_key"""
    return 448 + 512 * ((n - 1 - 448) // 512) if n > 448 else late_key(n)


def shape_scores(dist, q, k, segs, D):
    """Shape the scores of fp32 CPU operands q (rows, Hq, D) and k (keys, Hkv, D) in place; segs = [(first key, key count)] per segment / sample.
    sink: key 0 of every segment scores ~30 nats above the rest; late / late7: the dominant key sits in the last partial tile / in wave 7's range;
    tie: keys 0 and 64 (or the last key) hold the same K row and both dominate; t0 / t8 / t30: q scaled by 0 / 8 / 30; huge: q[0] = k[0] = 1000 at
    key 0 (a score of ~1e5 nats: m and s * scale_log2 of that size must still cancel exactly in exp2(s - m)).  Not random q / k of a few hundred:
    random scores of std ~4e4 put near-ties into some rows, and an fp32 score of that size is only known to ~1e-2 nats (2^-24 |s| per rounding) —
    no fp32 kernel can give the fp64 answer for such a row."""
    if dist in ("t0", "t8", "t30"):
        q.mul_(float(dist[1:]))
        return
    if dist == "huge":
        q[..., 0] = 1000.0
        k[..., 0] = 0.0
        for k0, n in segs:
            if n:
                k[k0, :, 0] = 1000.0
        return
    q[..., 0] = A
    k[..., 0] = 0.0
    b = 30.0 * math.sqrt(D) / A
    for k0, n in segs:
        if n == 0:
            continue
        keys = {"sink": [0], "late": [late_key(n)], "late7": [last_wave_key(n)],
                "tie": [0, 64] if n > 64 else sorted({0, n - 1})}[dist]
        for j in keys:
            k[k0 + j, :, 0] = b
        if len(keys) == 2:
            k[k0 + keys[1]] = k[k0 + keys[0]]


def poison_keys(k, v, keys, D, val=None, where=None):
    """val None: the keys score POISON_GAP nats above every (unshaped, q[..., 0] = A) visible key and carry V rows of POISON_V;
    else K (where = 'k') or V (where = 'v') rows of the keys := val (+inf / NaN)."""
    idx = torch.tensor(sorted(keys), dtype=torch.long)
    if val is None:
        k[idx, :, 0] = POISON_GAP * math.sqrt(D) / A
        v[idx] = POISON_V
    else:
        (k if where == "k" else v)[idx] = val


# ------------------------------------------------------------------------------------------------------------ attn_varlen
VARLEN = {
    "vit_window": dict(D=80, H=16, Hkv=16, lq=[64, 36, 48, 64]),
    "vit_full": dict(D=80, H=4, Hkv=4, lq=[2116]),
    "gqa16_2": dict(D=128, H=16, Hkv=2, lq=[577, 65, 1, 64], causal=True),
    "gqa28_4": dict(D=128, H=28, Hkv=4, lq=[513, 63, 7], causal=True),
    "cross_q2img": dict(D=80, H=16, Hkv=16, lq=[8, 5, 10], lk=[529, 345, 16]),
    "cross_img2q": dict(D=80, H=16, Hkv=16, lq=[300, 64], lk=[8, 7]),
    "rope_window": dict(D=80, H=16, Hkv=16, lq=[64, 36, 48, 64], rope=True),
}


def rope_tables(T, D, seed):
    """fp32 [T][D] cos / sin of random angles; pair 0 (d = 0, D/2) is not rotated, so a score planted in d = 0 stays where it was planted"""
    ang = torch.rand(T, D // 2, generator=torch.Generator().manual_seed(seed)) * 40
    ang[:, 0] = 0
    emb = torch.cat([ang, ang], -1).cuda()
    return emb.cos().contiguous(), emb.sin().contiguous()


def varlen_operands(c, seed):
    lq = c["lq"]
    lk = c.get("lk") or lq
    g = torch.Generator().manual_seed(seed)
    q, k, v = randn(g, sum(lq), c["H"], c["D"]), randn(g, sum(lk), c["Hkv"], c["D"]), randn(g, sum(lk), c["Hkv"], c["D"])
    return q, k, v, cum(lq), cum(lk)


def run_varlen(ops, c, dt, q, k, v, cq, ck, seed=0):
    """-> kernel output and the 16-bit q / k / v the reference reads (fused RoPE: the stand-alone rope_half kernel's rotated q / k)"""
    D, H, Hkv = c["D"], c["H"], c["Hkv"]
    qx, kx, vx = (t.reshape(t.shape[0], -1).to(dt).cuda() for t in (q, k, v))
    out = torch.zeros(qx.shape[0], H * D, dtype=dt, device="cuda")
    rope, qr, kr = None, qx, kx
    cqt = i32(cq)
    ckt = cqt if c.get("rope") else i32(ck)                   # fused RoPE wants ONE cu tensor (self-attention)
    if c.get("rope"):
        rope = rope_tables(qx.shape[0], D, seed)
        qr, kr = qx.clone(), kx.clone()
        ops.rope_half_(qr, rope[0], rope[1], H, D)
        ops.rope_half_(kr, rope[0], rope[1], Hkv, D)
    ops.attn_varlen(qx, kx, vx, out, cqt, ckt, max(cq[i + 1] - cq[i] for i in range(len(cq) - 1)), H, Hkv, D,
                    causal=c.get("causal", False), rope=rope)
    return out, qr, kr, vx


@X16
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("name", list(VARLEN))
def test_attn_varlen_score_distributions(ops, name, dist, dt):
    c = VARLEN[name]
    q, k, v, cq, ck = varlen_operands(c, seed=1)
    shape_scores(dist, q, k, list(zip(ck[:-1], [ck[i + 1] - ck[i] for i in range(len(ck) - 1)])), c["D"])
    out, qr, kr, vx = run_varlen(ops, c, dt, q, k, v, cq, ck)
    ref = ref_attn(qr, kr, vx, cq, ck, c["H"], c["Hkv"], c["D"], c.get("causal", False), dtype=F64)
    close16(out, ref, f"attn_varlen {name} {dist}")
    if dist == "t0" and not c.get("causal"):                  # exactly uniform: the fp64 mean of each segment's v
        mean = torch.cat([vx[ck[i]:ck[i + 1]].double().view(-1, c["Hkv"], c["D"]).mean(0).repeat_interleave(c["H"] // c["Hkv"], 0)
                          .reshape(1, -1).expand(cq[i + 1] - cq[i], -1) for i in range(len(cq) - 1)])
        close16(out, mean, f"attn_varlen {name}: uniform scores")


# Visibility layouts.  seg: (lq, lk, role): 'v' victim (its rows are compared), 's' spacer (its keys are the poison, its rows are not compared);
# diag: (lq, lk, p): causal segment whose key p is poisoned — the query at position p - shift - 1 sees exactly p keys.
BOUNDARY = {
    # neighbouring segments of cu_k: 0-query spacers of 2 keys around every victim
    "segments_cross": dict(D=80, H=16, Hkv=16, seg=[(0, 2, "s"), (8, 63, "v"), (0, 2, "s"), (5, 64, "v"), (0, 2, "s"), (10, 65, "v"),
                                                    (0, 2, "s"), (3, 513, "v"), (0, 2, "s"), (4, 1, "v"), (0, 2, "s")]),
    "segments_causal": dict(D=128, H=16, Hkv=2, causal=True, seg=[(4, 4, "s"), (63, 63, "v"), (4, 4, "s"), (64, 64, "v"), (4, 4, "s"),
                                                                  (65, 65, "v"), (4, 4, "s"), (513, 513, "v"), (4, 4, "s"), (1, 1, "v"), (4, 4, "s")]),
    # the next / previous ViT window on the fused-RoPE path
    "rope_windows": dict(D=80, H=16, Hkv=16, rope=True, seg=[(8, 8, "s"), (63, 63, "v"), (8, 8, "s"), (64, 64, "v"), (8, 8, "s"), (65, 65, "v"),
                                                             (8, 8, "s"), (36, 36, "v"), (8, 8, "s"), (1, 1, "v"), (8, 8, "s")]),
    # the causal diagonal, self (shift 0) and bottom-right aligned (lk > lq)
    "causal_diag": dict(D=128, H=16, Hkv=2, causal=True, diag=[(2, 2, 1), (66, 66, 63), (66, 66, 64), (67, 67, 65), (515, 515, 513),
                                                               (40, 104, 65)]),
    "causal_diag_28_4": dict(D=128, H=28, Hkv=4, causal=True, diag=[(2, 2, 1), (66, 66, 64), (67, 67, 65), (515, 515, 513)]),
}


def boundary_layout(c):
    """-> lq, lk, victim row mask list [(row0, row1)], poison keys (absolute), and per diag segment (q0, k0, lq, lk, p)"""
    if "seg" in c:
        lq, lk = [s[0] for s in c["seg"]], [s[1] for s in c["seg"]]
        cq, ck = cum(lq), cum(lk)
        victims = [(cq[i], cq[i + 1]) for i, s in enumerate(c["seg"]) if s[2] == "v"]
        poison = [j for i, s in enumerate(c["seg"]) if s[2] == "s" for j in range(ck[i], ck[i + 1])]
        return lq, lk, victims, poison, []
    lq, lk = [s[0] for s in c["diag"]], [s[1] for s in c["diag"]]
    cq, ck = cum(lq), cum(lk)
    diag = [(cq[i], ck[i], s[0], s[1], s[2]) for i, s in enumerate(c["diag"])]
    return lq, lk, [], [ck[i] + s[2] for i, s in enumerate(c["diag"])], diag


def check_boundary_rows(out, ref, victims, diag, what, close):
    """one comparison over every victim row of the launch (the suite's bounds take the rms of a launch's output); causal diagonals: the rows
    blind to the poisoned key p (the last of them sees exactly p keys), and separately the rows that see it (outputs ~1e4)"""
    rows = [r for r0, r1 in victims for r in range(r0, r1)]
    blind = [q0 + i for q0, k0, nq, nk, p in diag for i in range(min(nq, p - (nk - nq)))]
    seeing = [q0 + i for q0, k0, nq, nk, p in diag for i in range(max(0, p - (nk - nq)), nq)]
    for sel, which in ((rows, "rows next to poisoned segments"), (blind, "rows blind to the poisoned key"), (seeing, "rows that see it")):
        if sel:
            close(out[sel], ref[sel], f"{what}: {which}")


@X16
@pytest.mark.parametrize("name", list(BOUNDARY))
def test_attn_varlen_keys_outside_the_visible_set_would_win(ops, name, dt):
    c = BOUNDARY[name]
    lq, lk, victims, poison, diag = boundary_layout(c)
    q, k, v, cq, ck = varlen_operands(dict(c, lq=lq, lk=lk), seed=2)
    q[..., 0] = A
    k[..., 0] = 0.0
    poison_keys(k, v, poison, c["D"])
    out, qr, kr, vx = run_varlen(ops, dict(c, lq=lq, lk=lk), dt, q, k, v, cq, ck)
    ref = ref_attn(qr, kr, vx, cq, ck, c["H"], c["Hkv"], c["D"], c.get("causal", False), dtype=F64)
    check_boundary_rows(out, ref, victims, diag, f"attn_varlen {name}", close16)


@X16
@pytest.mark.parametrize("where", ["k", "v"])
@pytest.mark.parametrize("val", [math.inf, math.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("name", ["segments_cross", "segments_causal", "rope_windows"])
def test_attn_varlen_non_finite_keys_outside_the_visible_set(ops, name, val, where, dt):
    c = BOUNDARY[name]
    lq, lk, victims, poison, _ = boundary_layout(c)
    cc = dict(c, lq=lq, lk=lk)
    q, k, v, cq, ck = varlen_operands(cc, seed=3)
    clean, *_ = run_varlen(ops, cc, dt, q, k, v, cq, ck)
    poison_keys(k, v, poison, c["D"], val, where)
    out, *_ = run_varlen(ops, cc, dt, q, k, v, cq, ck)
    for r0, r1 in victims:
        assert same_bits(out[r0:r1], clean[r0:r1]), f"{name}: {val} in {where} of a neighbouring segment changed rows {r0}..{r1}"


def seen_mask(nrows, H, D, cq, ck, group, causal, what, seg, pos, head):
    """(rows, H*D) bool: the outputs that see a NaN planted at q row (seg, pos, head) or at key (seg, pos) of kv head `head`"""
    m = torch.zeros(nrows, H, D, dtype=torch.bool)
    q0, nq, nk = cq[seg], cq[seg + 1] - cq[seg], ck[seg + 1] - ck[seg]
    if what == "q":
        m[q0 + pos, head] = True
    else:
        rows = [i for i in range(nq) if not causal or pos <= i + nk - nq]
        for i in rows:
            m[q0 + i, head * group:(head + 1) * group] = True
    return m.view(nrows, H * D).cuda()


def leak_mask(nrows, H, D, cq, group, seg, head):
    """causal + NaN in V: the rows of the same segment and kv-head group (shared V^T fragment, 0 x NaN), not asserted"""
    m = torch.zeros(nrows, H, D, dtype=torch.bool)
    m[cq[seg]:cq[seg + 1], head * group:(head + 1) * group] = True
    return m.view(nrows, H * D).cuda()


def check_nan_spread(out, clean, seen, leak, what):
    bad = ~torch.isfinite(out.float())
    assert bad[seen].all(), f"{what}: {int((~bad[seen]).sum())} of {int(seen.sum())} outputs that see the NaN are finite"
    keep = ~seen if leak is None else ~(seen | leak)
    assert same_bits(out[keep], clean[keep]), f"{what}: outputs that do not see the NaN changed ({int((out[keep] != clean[keep]).sum())} differ)"


NAN_VARLEN = {"gqa16_2": (1, 40), "vit_window": (2, 5), "cross_q2img": (0, 300), "rope_window": (1, 20)}   # (segment, position)


@X16
@pytest.mark.parametrize("what", ["q", "k", "v"])
@pytest.mark.parametrize("name", list(NAN_VARLEN))
def test_attn_varlen_nan_inside_the_visible_set(ops, name, what, dt):
    c = VARLEN[name]
    seg, pos = NAN_VARLEN[name]
    if what == "q":
        pos = min(pos, c["lq"][seg] - 1)
    D, H, Hkv = c["D"], c["H"], c["Hkv"]
    q, k, v, cq, ck = varlen_operands(c, seed=4)
    clean, *_ = run_varlen(ops, c, dt, q, k, v, cq, ck)
    head = 1
    if what == "q":
        q[cq[seg] + pos, head, 3] = math.nan
    else:
        (k if what == "k" else v)[ck[seg] + pos, head, 3] = math.nan
    out, *_ = run_varlen(ops, c, dt, q, k, v, cq, ck)
    causal = c.get("causal", False)
    if what == "v":                                           # a NaN in one d column of V: only that column of the rows that see it
        seen = seen_mask(out.shape[0], H, D, cq, ck, H // Hkv, causal, what, seg, pos, head).view(-1, H, D)
        seen[..., :3] = False
        seen[..., 4:] = False
        seen = seen.view(out.shape[0], H * D)
    else:
        seen = seen_mask(out.shape[0], H, D, cq, ck, H // Hkv, causal, what, seg, pos, head)
    leak = leak_mask(out.shape[0], H, D, cq, H // Hkv, seg, head) if (what == "v" and causal) else None
    check_nan_spread(out, clean, seen, leak, f"attn_varlen {name}: NaN in {what}")


# ------------------------------------------------------------------------------------------------------------ decode attention
def decode_ref(q, kc, vt, lens, Hq, Hkv, D):
    """fp64: q (B, Hq*D), kc (B, Hkv, S, D), vt (B, Hkv, D, S) — keys [0, len) of each sample"""
    B, rep = q.shape[0], Hq // Hkv
    ref = torch.zeros(B, Hq * D, dtype=F64, device="cuda")
    for b in range(B):
        kk = kc[b, :, :lens[b]].double().repeat_interleave(rep, 0)
        vv = vt[b, :, :, :lens[b]].double().transpose(1, 2).repeat_interleave(rep, 0)
        sc = torch.einsum("hd,hld->hl", q[b].double().view(Hq, D), kk) * D ** -0.5
        ref[b] = torch.einsum("hl,hld->hd", torch.softmax(sc, -1), vv).reshape(-1)
    return ref


DEC = {"d32": (32, 4, 2), "d128": (128, 16, 2)}              # (D, Hq, Hkv)
DEC_LENS, DEC_S = [1, 63, 64, 65, 513], 576


def decode_operands(D, Hq, Hkv, lens, S, seed):
    """fp32 CPU: q (B, Hq, D), keys / values (B*S, Hkv, D) — sample b's key j at row b*S + j"""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    return randn(g, B, Hq, D), randn(g, B * S, Hkv, D), randn(g, B * S, Hkv, D)


def caches(k, v, B, S, dt):
    Hkv, D = k.shape[1], k.shape[2]
    kc = k.view(B, S, Hkv, D).permute(0, 2, 1, 3).to(dt).cuda().contiguous()
    vt = v.view(B, S, Hkv, D).permute(0, 2, 3, 1).to(dt).cuda().contiguous()
    return kc, vt


def run_decode(ops, dt, D, Hq, Hkv, q, k, v, lens, S):
    B = len(lens)
    kc, vt = caches(k, v, B, S, dt)
    qx = q.reshape(B, -1).to(dt).cuda()
    out = torch.zeros(B, Hq * D, dtype=dt, device="cuda")
    ops.decode_attn(qx, kc, vt, i32(lens), out, ops.new_decode_workspace(B, Hkv, D, S, "cuda"), Hq, Hkv, D, S, max(lens))
    return out, qx, kc, vt


@X16
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("shape", list(DEC))
def test_decode_attn_score_distributions(ops, shape, dist, dt):
    D, Hq, Hkv = DEC[shape]
    q, k, v = decode_operands(D, Hq, Hkv, DEC_LENS, DEC_S, seed=5)
    shape_scores(dist, q, k, [(b * DEC_S, n) for b, n in enumerate(DEC_LENS)], D)
    out, qx, kc, vt = run_decode(ops, dt, D, Hq, Hkv, q, k, v, DEC_LENS, DEC_S)
    close16(out, decode_ref(qx, kc, vt, DEC_LENS, Hq, Hkv, D), f"decode_attn {shape} {dist}")


# decode_attn_rope: slot = len - 1 is appended from the qkv row.  The rotation runs at position 0 for the shaped-score tests (cos 1, sin 0: a
# planted score stays planted) and at random positions elsewhere; the reference always reads the prompt kernel's (llm_qkv_post) q and caches.
ROPE_MODES = {"rowmajor": False, "packed_ds1": 2, "packed_ds2": 3}
RD, RHQ, RHKV, RSEC = 128, 16, 2, (16, 24, 24)
R_SLOTS, R_S = [0, 62, 63, 64, 512, 1289], 1344


def rope_decode_inputs(q, k, v, slots, S, dt, positions_seed=None):
    """fp32 CPU q (B, Hq, D) and keys / values (B*S, Hkv, D) -> qkv rows (the fresh k / v = key `slot`), caches, pos3"""
    B = len(slots)
    Hkv, D = k.shape[1], k.shape[2]
    kn = torch.stack([k[b * S + s] for b, s in enumerate(slots)])
    vn = torch.stack([v[b * S + s] for b, s in enumerate(slots)])
    qkv = torch.cat([q.reshape(B, -1), kn.reshape(B, -1), vn.reshape(B, -1)], 1).to(dt).cuda()
    kc, vt = caches(k, v, B, S, dt)
    if positions_seed is None:
        pos = torch.zeros(3, B, dtype=torch.int32, device="cuda")
    else:
        pos = torch.randint(0, 4000, (3, B), dtype=torch.int32, generator=torch.Generator().manual_seed(positions_seed)).cuda()
    return qkv, kc, vt, pos


def run_decode_rope(ops, mode, qkv, kc, vt, pos, slots, S, Hq=RHQ, Hkv=RHKV, D=RD):
    """-> output, and the prompt kernel's rotated q + appended row-major caches (the reference's operands)"""
    B = len(slots)
    dt = qkv.dtype
    inv = (1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))).cuda()
    cs = torch.zeros(B, D // 2, 2, device="cuda")
    ops.rope_table(pos, inv, cs, D, RSEC)
    slot_t = i32(slots)
    out = torch.zeros(B, Hq * D, dtype=dt, device="cuda")
    cp = ROPE_MODES[mode]
    if cp:
        ops.decode_attn_rope(qkv, cs, slot_t, ops.pack_k_cache(kc), ops.pack_vt_cache(vt), out, None, Hq, Hkv, D, S, S, cache_packed=cp)
    else:
        ops.decode_attn_rope(qkv, cs, slot_t, kc.clone(), vt.clone(), out, ops.new_decode_workspace(B, Hkv, D, S, "cuda"), Hq, Hkv, D, S, S)
    qr, kr, vr = torch.zeros(B, Hq * D, dtype=dt, device="cuda"), kc.clone(), vt.clone()
    ops.llm_qkv_post(qkv, pos, inv, qr, kr, vr, Hq, Hkv, D, S, RSEC, slot=slot_t)
    return out, qr, kr, vr


@X16
@pytest.mark.parametrize("dist", DISTS + ["late7"])
@pytest.mark.parametrize("mode", list(ROPE_MODES))
def test_decode_attn_rope_score_distributions(ops, mode, dist, dt):
    q, k, v = decode_operands(RD, RHQ, RHKV, R_SLOTS, R_S, seed=6)
    lens = [s + 1 for s in R_SLOTS]
    shape_scores(dist, q, k, [(b * R_S, n) for b, n in enumerate(lens)], RD)
    qkv, kc, vt, pos = rope_decode_inputs(q, k, v, R_SLOTS, R_S, dt)
    out, qr, kr, vr = run_decode_rope(ops, mode, qkv, kc, vt, pos, R_SLOTS, R_S)
    close16(out, decode_ref(qr, kr, vr, lens, RHQ, RHKV, RD), f"decode_attn_rope {mode} {dist}")


# every decode entry point: (kind, D, Hq, Hkv)
DEC_ENTRIES = {"decode_attn_d32": ("plain", 32, 4, 2), "decode_attn_d128": ("plain", 128, 16, 2),
               "rope_rowmajor": ("rowmajor", 128, 16, 2), "rope_packed_ds1": ("packed_ds1", 128, 16, 2), "rope_packed_ds2": ("packed_ds2", 128, 16, 2)}


def run_entry(ops, entry, dt, q, k, v, lens, S, positions_seed=7):
    """-> output and the reference's operands (q, row-major K cache, V^T cache)"""
    kind, D, Hq, Hkv = DEC_ENTRIES[entry]
    if kind == "plain":
        out, qx, kc, vt = run_decode(ops, dt, D, Hq, Hkv, q, k, v, lens, S)
        return out, qx, kc, vt
    slots = [n - 1 for n in lens]
    qkv, kc, vt, pos = rope_decode_inputs(q, k, v, slots, S, dt, positions_seed)
    return run_decode_rope(ops, kind, qkv, kc, vt, pos, slots, S, Hq, Hkv, D)


def stale_rows(lens, S):
    return [b * S + j for b, n in enumerate(lens) for j in range(n, S)]


@X16
@pytest.mark.parametrize("entry", list(DEC_ENTRIES))
def test_decode_stale_cache_rows_would_win(ops, entry, dt):
    """cache rows len .. S_max-1 score 60 nats above every visible key and hold V = 1e4: the output is the fp64 attention over [0, len)."""
    _, D, Hq, Hkv = DEC_ENTRIES[entry]
    lens, S = ([1, 63, 64, 65, 513], 576) if D == 32 or "decode_attn" in entry else ([1, 63, 64, 65, 513, 1025], 1088)
    q, k, v = decode_operands(D, Hq, Hkv, lens, S, seed=8)
    q[..., 0] = A
    k[..., 0] = 0.0
    poison_keys(k, v, stale_rows(lens, S), D)
    out, qr, kr, vr = run_entry(ops, entry, dt, q, k, v, lens, S, positions_seed=None)   # position 0: the planted scores are not rotated away
    close16(out, decode_ref(qr, kr, vr, lens, Hq, Hkv, D), f"{entry}: stale rows past len")


@X16
@pytest.mark.parametrize("where", ["k", "v"])
@pytest.mark.parametrize("val", [math.inf, math.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("entry", list(DEC_ENTRIES))
def test_decode_non_finite_stale_cache_rows(ops, entry, val, where, dt):
    """+inf / NaN in the K or V rows past len (a reused session cache after an overflowed batch): outputs bit-identical to clean rows there."""
    _, D, Hq, Hkv = DEC_ENTRIES[entry]
    lens, S = [1, 63, 64, 65, 513], 576
    q, k, v = decode_operands(D, Hq, Hkv, lens, S, seed=9)
    clean, *_ = run_entry(ops, entry, dt, q, k, v, lens, S)
    poison_keys(k, v, stale_rows(lens, S), D, val, where)
    out, *_ = run_entry(ops, entry, dt, q, k, v, lens, S)
    diff = [b for b in range(len(lens)) if not same_bits(out[b], clean[b])]
    assert not diff, f"{entry}: {val} in the {where} rows past len changed the outputs of samples with len {[lens[b] for b in diff]}"


@X16
@pytest.mark.parametrize("what", ["q", "k", "v"])
@pytest.mark.parametrize("entry", list(DEC_ENTRIES))
def test_decode_nan_inside_the_visible_set(ops, entry, what, dt):
    """A NaN in one q head (the range guard's overflow marker) or in one visible K / V row of one sample: that sample's rows that see it are
    non-finite, every other output is bit-identical."""
    _, D, Hq, Hkv = DEC_ENTRIES[entry]
    lens, S = [1, 63, 64, 65, 513], 576
    q, k, v = decode_operands(D, Hq, Hkv, lens, S, seed=10)
    clean, *_ = run_entry(ops, entry, dt, q, k, v, lens, S)
    b, j, g = 3, 64, 1                                        # sample 3 (len 65): key 64 is its fresh token on the rope paths
    if what == "q":
        q[b, g * (Hq // Hkv) + 1, 5] = math.nan
    else:
        (k if what == "k" else v)[b * S + j, g, 5] = math.nan
    out, *_ = run_entry(ops, entry, dt, q, k, v, lens, S)
    seen = torch.zeros(len(lens), Hq, D, dtype=torch.bool)
    if what == "q":
        seen[b, g * (Hq // Hkv) + 1] = True
    elif what == "k":
        seen[b, g * (Hq // Hkv):(g + 1) * (Hq // Hkv)] = True
    else:
        seen[b, g * (Hq // Hkv):(g + 1) * (Hq // Hkv), 5] = True
    check_nan_spread(out, clean, seen.view(len(lens), -1).cuda(), None, f"{entry}: NaN in {what}")


@pytest.mark.parametrize("mode", ["rowmajor", "packed"])
def test_decode_attn_rope_fp16_session_reuse_after_an_overflowed_batch(ops, mode):
    """LLM.session() reuses a lane's fp16 caches across batches.  A batch whose v overflowed (inf) and whose k overflowed through rope_fin (NaN)
    appends such rows; the next, shorter batch on the same buffers must produce finite rows that padt_check_finite does not flag."""
    D, Hq, Hkv, S, B = RD, RHQ, RHKV, 704, 3
    g = torch.Generator().manual_seed(11)
    kc = torch.randn(B, Hkv, S, D, generator=g).to(F16).cuda()
    vt = torch.randn(B, Hkv, D, S, generator=g).to(F16).cuda()
    packed = mode == "packed"
    if packed:
        kc, vt = ops.pack_k_cache(kc), ops.pack_vt_cache(vt)
    inv = (1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))).cuda()
    cs = torch.zeros(B, D // 2, 2, device="cuda")
    ws = None if packed else ops.new_decode_workspace(B, Hkv, D, S, "cuda")
    out = torch.zeros(B, Hq * D, dtype=F16, device="cuda")
    pos = torch.randint(0, 4000, (3, B), dtype=torch.int32, generator=torch.Generator().manual_seed(12)).cuda()
    ops.rope_table(pos, inv, cs, D, RSEC)
    for t in range(8):                                        # the overflowed batch: 8 steps of inf v and of k beyond fp16 after the rotation
        qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).to(F16).cuda()
        qkv[:, Hq * D:(Hq + Hkv) * D] = 6e4
        qkv[:, (Hq + Hkv) * D:] = math.inf
        ops.decode_attn_rope(qkv, cs, i32([600 + t, 10 + t, 100 + t]), kc, vt, out, ws, Hq, Hkv, D, S, S, cache_packed=packed)
    flags = torch.zeros(B, dtype=torch.int32, device="cuda")
    ops.check_finite(out, flags, rows_per_flag=1)
    assert flags.tolist() == [1, 1, 1], "the overflowed batch itself must be flagged"
    stale = (ops.unpack_vt_cache(vt) if packed else vt)[0, 0, 0, 600:608].float()
    assert torch.isinf(stale).all(), "the overflowed batch left no inf rows behind"
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).to(F16).cuda()
    ops.decode_attn_rope(qkv, cs, i32([590, 0, 96]), kc, vt, out, ws, Hq, Hkv, D, S, S, cache_packed=packed)   # 600..607 / 10..17 / 100..107 sit
    flags.zero_()                                                                                               # in each sample's last split
    ops.check_finite(out, flags, rows_per_flag=1)
    assert flags.tolist() == [0, 0, 0], f"a clean batch over stale overflowed rows was flagged: {flags.tolist()}"


# ------------------------------------------------------------------------------------------------------------ attn_f32 (VALU qfew / kfew, MFMA)
F32_CASES = {
    "self_qfew": dict(D=80, H=16, Hkv=16, lq=[64, 36, 48]),
    "cross_q2img": dict(D=80, H=16, Hkv=16, lq=[8, 5, 10], lk=[529, 345, 16]),
    "cross_img2q_kfew": dict(D=80, H=16, Hkv=16, lq=[300, 64], lk=[8, 7]),
    "causal_gqa_kfew": dict(D=128, H=16, Hkv=2, lq=[577, 65, 1], causal=True),
    "causal_gqa_qfew": dict(D=128, H=16, Hkv=2, lq=[40, 7, 64], causal=True),
    "cache": dict(D=128, H=16, Hkv=2, cache=([1, 63, 64, 65, 513], 576)),
}
MFMA = pytest.mark.parametrize("mfma", [False, True], ids=["valu", "mfma"])


def f32_operands(c, seed):
    if "cache" in c:
        lens, S = c["cache"]
        q, k, v = decode_operands(c["D"], c["H"], c["Hkv"], lens, S, seed)
        return q, k, v, list(range(len(lens) + 1)), [b * S for b in range(len(lens) + 1)]
    return varlen_operands(c, seed)


def key_segs(c, ck):
    if "cache" in c:
        lens, S = c["cache"]
        return [(b * S, n) for b, n in enumerate(lens)]
    return [(ck[i], ck[i + 1] - ck[i]) for i in range(len(ck) - 1)]


def run_f32(ops, c, q, k, v, cq, ck, mfma):
    D, H, Hkv = c["D"], c["H"], c["Hkv"]
    qx, kx, vx = (t.reshape(t.shape[0], -1).cuda().contiguous() for t in (q, k, v))
    len_k = i32(c["cache"][0]) if "cache" in c else None
    mq = max(cq[i + 1] - cq[i] for i in range(len(cq) - 1))
    mk = c["cache"][1] if "cache" in c else max(ck[i + 1] - ck[i] for i in range(len(ck) - 1))
    out = ops.attn_f32(qx, kx, vx, i32(cq), i32(ck), mq, max(mk, 1), H, D, kv_group=H // Hkv, causal=c.get("causal", False), len_k=len_k, mfma=mfma)
    return out, qx, kx, vx


def ref_f32(c, qx, kx, vx, cq, ck):
    if "cache" in c:
        lens, S = c["cache"]
        return torch.cat([ref_attn(qx[b:b + 1], kx[b * S:b * S + n], vx[b * S:b * S + n], [0, 1], [0, n], c["H"], c["Hkv"], c["D"], False, dtype=F64)
                          for b, n in enumerate(lens)])
    return ref_attn(qx, kx, vx, cq, ck, c["H"], c["Hkv"], c["D"], c.get("causal", False), dtype=F64)


def f32_close(mfma):
    return lambda got, ref, what: split_close(got, ref, what, noise=8e-6 if mfma else 2e-6)


@MFMA
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("name", list(F32_CASES))
def test_attn_f32_score_distributions(ops, name, dist, mfma):
    c = F32_CASES[name]
    q, k, v, cq, ck = f32_operands(c, seed=12)
    shape_scores(dist, q, k, key_segs(c, ck), c["D"])
    out, qx, kx, vx = run_f32(ops, c, q, k, v, cq, ck, mfma)
    ref = ref_f32(c, qx, kx, vx, cq, ck)
    rows = [r for i in range(len(cq) - 1) if key_segs(c, ck)[i][1] > 0 for r in range(cq[i], cq[i + 1])]
    noise = 8e-6 if mfma else 2e-6
    if dist in ("t8", "t30"):
        # split_close's noise term is written for scores of O(1).  An fp32 score s = scale * q.k carries an absolute rounding error that grows with
        # its size: ~(sqrt(D) + 2) 2^-24 S, S = scale max|q| max|k| (Cauchy-Schwarz bound of |q.k| scale), and a score perturbation ds moves a
        # softmax average by at most ds * max|v|.  At t8 / t30 (S ~ 100-500) that is 1e-5 .. 1e-3 of the output, above 2e-6 x rms: added to the
        # noise term here, for these two temperatures only (measured 2e-5 .. 3.5e-5, ~30x inside it).
        D = c["D"]
        S = D ** -0.5 * qx.view(-1, D).norm(dim=1).max().item() * kx.view(-1, D).norm(dim=1).max().item()
        ds = (math.sqrt(D) + 2) * 2.0 ** -24 * S
        noise += ds * vx.abs().max().item() / ref[rows].pow(2).mean().sqrt().item()
    split_close(join(out, c["H"] * c["D"])[rows], ref[rows], f"attn_f32 {name} {dist}", noise=noise)


F32_BOUNDARY = {
    "segments_cross": BOUNDARY["segments_cross"],             # few queries (qfew)
    "segments_kfew": dict(D=80, H=16, Hkv=16, seg=[(0, 2, "s"), (300, 63, "v"), (0, 2, "s"), (100, 64, "v"), (0, 2, "s"), (70, 65, "v"),
                                                   (0, 2, "s"), (80, 1, "v"), (0, 2, "s")]),
    "causal_diag": BOUNDARY["causal_diag"],                   # max_q > 64: kfew
    "causal_diag_qfew": dict(D=128, H=16, Hkv=2, causal=True, diag=[(2, 2, 1), (64, 64, 63), (40, 104, 65)]),
    "cache": dict(D=128, H=16, Hkv=2, cache=([1, 63, 64, 65, 513], 576)),
}


def f32_boundary_layout(c):
    if "cache" in c:
        lens, S = c["cache"]
        return None, None, [(b, b + 1) for b in range(len(lens))], stale_rows(lens, S), []
    return boundary_layout(c)


@MFMA
@pytest.mark.parametrize("name", list(F32_BOUNDARY))
def test_attn_f32_keys_outside_the_visible_set_would_win(ops, name, mfma):
    c = F32_BOUNDARY[name]
    lq, lk, victims, poison, diag = f32_boundary_layout(c)
    cc = c if lq is None else dict(c, lq=lq, lk=lk)
    q, k, v, cq, ck = f32_operands(cc, seed=13)
    q[..., 0] = A
    k[..., 0] = 0.0
    poison_keys(k, v, poison, c["D"])
    out, qx, kx, vx = run_f32(ops, cc, q, k, v, cq, ck, mfma)
    check_boundary_rows(join(out, c["H"] * c["D"]), ref_f32(cc, qx, kx, vx, cq, ck), victims, diag, f"attn_f32 {name}", f32_close(mfma))


@MFMA
@pytest.mark.parametrize("where", ["k", "v"])
@pytest.mark.parametrize("val", [math.inf, math.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("name", ["segments_cross", "segments_kfew", "cache"])
def test_attn_f32_non_finite_keys_outside_the_visible_set(ops, name, val, where, mfma):
    c = F32_BOUNDARY[name]
    lq, lk, victims, poison, _ = f32_boundary_layout(c)
    cc = c if lq is None else dict(c, lq=lq, lk=lk)
    q, k, v, cq, ck = f32_operands(cc, seed=14)
    clean, *_ = run_f32(ops, cc, q, k, v, cq, ck, mfma)
    poison_keys(k, v, poison, c["D"], val, where)
    out, *_ = run_f32(ops, cc, q, k, v, cq, ck, mfma)
    for r0, r1 in victims:
        assert same_bits(out[r0:r1], clean[r0:r1]), f"attn_f32 {name}: {val} in {where} outside the visible set changed rows {r0}..{r1}"


NAN_F32 = {"self_qfew": (1, 20), "causal_gqa_kfew": (1, 40), "causal_gqa_qfew": (0, 20), "cache": (3, 64)}


@MFMA
@pytest.mark.parametrize("what", ["q", "k", "v"])
@pytest.mark.parametrize("name", list(NAN_F32))
def test_attn_f32_nan_inside_the_visible_set(ops, name, what, mfma):
    c = F32_CASES[name]
    seg, pos = NAN_F32[name]
    D, H, Hkv = c["D"], c["H"], c["Hkv"]
    q, k, v, cq, ck = f32_operands(c, seed=15)
    out0, *_ = run_f32(ops, c, q, k, v, cq, ck, mfma)
    head = 1
    if what == "q":
        pos = min(pos, cq[seg + 1] - cq[seg] - 1)
        q[cq[seg] + pos, head, 3] = math.nan
    else:
        (k if what == "k" else v)[ck[seg] + pos, head, 3] = math.nan
    out1, *_ = run_f32(ops, c, q, k, v, cq, ck, mfma)
    got, clean = join(out1, H * D), join(out0, H * D)
    causal = c.get("causal", False)
    seen = seen_mask(got.shape[0], H, D, cq, ck, H // Hkv, causal, what, seg, pos, head)     # (cache: one query per sample, not causal)
    if what == "v":
        seen = seen.view(-1, H, D)
        seen[..., :3] = False
        seen[..., 4:] = False
        seen = seen.view(got.shape[0], H * D)
    leak = leak_mask(got.shape[0], H, D, cq, H // Hkv, seg, head) if (what == "v" and causal) else None
    bad = ~torch.isfinite(got)
    assert bad[seen].all(), f"attn_f32 {name}: {int((~bad[seen]).sum())} of {int(seen.sum())} outputs that see the NaN are finite"
    keep = ~seen if leak is None else ~(seen | leak)
    assert torch.equal(got[keep], clean[keep]), f"attn_f32 {name}: outputs that do not see the NaN changed"
