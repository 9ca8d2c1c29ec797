"""Token selection against exact references: every kernel a token id comes out of (csrc/vrt_head.hip), at the shapes, types and edges where
it could go wrong without the end-to-end tests noticing.

  * padt_vrt_head in every dispatch variant — row-major <MT = 1, 2, 4, 8> and packed <MT, NT = 4> / <8, 2> — over ragged per-sample prototype
    counts (one sample without any), grids whose block count is 1 or 3 mod 4 (a partially filled last thread block), V % 16 != 0 (a block
    straddling the two tables) and D = 200 (a partial last K-step), in both 16-bit operand types: logits against an fp64 matmul of the same
    operands within the fp32-accumulation bound, the identical -inf support, the fused token == the first arg-max of the kernel's own row,
    packed == row-major bit for bit, planted exact ties → the lowest index;
  * the fused repetition penalty against HF's where(s < 0, s * p, s / p) on the kernel's own unpenalised row, bit for bit, over a seen bitmap
    built by padt_seen_init, in all four scripted modes;
  * padt_greedy_step over a real vocabulary's partials, the EOS list, pad, the seen bitmap, advance = 0, steps past T_max, all-NaN rows;
  * padt_argmax_rows_f32 against torch.argmax (NaN is the maximum, ties → the first);
  * padt_sample_token per row against HF's warpers (oracle.warp_logits): support, the warped rows it writes back, ties at the k-th value,
    more than 1024 nucleus candidates, determinism;
  * padt_collect_summary, padt_assemble_sequences, padt_logit_mask, padt_stash_step_f32 against torch statements.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
X16 = pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
SENTINEL = 0x7fffffff
# fp32 accumulation of a D-term dot product (the MFMA's internal sum, the K-steps, the 4-wave combine: at most D additions in any order),
# each addition rounding its result (|partial| <= sum |h||e|) by at most 2^-23 relative (one ulp: covers a directed rounding of the MFMA's
# internal adder, twice the 2^-24 of round-to-nearest).  Products of two 16-bit operands are exact in fp32.  So |err| <= D * 2^-23 * sum |h||e|,
# i.e. c * D * 2^-24 * sum |h||e| with c = 2; the fp64 reference adds nothing at this scale.
C_ACC = 2.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


def i64(xs):
    return torch.tensor(xs, dtype=torch.int64, device="cuda")


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ head helpers
def head_problem(B, V, counts, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    NP = sum(counts)
    E = torch.randn(V, D, generator=g).to(dt).cuda()
    P = torch.randn(max(NP, 1), D, generator=g)[:NP].to(dt).cuda()
    h = torch.randn(B, D, generator=g).to(dt).cuda()
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return E, P, h, off


def ragged_counts(B):
    """per-sample prototype counts: sample 0 has none (when there are two or more samples), the rest 1..11, not a pattern of 16"""
    if B == 1:
        return [9]
    return [0] + [1 + (5 * b + b // 3) % 11 for b in range(1, B)]


def vocab_for(counts, r, tail=0):
    """V (a multiple of 16, plus `tail`) such that the head's block count is r mod 4"""
    nbp = (sum(counts) + 15) // 16
    vb = 64 + (r - 64 - nbp) % 4
    V = 16 * vb + tail
    assert ((V + sum(counts) + 15) // 16) % 4 == r or tail
    return V


def run_head(ops, h, E, P, off, packed, eos=-3, mode_table=None, step=None, gen_cfg=None, seen=None):
    """→ (part_val, part_idx, logits, nblk); every output buffer starts as NaN / garbage so that an unwritten entry shows"""
    B, D = h.shape
    V, NP = E.shape[0], P.shape[0]
    nblk = ops.vrt_head_nblk(V, NP)
    pv = torch.full((nblk * B,), float("nan"), device="cuda")
    pi = torch.full((nblk * B,), -5, dtype=torch.int32, device="cuda")
    lg = torch.full((B, V + NP), float("nan"), device="cuda")
    offt = i32(off)
    if packed:
        hp = torch.zeros((B + 15) // 16 * 16, D, device="cuda", dtype=h.dtype)
        ops.pack_rows(h, hp, B, to_packed=True)
        ops.vrt_head(hp, E, P, offt, pv, pi, eos, mode_table=mode_table, step=step, logits=lg, table_packed=ops.pack_weight(E), rows=B,
                     gen_cfg=gen_cfg, seen=seen)
    else:
        ops.vrt_head(h, E, P, offt, pv, pi, eos, mode_table=mode_table, step=step, logits=lg, gen_cfg=gen_cfg, seen=seen)
    return pv, pi, lg, nblk


def greedy_select(ops, pv, pi, nblk, B, pad=0):
    """the fused token: padt_greedy_step over the partials (no EOS, fresh state)"""
    D = 8
    hid = torch.zeros(B, D, device="cuda", dtype=BF)
    unf = torch.ones(B, dtype=torch.int32, device="cuda")
    tok = torch.full((B, 1), -9, dtype=torch.int64, device="cuda")
    cur = torch.full((B,), -9, dtype=torch.int64, device="cuda")
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    ops.greedy_step(pv, pi, nblk, hid, torch.zeros(1, B, D, device="cuda", dtype=BF), unf, tok, cur, z(1), z(B), z(B), z(3, B), -1, pad)
    assert torch.equal(tok[:, 0], cur)
    return cur.cpu()


def allowed(B, V, off, mode=0, eos=-3):
    NP = off[-1]
    m = torch.zeros(B, V + NP, dtype=torch.bool)
    if mode in (0, 1):
        m[:, :V] = True
    if mode in (0, 2):
        for b in range(B):
            m[b, V + off[b]: V + off[b + 1]] = True
    if mode == 3 and 0 <= eos < V:
        m[:, eos] = True
    return m


def check_logits(lg, h, E, P, off, what, mode=0, eos=-3):
    """fp64 reference on the same operands, element-wise fp32-accumulation bound, identical -inf support"""
    B, D = h.shape
    V = E.shape[0]
    W = torch.cat([E, P]).cpu().double()
    hd = h.cpu().double()
    ref = hd @ W.T
    bound = C_ACC * D * 2.0 ** -24 * (hd.abs() @ W.abs().T)
    m = allowed(B, V, off, mode, eos)
    out = lg.cpu()
    assert torch.equal(torch.isfinite(out), m), f"{what}: -inf support differs from the logit mask"
    assert bool((out[~m] == float("-inf")).all()), f"{what}: masked entries are not -inf"
    err = (out.double() - ref).abs()
    bad = m & (err > bound)
    assert not bad.any(), (f"{what}: {int(bad.sum())} logits outside c*D*2^-24*sum|h||e|, worst err/bound "
                           f"{(err[m] / bound[m]).max().item():.2f}")
    return ref


HEAD_B = [1, 16, 17, 32, 33, 64, 65, 128]
# the tail shapes (V % 16 == 5: one block straddles the tables; D = 200: a partial last K-step) at one B per row-block count MT
HEAD_CASES = ([("rowmajor", B) for B in HEAD_B] + [("packed", B) for B in HEAD_B]
              + [(lay, B) for lay in ("rowmajor_vtail", "rowmajor_d200") for B in (1, 17, 33, 65)])


def layout_shape(layout, B):
    counts = ragged_counts(B)
    r = 1 if HEAD_B.index(B) % 2 == 0 else 3
    D = 200 if layout == "rowmajor_d200" else 256
    V = vocab_for(counts, r, tail=5 if layout == "rowmajor_vtail" else 0)
    return counts, V, D


@X16
@pytest.mark.parametrize("layout,B", HEAD_CASES, ids=[f"{lay}-B{B}" for lay, B in HEAD_CASES])
def test_vrt_head_logits_every_dispatch_variant(ops, dt, layout, B):
    """logits vs fp64, -inf support, fused token == first arg-max of the written row; packed == row-major bit for bit"""
    counts, V, D = layout_shape(layout, B)
    E, P, h, off = head_problem(B, V, counts, D, dt, seed=1000 + B)
    packed = layout == "packed"
    pv, pi, lg, nblk = run_head(ops, h, E, P, off, packed)
    check_logits(lg, h, E, P, off, f"{layout} B={B}")
    tok = greedy_select(ops, pv, pi, nblk, B)
    assert torch.equal(tok, lg.cpu().argmax(-1)), "fused token != first arg-max of the kernel's own logits row"
    if packed:
        pv2, pi2, lg2, _ = run_head(ops, h, E, P, off, False)
        assert torch.equal(bits(lg), bits(lg2)), "packed logits differ from row-major"
        assert torch.equal(bits(pv), bits(pv2)) and torch.equal(pi, pi2), "packed partials differ from row-major"


TIE_CASES = ["across_thread_blocks", "across_nt_groups", "text_vs_vrt", "vrt_vs_vrt"]


@X16
@pytest.mark.parametrize("layout", ["rowmajor", "packed"])
@pytest.mark.parametrize("B", [1, 17, 65, 128])
@pytest.mark.parametrize("case", TIE_CASES)
def test_vrt_head_planted_ties_go_to_the_lowest_index(ops, dt, layout, B, case):
    """identical table rows whose logit is every sample's maximum: the token is the lowest of their indices, wherever they sit —
    blocks of different thread blocks (37 / 200), the NT groups of one thread block (blocks 2 and 3: one thread block at NT = 4 and NT = 2),
    a text row against the sample's own VRT row, two VRT rows of one sample"""
    counts, V, D = layout_shape(layout, B)
    E, P, h, off = head_problem(B, V, counts, D, dt, seed=2000 + B)
    h[:, 0] = 16.0
    u = E[11].clone()
    u[0] = 16.0                                                       # 256 + N(0, 16^2) against N(0, 22^2) for every other row
    win = torch.full((B,), -1, dtype=torch.int64)
    if case == "across_thread_blocks":
        E[37], E[200] = u, u
        win[:] = 37
    elif case == "across_nt_groups":
        E[40], E[60] = u, u
        win[:] = 40
    elif case == "text_vs_vrt":
        E[V - 3] = u
        for b in range(B):
            if counts[b] > 0:
                P[off[b + 1] - 1] = u
        win[:] = V - 3
    else:
        for b in range(B):
            if counts[b] >= 2:
                P[off[b]] = u
                P[off[b + 1] - 1] = u
                win[b] = V + off[b]
    pv, pi, lg, nblk = run_head(ops, h, E, P, off, layout == "packed")
    ref = check_logits(lg, h, E, P, off, f"ties {case}")
    tok = greedy_select(ops, pv, pi, nblk, B)
    out = lg.cpu()
    assert torch.equal(tok, out.argmax(-1))
    for b in range(B):
        if win[b] < 0:
            continue
        mx = ref[b][allowed(B, V, off)[b]].max()
        assert ref[b, win[b]] == mx, "construction: the planted rows are not the maximum"
        tied = (out[b] == out[b, win[b]]).nonzero().flatten().tolist()
        n_planted = 1 if case == "text_vs_vrt" and counts[b] == 0 else 2       # a sample without prototypes: the text row alone
        assert len(tied) >= n_planted and tied[0] == win[b], f"row {b}: the planted rows do not tie exactly: {tied}"
        assert int(tok[b]) == int(win[b]), f"row {b}: tie went to {int(tok[b])}, not the lowest index {int(win[b])}"


# ------------------------------------------------------------------------------------------------------------ repetition penalty
def seen_ids(B, V, off, words):
    """per sample: bits 0 / 31 / 32 of a word, the last table column, its own VRT row, another sample's VRT row, duplicates, ids outside
    [0, words * 32) (ignored) and ids in [table, words * 32) (set, but no table column)"""
    NTOT = V + off[-1]
    ids, rows = [], []
    g = torch.Generator().manual_seed(5)
    for b in range(B):
        mine = [0, 31, 32, 63, 64, 95, 96, NTOT - 1, 7, 31, 31, NTOT + 3, -1, -40, words * 32, words * 32 + 17]
        if off[b + 1] > off[b]:
            mine += [V + off[b], V + off[b + 1] - 1, V + off[b]]
        other = (b + 1) % B
        if off[other + 1] > off[other]:
            mine.append(V + off[other])
        mine += torch.randint(0, NTOT, (40,), generator=g).tolist()
        ids += mine
        rows += [b] * len(mine)
    return ids, rows


def expected_bitmap(ids, rows, B, words):
    exp = torch.zeros(B, words * 32, dtype=torch.bool)
    for i, r in zip(ids, rows):
        if 0 <= i < words * 32:
            exp[r, i] = True
    return exp


def bitmap_bool(seen, words):
    s = seen.cpu().view(torch.int32).long() & 0xFFFFFFFF
    sh = torch.arange(32)
    return ((s[:, :, None] >> sh) & 1).bool().reshape(s.shape[0], words * 32)


def hf_penalty(s, p):
    """RepetitionPenaltyLogitsProcessor: where(s < 0, s * p, s / p) in fp32 (correctly rounded: the exact fp64 product / quotient of two fp32
    values, rounded once to fp32 — fp64 carries more than 2 * 24 + 2 bits, so the double rounding is exact)"""
    p32 = torch.tensor(p, dtype=F32).double()
    sd = s.double()
    return torch.where(s < 0, (sd * p32).float(), (sd / p32).float())


@X16
@pytest.mark.parametrize("layout,B", [("rowmajor", 5), ("packed", 70)], ids=["rowmajor-B5", "packed-B70"])
def test_vrt_head_repetition_penalty_is_hf_formula_bit_for_bit(ops, dt, layout, B):
    counts = ragged_counts(B)
    V, D = vocab_for(counts, 1), 256
    E, P, h, off = head_problem(B, V, counts, D, dt, seed=3000 + B)
    NTOT = V + off[-1]
    words = (NTOT + 31) // 32 + 3                                        # wider than the table needs
    ids, rows = seen_ids(B, V, off, words)
    seen = torch.zeros(B, words, dtype=torch.int32, device="cuda")
    ops.seen_init(i64(ids), i32(rows), seen)
    exp_bits = expected_bitmap(ids, rows, B, words)
    assert torch.equal(bitmap_bool(seen, words), exp_bits), "seen_init bitmap"
    pen = 1.3
    cfg_p = ops.gen_cfg_tensor(pen, (), "cuda")
    cfg_1 = ops.gen_cfg_tensor(1.0, (), "cuda")
    eos = 7                                                              # seen in every row: mode 3 keeps exactly this (penalised) column
    modes = i32([0, 1, 2, 3])
    sb = exp_bits[:, :NTOT]
    for mode in range(4):
        step = i32([mode])
        pv, pi, lg_p, nblk = run_head(ops, h, E, P, off, layout == "packed", eos=eos, mode_table=modes, step=step, gen_cfg=cfg_p, seen=seen)
        _, _, lg_1, _ = run_head(ops, h, E, P, off, layout == "packed", eos=eos, mode_table=modes, step=step, gen_cfg=cfg_1, seen=seen)
        check_logits(lg_1, h, E, P, off, f"unpenalised mode {mode}", mode=mode, eos=eos)
        s1, sp = lg_1.cpu(), lg_p.cpu()
        hit = sb & torch.isfinite(s1)
        if mode == 0:
            assert bool((s1[hit] < 0).any()) and bool((s1[hit] > 0).any()), "construction: both penalty branches"
        exp = s1.clone()
        exp[hit] = hf_penalty(s1[hit], pen)
        bad = bits(sp) != bits(exp)
        assert not bad.any(), (f"mode {mode}: {int(bad.sum())} entries differ from HF's penalty on the kernel's own row "
                               f"(first at {bad.nonzero()[0].tolist()})")
        tok = greedy_select(ops, pv, pi, nblk, B)
        assert torch.equal(tok, sp.argmax(-1))
    # the bitmap is read-only for the head
    assert torch.equal(bitmap_bool(seen, words), exp_bits)


# ------------------------------------------------------------------------------------------------------------ greedy_step
class Loop:
    """device state of a greedy_step sequence + the host model of what it must hold"""

    def __init__(self, B, T_max, D=8, words=4):
        self.B, self.T_max, self.D, self.words = B, T_max, D, words
        z = lambda *s, v=0: torch.full(s, v, dtype=torch.int32, device="cuda")
        self.unf = z(B, v=1)
        self.tok = torch.full((B, T_max), -9, dtype=torch.int64, device="cuda")
        self.cur = torch.full((B,), -9, dtype=torch.int64, device="cuda")
        self.step = z(1)
        self.slot, self.lens, self.pos3 = z(B, v=5), z(B, v=6), z(3, B, v=9)
        g = torch.Generator().manual_seed(3)
        self.hid = torch.randn(B, D, generator=g).to(BF).cuda()
        self.hbuf = torch.full((T_max, B, D), 7.0, device="cuda", dtype=BF)
        self.seen = z(B, words)

    def run(self, pv, pi, nblk, eos, pad, advance=True, gen_cfg=None, seen=True):
        from padt_amd import ops
        ops.greedy_step(pv, pi, nblk, self.hid, self.hbuf, self.unf, self.tok, self.cur, self.step, self.slot, self.lens, self.pos3, eos, pad,
                        advance=advance, gen_cfg=gen_cfg, seen=self.seen if seen else None)


@pytest.mark.parametrize("B", [8, 128])
def test_greedy_step_over_real_vocabulary_partials(ops, B):
    """V = 151 936 text rows + ragged prototypes, packed head: about 9 600 blocks of partials per row; even rows carry a planted exact tie
    between rows 3 and 150 001 (blocks ~9 400 apart) at their maximum"""
    V, D = 151936, 256
    counts = ragged_counts(B)
    E, P, h, off = head_problem(B, V, counts, D, BF, seed=4000 + B)
    u = E[11].clone()
    u[0] = 16.0
    E[3], E[150001] = u, u
    h[0::2, 0] = 16.0
    pv, pi, lg, nblk = run_head(ops, h, E, P, off, True)
    assert nblk == (V + off[-1] + 15) // 16 and nblk > 9400
    out = lg.cpu()
    m = allowed(B, V, off)
    assert torch.equal(torch.isfinite(out), m)
    L = Loop(B, 4, words=(V + off[-1] + 31) // 32)
    L.run(pv, pi, nblk, eos=-1, pad=0)
    want = out.argmax(-1)
    assert torch.equal(L.cur.cpu(), want) and torch.equal(L.tok[:, 0].cpu(), want)
    assert (want[0::2] == 3).all(), "planted tie: the lowest index"


@pytest.mark.parametrize("n_eos", [1, 2, 3, 4])
def test_greedy_step_eos_list_pad_and_seen(ops, n_eos):
    """scripted partials (nblk = 3, the wanted token tied at a higher index in the next block): EOS ids of gen_cfg (unused slots -1) finish a
    row, finished rows emit pad, the seen bit of every emitted token (pad included) is set; step / slot / lens / pos3 advance"""
    B, T_max, eos, pad = 6, 5, 2, 5
    lst = [2, 9, 13, 21][:n_eos]
    cfg = ops.gen_cfg_tensor(1.0, lst, "cuda")
    assert cfg.cpu()[1 + n_eos: 5].tolist() == [-1] * (4 - n_eos)
    script = [[9, 40, 2, 13, 33, 21],
              [21, 41, 3, 44, 13, 9],
              [1, 2, 6, 13, 7, 8],
              [9, 50, 51, 52, 53, 54]]
    L = Loop(B, T_max)
    unf = [True] * B
    seen = torch.zeros(B, L.words * 32, dtype=torch.bool)
    for s, toks in enumerate(script):
        pv = torch.tensor([5.0] * B + [5.0] * B + [4.0] * B, device="cuda")
        pi = i32(toks + [t + 64 for t in toks] + [3] * B)
        L.run(pv, pi, 3, eos, pad, gen_cfg=cfg)
        emit = [toks[b] if unf[b] else pad for b in range(B)]
        for b in range(B):
            seen[b, emit[b]] = True
            unf[b] = unf[b] and not (emit[b] == eos or emit[b] in lst)
        assert L.tok[:, s].tolist() == emit and L.cur.tolist() == emit, f"step {s}"
        assert L.unf.cpu().bool().tolist() == unf, f"step {s}: unfinished"
        assert torch.equal(bitmap_bool(L.seen, L.words), seen), f"step {s}: seen bitmap"
        assert int(L.step) == s + 1
        assert torch.equal(L.hbuf[s], L.hid)
    assert (L.slot == 5 + len(script)).all() and (L.lens == 6 + len(script)).all() and (L.pos3 == 9 + len(script)).all()
    assert (L.tok[:, len(script):] == -9).all()


def test_greedy_step_advance_zero_and_steps_past_t_max(ops):
    B, T_max = 4, 3
    L = Loop(B, T_max)
    pv = torch.tensor([1.0] * B, device="cuda")
    pi = i32([10, 11, 12, 13])
    L.run(pv, pi, 1, -1, 0, advance=False)
    assert (L.slot == 5).all() and (L.lens == 6).all() and (L.pos3 == 9).all(), "advance = 0 moved slot / lens / pos3"
    assert L.cur.tolist() == [10, 11, 12, 13] and L.tok[:, 0].tolist() == [10, 11, 12, 13] and int(L.step) == 1
    L.step.fill_(T_max)
    tok0, hb0 = L.tok.clone(), L.hbuf.clone()
    pi2 = i32([20, 21, 22, 23])
    L.run(pv, pi2, 1, -1, 0)
    assert torch.equal(L.tok, tok0), "step >= T_max wrote tokens_out"
    assert torch.equal(L.hbuf, hb0), "step >= T_max wrote hidden_buf"
    assert L.cur.tolist() == [20, 21, 22, 23], "cur_tok must still be set"
    assert int(L.step) == T_max + 1
    assert bool(bitmap_bool(L.seen, L.words)[torch.arange(B), torch.tensor([20, 21, 22, 23])].all())


@pytest.mark.parametrize("layout", ["rowmajor", "packed"])
def test_greedy_step_all_nan_row_emits_pad(ops, layout):
    """a NaN hidden row: every one of its logits is NaN, no partial has an index (sentinel), the row emits pad; the other rows are untouched"""
    B = 5
    counts = ragged_counts(B)
    V = vocab_for(counts, 1)
    E, P, h, off = head_problem(B, V, counts, 256, BF, seed=77)
    h[2] = float("nan")
    pv, pi, lg, nblk = run_head(ops, h, E, P, off, layout == "packed")
    pic = pi.view(nblk, B).cpu()
    assert (pic[:, 2] == SENTINEL).all() and (pv.view(nblk, B).cpu()[:, 2] == float("-inf")).all()
    pad = 17
    L = Loop(B, 2, words=(V + off[-1] + 31) // 32)
    L.run(pv, pi, nblk, -1, pad)
    want = lg.cpu().argmax(-1)
    want[2] = pad
    assert torch.equal(L.cur.cpu(), want)
    assert bool(bitmap_bool(L.seen, L.words)[2, pad])
    # the same contract straight from sentinel partials
    L2 = Loop(3, 2)
    L2.run(torch.full((6,), float("-inf"), device="cuda"), torch.full((6,), SENTINEL, dtype=torch.int32, device="cuda"), 2, -1, pad)
    assert L2.cur.tolist() == [pad] * 3


# ------------------------------------------------------------------------------------------------------------ argmax_rows
def argmax_rows_check(ops, x, n):
    B = x.shape[0]
    pv = torch.full((B,), 3.0, device="cuda")
    pi = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    ops.argmax_rows(x, n, pv, pi, B)
    xc = x.cpu()[:, :n]
    want = xc.argmax(-1)
    got = pi.cpu().long()
    assert torch.equal(got, want), f"rows {(got != want).nonzero().flatten().tolist()}: {got[got != want].tolist()} vs {want[got != want].tolist()}"
    assert torch.equal(bits(pv.cpu()), bits(xc[torch.arange(B), want]))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 156000])
def test_argmax_rows_matches_torch_argmax(ops, n):
    g = torch.Generator().manual_seed(n)
    ld = n + 7                                                           # padding columns hold NaN: never read
    rows = []
    base = lambda: torch.randn(n, generator=g)
    clamp = lambda i: min(max(i, 0), n - 1)
    r = base()
    rows.append(r)                                                       # random
    r = base()
    r[clamp(5)] = 9.0
    r[clamp(5 + 1024)] = 9.0                                             # tie within one thread's stride
    rows.append(r)
    r = base()
    r[clamp(n - 2)] = 9.0
    r[clamp(n // 2 + 1)] = 9.0
    r[clamp(n // 2)] = 9.0                                               # ties across neighbouring threads
    rows.append(r)
    for pos in (0, n // 3, n - 1):                                       # the first NaN at several positions
        r = base()
        r[clamp(pos)] = float("nan")
        r[clamp(pos + 1)] = 50.0
        rows.append(r)
    r = base()
    for pos in (n - 1, n // 2, n // 5 + 1030, 3):                        # several NaNs: the first one wins
        r[clamp(pos)] = float("nan")
    rows.append(r)
    r = base()
    r[clamp(n // 4)] = float("inf")
    r[clamp(n // 4 + 2048)] = float("inf")
    r[clamp(n // 7)] = float("-inf")
    rows.append(r)
    r = base()
    r[clamp(1)] = float("inf")
    r[0] = float("-inf")
    rows.append(r)
    rows.append(torch.full((n,), float("-inf")))                         # all -inf → 0
    x = torch.full((len(rows), ld), float("nan"))
    x[:, n:] = float("nan")
    x[-1, n:] = float("inf")
    for i, r in enumerate(rows):
        x[i, :n] = r
    argmax_rows_check(ops, x.cuda(), n)


def test_argmax_rows_128_distinct_rows(ops):
    n, B = 5003, 128
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, n + 1, generator=g)
    x[:, n] = float("nan")
    for b in range(B):
        x[b, (b * 37 + 5) % n] = 10.0 + b % 5                            # each row's maximum at its own position
    argmax_rows_check(ops, x.cuda(), n)


# ------------------------------------------------------------------------------------------------------------ sample_token
def ref_warp(row, T, k, p):
    """HF's Temperature → TopK → TopP on one fp32 row, evaluated in fp64 in the kernel's rank order (value descending, index ascending):
    → (kept, ambiguous): `ambiguous` marks the ranks whose mass-before lies within fp32 rounding of top_p"""
    x = row.double()
    n = x.numel()
    fin = x > float("-inf")
    keep = fin.clone()
    if 0 < k < n and int(fin.sum()) > k:
        kth = torch.sort(x[fin], descending=True).values[k - 1]
        keep = fin & (x >= kth)
    amb = torch.zeros(n, dtype=torch.bool)
    if p < 1.0:
        idx = keep.nonzero().flatten()                                   # ascending index
        order = idx[torch.sort(-x[idx], stable=True).indices]
        v = x[order]
        w = torch.exp((v - v.max()) / T)
        before = (torch.cumsum(w, 0) - w) / w.sum()
        kr = before < p
        kr[0] = True
        keep = torch.zeros(n, dtype=torch.bool)
        keep[order[kr]] = True
        amb[order[(before - p).abs() < 1e-5]] = True
    return keep, amb


def check_against_hf(row, T, k, p, keep, amb):
    """the rank-order reference agrees with oracle.warp_logits (HF's code): the same support where no tie straddles the nucleus cut, the same
    number of kept entries inside a tie that does"""
    import padt_oracle as O
    hf = torch.isfinite(O.warp_logits(row[None, :], T, k, p)[0])
    if amb.any():
        return
    assert int(hf.sum()) == int(keep.sum())
    diff = hf != keep
    if diff.any():
        vals = row[diff].unique()
        assert vals.numel() == 1, "reference and HF differ outside one tied value"
        tv = vals[0]
        assert int(hf[row == tv].sum()) == int(keep[row == tv].sum())


def sample(ops, x, n, cfg, step, B):
    pv = torch.full((B,), 3.0, device="cuda")
    pi = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    ops.sample_token(x, n, cfg, step, pv, pi, B)
    return pi.cpu().long()


def row_case(case, n, g):
    """one base row per case; the test gives row b the base rolled by 191 b (every row different, the structure kept)"""
    r = torch.randn(n, generator=g) * 2.0
    if case == "few_finite":
        r[:] = float("-inf")
        pos = torch.randperm(n, generator=g)[:25]
        r[pos] = torch.randn(25, generator=g)
    elif case == "kth_ties":
        top = torch.randperm(n, generator=g)[:13]
        r[top[:9]] = 12.0 + torch.rand(9, generator=g)                   # 9 above the k-th value
        r[top[9:]] = 11.5                                                # the 10th largest, tied four times: all four stay (k = 10)
    elif case == "single":
        r[:] = float("-inf")
        r[int(torch.randint(0, n, (1,), generator=g))] = 0.25
    return r


SAMPLE_CASES = [  # (case, n, T, top_k, top_p)
    ("plain", 3000, 1.0, 0, 1.0),
    ("plain", 3000, 1.0, 40, 1.0),
    ("plain", 3000, 0.7, 50, 0.9),
    ("plain", 3000, 0.05, 20, 0.9),
    ("plain", 3000, 4.0, 20, 0.9),
    ("plain", 3000, 4.0, 300, 0.5),
    ("few_finite", 3000, 1.0, 40, 1.0),
    ("few_finite", 3000, 1.0, 40, 0.95),
    ("plain", 500, 1.0, 500, 0.8),                                       # k >= n
    ("plain", 500, 1.0, 900, 0.8),
    ("plain", 500, 1.0, 900, 1.0),
    ("kth_ties", 3000, 1.0, 10, 1.0),
    ("kth_ties", 3000, 1.0, 10, 0.999),
    ("single", 3000, 1.0, 5, 0.5),
    ("single", 3000, 1.0, 0, 1.0),
]


@pytest.mark.parametrize("case,n,T,top_k,top_p", SAMPLE_CASES, ids=[f"{c[0]}-n{c[1]}-T{c[2]}-k{c[3]}-p{c[4]}" for c in SAMPLE_CASES])
def test_sample_token_per_row_support_and_written_back_scores(ops, case, n, T, top_k, top_p):
    """B = 16 different rows, ld > n with +inf / NaN poison past n: every draw lies in the row's own warped support; with write_back the row
    becomes l / T (bit for bit, correctly rounded fp32) on exactly that support and -inf elsewhere, the poison untouched"""
    B, ld, steps = 16, n + 12, 24
    g = torch.Generator().manual_seed(sum(map(ord, case)) + n + top_k)
    base = row_case(case, n, g)
    x = torch.empty(B, ld)
    x[:, n:] = float("inf")
    x[:, n + 1::2] = float("nan")
    for b in range(B):
        x[b, :n] = torch.roll(base, 191 * b)
    refs = []
    for b in range(B):
        keep, amb = ref_warp(x[b, :n], T, top_k, top_p)
        check_against_hf(x[b, :n], T, top_k, top_p, keep, amb)
        refs.append((keep, amb))
    xd = x.cuda()
    cfg = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=99, temperature=T, top_k=top_k, top_p=top_p)
    draws = []
    for s in range(steps):
        draws.append(sample(ops, xd, n, cfg, i32([s]), B))
    assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32)), "sample_token without write_back changed its input"
    for b in range(B):
        keep, amb = refs[b]
        for s in range(steps):
            t = int(draws[s][b])
            assert 0 <= t < n and (keep[t] or amb[t]), f"row {b} step {s}: drew {t}, outside the row's warped support"
        if case == "single":
            assert all(int(d[b]) == int(keep.nonzero()[0]) for d in draws)
    # same (seed, step, row) → the same draw
    assert torch.equal(sample(ops, xd, n, cfg, i32([3]), B), draws[3])
    # write-back
    cfg_w = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=99, temperature=T, top_k=top_k, top_p=top_p, write_back=True)
    xw = xd.clone()
    got = sample(ops, xw, n, cfg_w, i32([3]), B)
    assert torch.equal(got, draws[3]), "write_back changed the draw"
    w = xw.cpu()
    assert torch.equal(w[:, n:].view(torch.int32), x[:, n:].view(torch.int32)), "write_back touched the columns past n"
    t32 = torch.tensor(T, dtype=F32).double()
    for b in range(B):
        keep, amb = refs[b]
        wb = w[b, :n]
        kept = torch.isfinite(wb)
        assert torch.equal(kept[~amb], keep[~amb]), f"row {b}: written-back support differs from HF's warpers"
        assert bool((wb[~kept] == float("-inf")).all())
        exp = (x[b, :n].double() / t32).float()
        assert torch.equal(bits(wb[kept]), bits(exp[kept])), f"row {b}: written-back values are not l / T"


def test_sample_token_identical_rows_draw_independently(ops):
    n, B = 3000, 64
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(n, generator=g) * 0.5)[None, :].repeat(B, 1).cuda()
    cfg = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=5, temperature=1.0, top_k=0, top_p=1.0)
    for s in range(3):
        d = sample(ops, x, n, cfg, i32([s]), B)
        assert d.unique().numel() > 8, f"step {s}: identical rows drew {d.unique().numel()} distinct tokens out of {B}"
        assert torch.equal(d, sample(ops, x, n, cfg, i32([s]), B))


def nucleus_tie_row(g, n=3000, n_above=823, n_tie=250):
    """one dominant token (at the last index), n_above distinct values in (1, 3), n_tie entries tied at 0.5 — the 1024-th largest value —
    and the rest below: 1 + n_above + n_tie > 1024 top-k survivors"""
    r = torch.empty(n)
    idx = torch.randperm(n - 1, generator=g)
    dom = n - 1
    above, ties, below = idx[:n_above], idx[n_above: n_above + n_tie], idx[n_above + n_tie:]
    r[dom] = 10.0
    r[above] = 1.0 + 2.0 * torch.rand(n_above, generator=g)
    r[ties] = 0.5
    r[below] = -1.0 + 0.3 * torch.rand(below.numel(), generator=g)
    assert r[above].unique().numel() == n_above
    return r, dom, torch.sort(ties).values


@pytest.mark.parametrize("top_p", [0.9, 0.999])
def test_sample_token_nucleus_with_more_than_1024_candidates(ops, top_p):
    """top_k = 1024 with 250 entries tied at the k-th value (1074 candidates): the nucleus is HF's — its number of tied entries, the lowest
    indices among them — frequencies within 5 sigma, and the draws repeat exactly across launches"""
    n, B, reps, k, T = 3000, 64, 1024, 1024, 1.0
    g = torch.Generator().manual_seed(37)                                # a row with no rank within rounding of either top_p
    row, dom, ties = nucleus_tie_row(g)
    keep, amb = ref_warp(row, T, k, top_p)
    assert not amb.any(), "construction: no rank within rounding of top_p"
    check_against_hf(row, T, k, top_p, keep, amb)
    n_keep_tie = int(keep[ties].sum())
    assert torch.equal(keep[ties], torch.arange(ties.numel()) < n_keep_tie), "reference: the lowest-index tied entries"
    if top_p > 0.99:
        assert 0 < n_keep_tie < ties.numel(), "construction: the cut lies inside the tie"
    exp = torch.where(keep, row, torch.full_like(row, float("-inf")))
    pr = exp.double().softmax(-1)
    x = row[None, :].repeat(B, 1).cuda()
    cfg = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=77, temperature=T, top_k=k, top_p=top_p)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.long, device="cuda")
    pv = torch.zeros(B, device="cuda")
    pi = torch.zeros(B, dtype=torch.int32, device="cuda")
    first = []
    for r in range(reps):
        step.fill_(r)
        ops.sample_token(x, n, cfg, step, pv, pi, B)
        counts += torch.bincount(pi.long().clamp(0, n), minlength=n + 1)[:n]
        if r < 16:
            first.append(pi.clone())
    assert int(counts.sum()) == B * reps, "a draw outside [0, n)"
    N = B * reps
    c = counts.cpu()
    assert int(c[~keep].sum()) == 0, f"drew outside the nucleus: {(c * (~keep)).nonzero().flatten()[:10].tolist()}"
    freq = c.double() / N
    common = keep & (pr * N >= 50)
    sigma = (pr * (1 - pr) / N).sqrt()
    dev = ((freq - pr).abs() / (sigma + 1e-12))[common]
    assert dev.max().item() < 5.0, f"worst deviation {dev.max().item():.2f} sigma"
    rare = keep & ~common
    if bool(rare.any()):
        pm, fm = pr[rare].sum().item(), freq[rare].sum().item()
        assert abs(fm - pm) < 5.0 * math.sqrt(pm * (1 - pm) / N) + 1e-9, f"rare-token mass {fm:.5f} vs {pm:.5f}"
    for r in range(16):                                                  # the same launches again: the same draws
        step.fill_(r)
        ops.sample_token(x, n, cfg, step, pv, pi, B)
        assert torch.equal(pi, first[r]), f"launch {r}: the draws are not deterministic"
    # the kept set, exactly: written-back rows (one launch over rows that differ by a roll)
    cfg_w = ops.gen_cfg_tensor(1.0, (), "cuda", do_sample=True, seed=77, temperature=T, top_k=k, top_p=top_p, write_back=True)
    xs = torch.stack([torch.roll(row, 7 * b) for b in range(8)])
    xw = xs.cuda()
    ops.sample_token(xw, n, cfg_w, step, pv, pi, 8)
    w = xw.cpu()
    for b in range(8):
        kb, _ = ref_warp(xs[b], T, k, top_p)
        assert torch.equal(torch.isfinite(w[b]), kb), f"row {b}: written-back nucleus differs"
        assert torch.equal(bits(w[b][kb]), bits(xs[b][kb]))


# ------------------------------------------------------------------------------------------------------------ bookkeeping kernels
def test_collect_summary(ops):
    n_rows, n_batch, T_max, done, eos = 6, 3, 8, 5, 2
    lst = [2, 9, 13]
    tok = torch.tensor([[4, 4, 9, 2, 4, 4, 4, 4],                        # list id first
                        [4, 2, 4, 4, 4, 4, 4, 4],                        # config eos
                        [4, 4, 4, 4, 4, 2, 9, 4],                        # EOS only past `done`: ignored
                        [13, 4, 4, 4, 4, 4, 4, 4],
                        [4, 4, 4, 4, 21, 4, 4, 4],                        # 21: not an EOS id
                        [4, 4, 4, 4, 9, 4, 4, 4]])
    err = i32([3])
    unf = i32([0, 0, 1, 0, 0, 0])
    nf_rows = i32([0, 1, 0, 0, 1, 0])
    nf_batch = i32([1, 0, 1, 7])
    out = torch.full((2 + 2 * n_rows + n_batch,), -99, dtype=torch.int32, device="cuda")
    cfg = ops.gen_cfg_tensor(1.0, lst, "cuda")
    ops.collect_summary(err, unf, nf_rows, nf_batch, n_batch, tok.cuda(), done, eos, cfg, out)
    is_eos = (tok[:, :done, None] == torch.tensor(lst + [eos])).any(-1)
    first = torch.where(is_eos.any(-1), is_eos.int().argmax(-1), torch.full((n_rows,), -1))
    want = [3, 1] + nf_rows.tolist() + nf_batch.tolist()[:n_batch] + first.tolist()
    assert out.tolist() == want
    assert first.tolist() == [2, 1, -1, 0, -1, 4]
    # without the list only the config eos counts; all finished → any = 0
    ops.collect_summary(err, torch.zeros_like(unf), nf_rows, nf_batch, n_batch, tok.cuda(), done, eos, None, out)
    assert out[1].item() == 0 and out[2 + n_rows + n_batch:].tolist() == [3, 1, -1, -1, -1, -1]


@pytest.mark.parametrize("L,n_steps", [(5, 4), (0, 4), (5, 0), (3, 7)])
def test_assemble_sequences(ops, L, n_steps):
    B, T_max, vocab, row0 = 3, 7, 100, 40
    g = torch.Generator().manual_seed(L * 10 + n_steps)
    ids = torch.randint(0, 140, (B, L + 2), generator=g)[:, :L]            # ld_ids > L
    tok = torch.tensor([[5, 100, 140, 99, 101, 3, 1000],
                        [vocab + row0, 7, vocab, vocab - 1, 0, 150, 8],
                        [1, 2, 3, 4, 5, 6, 139]])
    ids_full = torch.randint(0, 140, (B, L + 2), generator=g)
    ids_full[:, :L] = ids
    out = ops.assemble_sequences(ids_full.cuda()[:, :L], tok.cuda(), n_steps, vocab, row0).cpu()
    t = tok[:, :n_steps]
    want = torch.cat([ids, torch.where(t >= vocab, t - row0, t)], 1)
    assert out.shape == (B, L + n_steps) and torch.equal(out, want)


def test_logit_mask_with_a_nonzero_first_prototype_row(ops):
    vocab, B, p0 = 50, 3, 7
    off = [7, 7, 12, 20]                                                  # session offsets; the batch's first prototype row is 7
    table_rows = vocab + 13
    m = ops.logit_mask(i32(off), vocab, table_rows, p0, B).cpu()
    c = torch.arange(table_rows)
    want = torch.stack([(c < vocab) | ((c - vocab + p0 >= off[b]) & (c - vocab + p0 < off[b + 1])) for b in range(B)])
    assert torch.equal(m, want)
    assert int(m[0].sum()) == vocab and int(m[1, vocab:].sum()) == 5 and int(m[2, vocab:].sum()) == 8


@pytest.mark.parametrize("step", [-1, 0, 2, 3, 9])
def test_stash_step_f32_writes_only_steps_inside_the_buffer(ops, step):
    t_max, n = 3, 4 * 37 + 4 * 1024
    src = torch.randn(n, device="cuda")
    dst = torch.full((t_max, n), -7.5, device="cuda")
    ops.stash_step_f32(src, i32([step]), dst)
    want = torch.full((t_max, n), -7.5, device="cuda")
    if 0 <= step < t_max:
        want[step] = src
    assert torch.equal(dst, want)
