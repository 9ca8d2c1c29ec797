"""generate(frequency_penalty=, presence_penalty=, patch_suppression=) on the device.

Kernel level: padt_count_update against generation.count_state bit for bit, every table inside a larger poisoned buffer that is compared as a
whole (three rows with grids 2x3, 3x2 and 1x1 whose patch ranges are adjacent; a finished row, a row without suppression, a run closed in the
step and one left open; saturation), and the COUNTS head kernels (padt_vrt_head_counts) against generation.count_penalty_row evaluated in fp32
torch on the parent head's penalty-free row: the written row bit for bit, the arg-max partials, the LSE fold (test_token_logprobs_gpu.within,
derived there for this fold of the same logit bits), the probe value — 3 and 17 rows, packed (96 text rows) and row-major (90 text rows: not
a multiple of 16, nor of the 4 columns a lane loads at once) table, both operand twins, with and without bias / decay.

End to end (the small synthetic model, two ragged samples; every test below `setup` runs once per operand twin, fp16 and bf16): the captured
step against the HOOKED loop running a ``logits_processor`` written from the two specification functions — sequences, every score row and the
hidden rows equal."""
import types

import pytest
import torch

import test_score_bias_gpu as SB
import test_token_logprobs_gpu as TL
import test_token_selection_gpu as TS

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
X16 = TL.X16
INF = float("inf")
PAD = TL.PAD
i32, i64, bits, within, ref_logprob = TS.i32, TS.i64, TS.bits, TL.within, TL.ref_logprob
guarded, guards_ok, first_argmax = SB.guarded, SB.guards_ok, SB.first_argmax
GUARD = 8
POISON = 0x5A5A


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------ the update kernel
UV, ULD = 50, 52                                                      # text ids 0 .. 49, rows of 52 counts (2 never-touched padding columns)
UGRIDS = [(2, 3), (3, 2), (1, 1)]
UOFF = [0, 6, 12, 13]                                                 # adjacent patch ranges
URADIUS = [2, -1, 1]                                                  # row 1: no suppression
UEOS = 9


def v(j):
    return UV + j


# row 0: a token on its LAST patch (5 = (1, 2)) with radius 2 covers its whole grid and must not reach row 1's patches; runs closed by text,
#        a foreign VRT id (row 1's patch) inside a run, and a run left open at the end
# row 1: VRT tokens and repeats, suppression off
# row 2: one patch; finished by the EOS at index 3 — the bookkeeping kernel clears `unfinished` in that step, so the kernel sees tokens 0 .. 2
UTOKENS = [[3, v(5), v(0), 7, 7, v(1), v(8), v(1), 3, v(4), v(4)],
           [v(6), v(7), 4, 4, v(11), v(6), 4, 30, 4, v(0), 4],
           [v(12), 9 + 1, v(12), UEOS, PAD, PAD, PAD, PAD, PAD, PAD, PAD]]
ULIVE = [11, 11, 3]                                                   # tokens the kernel is to see per row


def poisoned(shape):
    """an int16 table of zeros inside a poisoned flat buffer → (flat, view)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((2 * GUARD + n,), POISON, device="cuda", dtype=torch.int16)
    view = flat[GUARD: GUARD + n].view(*shape)
    view.zero_()
    return flat, view


def expected_tables(ops, n_seen, preload=None):
    """the three whole buffers (guards and padding columns included) after the rows saw n_seen[b] tokens, from count_state"""
    from padt_amd.generation import count_state
    text = torch.full((2 * GUARD + 3 * ULD,), POISON, dtype=torch.int32)
    patch = torch.full((2 * GUARD + UOFF[-1],), POISON, dtype=torch.int32)
    near = patch.clone()
    tv, pv, nv = text[GUARD:-GUARD].view(3, ULD), patch[GUARD:-GUARD], near[GUARD:-GUARD]
    tv[:, :UV] = 0
    pv.zero_()
    nv.zero_()
    for b in range(3):
        count, nr = count_state(UTOKENS[b], n_seen[b], UV, UOFF[b], UOFF[b + 1], UGRIDS[b], URADIUS[b] if URADIUS[b] >= 0 else None)
        for c, k in count.items():
            if c < UV:
                tv[b, c] = k
            else:
                pv[c - UV] = k
        nv[UOFF[b]: UOFF[b + 1]] = torch.tensor(nr, dtype=torch.int32)
    return text, patch, near


def test_count_update_is_count_state_bit_for_bit_in_poisoned_buffers(ops):
    T = len(UTOKENS[0])
    tf, text = poisoned((3, ULD))
    text[:, UV:] = POISON                                             # the padding columns are never read or written
    pf, patch = poisoned((UOFF[-1],))
    nf, near = poisoned((UOFF[-1],))
    tokens = i64(UTOKENS)
    closed = opened = False
    for n in range(1, T + 1):
        unf = i32([1 if n <= ULIVE[b] else 0 for b in range(3)])
        ops.count_update(tokens, i32([n]), unf, i32(UOFF), i32(UGRIDS), i32(URADIUS), text, patch, near, UV, UOFF[-1])
        want = expected_tables(ops, [min(n, ULIVE[b]) for b in range(3)])
        for name, flat, w in (("cnt_text", tf, want[0]), ("cnt_patch", pf, want[1]), ("near", nf, want[2])):
            assert torch.equal(ops.count_values(flat).cpu(), w), f"{name} after {n} tokens"
        closed |= n >= 2 and UTOKENS[0][n - 1] < UV <= UTOKENS[0][n - 2]
        opened |= UTOKENS[0][n - 1] >= UV
    assert closed and opened and UTOKENS[0][-1] >= UV                 # a run closed in a step, and one left open at the end
    got_near = ops.count_values(near).cpu()
    # row 0's windows: tokens 5 and 0 (first run), 1 and 1 (second; the foreign id adds nothing) with radius 2 on 2 x 3 — and nothing beyond patch 5
    assert got_near[:6].tolist() == [4, 4, 4, 4, 4, 4] and got_near[6:12].tolist() == [0] * 6 and got_near[12].item() == 1
    assert ops.count_values(patch).cpu()[8].item() == 0               # row 0's foreign VRT token is not row 1's count


def test_count_update_saturates(ops):
    tf, text = poisoned((3, ULD))
    pf, patch = poisoned((UOFF[-1],))
    nf, near = poisoned((UOFF[-1],))
    text[0, 7] = -1                                                   # 65535
    near[2] = -1
    patch[6] = -1
    tokens = i64([[3, v(5), v(0), 7], [v(6), v(6), v(6), v(6)], [1, 1, 1, 1]])
    for n in (1, 2, 3, 4):
        ops.count_update(tokens, i32([n]), i32([1, 1, 1]), i32(UOFF), i32(UGRIDS), i32(URADIUS), text, patch, near, UV, UOFF[-1])
    assert ops.count_values(text)[0, 7].item() == 65535 and ops.count_values(text)[0, 3].item() == 1
    assert ops.count_values(near)[:6].tolist() == [2, 2, 65535, 2, 2, 2]
    assert ops.count_values(patch)[6].item() == 65535 and ops.count_values(patch)[5].item() == 1
    for flat in (tf, pf, nf):
        assert bool((flat[:GUARD] == POISON).all()) and bool((flat[-GUARD:] == POISON).all())


def test_count_update_writes_nothing_outside_its_step_range_or_for_a_wrong_grid(ops):
    tf, text = poisoned((3, ULD))
    pf, patch = poisoned((UOFF[-1],))
    nf, near = poisoned((UOFF[-1],))
    tokens = i64([[v(0), 3], [v(6), 4], [v(12), 5]])
    before = [f.clone() for f in (tf, pf, nf)]
    for n in (0, 3, -1):                                              # no token yet / past the buffer
        ops.count_update(tokens, i32([n]), i32([1, 1, 1]), i32(UOFF), i32(UGRIDS), i32(URADIUS), text, patch, near, UV, UOFF[-1])
    assert all(torch.equal(a, b) for a, b in zip(before, (tf, pf, nf)))
    ops.count_update(tokens, i32([2]), i32([1, 1, 1]), i32(UOFF), i32([(2, 2), (3, 2), (1, 1)]), i32([2, 1, 9]), text, patch, near, UV, UOFF[-1])
    got = ops.count_values(near).cpu()                                # row 0: 2 x 2 is not its 6 patches; row 2: a radius above the cap — both ignored
    assert got[:6].tolist() == [0] * 6 and got[6:12].tolist() == [1, 1, 1, 1, 0, 0] and got[12].item() == 0
    assert ops.count_values(text)[:, :6].tolist() == [[0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1]]


# ------------------------------------------------------------------------------------------------------------ the head
D = 64
EOS, EOS2 = 37, 41
PEN = 1.3
START, FACTOR, T_DECAY = 2, 1.3, 6
MODE_TABLE = [0, 1, 0, 2, 0, 3, 0, 0]                                 # step 1 text only, 3 own patches only, 5 EOS forced
STEPS = [0, 3, 4, 5]
PCOUNTS = (5, 12, 3)                                                  # ragged patch ranges; further rows have none
LAYOUT_V = {"packed": 96, "rowmajor": 90}                             # 90: no multiple of 16, nor of a lane's 4 columns


@pytest.fixture(scope="module")
def problem():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops
    from padt_amd.generation import decay_table
    out = {}
    for layout, V in LAYOUT_V.items():
        for B in (3, 17):
            for dt in (BF, F16):
                pc = list(PCOUNTS) + [0] * (B - 3)
                NP = sum(pc)
                NTOT = V + NP
                E, P, h, off = TS.head_problem(B, V, pc, D, dt, seed=300 + B + V)
                g = torch.Generator().manual_seed(500 + B + V)
                words = (NTOT + 31) // 32
                seen_b = torch.rand(B, NTOT, generator=g) < 0.3
                ban_b = torch.rand(B, NTOT, generator=g) < 0.1
                bias = torch.zeros(NTOT)
                pick = torch.randperm(NTOT, generator=g)[:40]
                bias[pick] = torch.randn(40, generator=g) * 6
                bias[[3, 20]] = -INF
                seen_b[:, [0, EOS, V]] = True
                ban_b[:, [0, EOS, EOS2, V, V + 5]] = False
                ban_b[0, EOS2] = True

                def bitmap(m):
                    w = torch.zeros(B, words * 32, dtype=torch.int64)
                    w[:, :NTOT] = m.long()
                    packed = (w.view(B, words, 32) << torch.arange(32)).sum(-1)
                    return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32).cuda()
                base = {}
                for mode in (0, 1, 2, 3):                             # the same head with counts off: masked, penalty-free, unbanned
                    lg = torch.full((B, NTOT), float("nan"), device="cuda")
                    nblk = ops.vrt_head_nblk(V, NP)
                    ops.vrt_head(h, E, P, i32(off), torch.empty(nblk * B, device="cuda"), torch.empty(nblk * B, dtype=torch.int32, device="cuda"), EOS,
                                 mode_table=i32([mode]), step=i32([0]), logits=lg)
                    base[mode] = lg.cpu()
                # the count tables: text [B][ld] with poisoned padding columns, patch / near [NP]; values 0 (most), small, 1024 and the maximum
                ld = (V + 3) // 4 * 4
                val = torch.tensor([0, 0, 0, 1, 2, 3, 7, 1024])
                cnt_text = val[torch.randint(0, 8, (B, V), generator=g)]
                cnt_patch = val[torch.randint(0, 8, (NP,), generator=g)]
                near = val[torch.randint(0, 7, (NP,), generator=g)]
                cnt_text[:, [0, EOS]] = torch.tensor([2, 5])          # the forced columns of the probe head: counted
                cnt_text[1, 15] = 65535
                cnt_patch[0], near[0], near[5], near[6] = 3, 0, 2, 65535
                near[17:20] = torch.tensor([1, 2, 3])                 # row 2's three patches: all suppressed
                f = (torch.rand(B, generator=g) * 4 - 2).float()
                pp = (torch.rand(B, generator=g) * 4 - 2).float()
                sp = torch.tensor([1.5, INF, INF] + [0.0] * (B - 3))  # row 2: every own patch banned — no candidate at the patches-only step
                f[0], pp[0] = 2.0, 1.0
                if B > 3:
                    f[3], pp[3] = 0.0, 0.0                            # a row of the batch without penalties
                tbl = torch.full((B, ld), POISON, dtype=torch.int32)
                tbl[:, :V] = cnt_text
                as16 = lambda t: torch.where(t >= 32768, t - 65536, t).to(torch.int16).cuda()
                counts_full = torch.zeros(B, NTOT, dtype=torch.int64)
                counts_full[:, :V] = cnt_text
                counts_full[:, V:] = cnt_patch
                near_full = torch.zeros(B, NTOT, dtype=torch.int64)
                near_full[:, V:] = near
                out[(layout, B, dt)] = types.SimpleNamespace(
                    B=B, V=V, NP=NP, NTOT=NTOT, E=E, P=P, h=h, off=off, seen_b=seen_b, ban_b=ban_b, seen=bitmap(seen_b), ban=bitmap(ban_b),
                    bias=bias, bias_d=bias.cuda(), decay=decay_table((START, FACTOR), T_DECAY), base=base,
                    cfg=ops.gen_cfg_tensor(PEN, (EOS, EOS2), "cuda"), cnt_text=as16(tbl), cnt_patch=as16(cnt_patch), near=as16(near),
                    cpen=torch.stack([f, pp, sp]).cuda().contiguous(), counts_full=counts_full, near_full=near_full, f=f, p=pp, sp=sp)
                out[(layout, B, dt)].decay_d = out[(layout, B, dt)].decay.cuda()
    return out


def run(ops, p, packed, head, step, edits=True, counts=True):
    """one launch of padt_vrt_head_counts (counts=False: padt_vrt_head_bias) + the bookkeeping kernel, every output between guard words"""
    B, V, NTOT = p.B, p.V, p.NTOT
    nblk = ops.vrt_head_nblk(V, p.NP)
    r = types.SimpleNamespace(nblk=nblk, step=step)
    fl = {}
    fl["pv"], r.pv = guarded(nblk * B)
    fl["pi"], r.pi = guarded(nblk * B, torch.int32)
    fl["lg"], lg = guarded(B * NTOT)
    r.lg = lg.view(B, NTOT)
    fl["ps"], r.ps = guarded(nblk * B)
    fl["probe"], r.probe = guarded(B)
    t_max = 8
    fl["lp"], lp = guarded(B * t_max)
    r.lp = lp.view(B, t_max)
    st = i32([step])
    cols = [0, EOS, V, V + 5, 3, -1, 15, EOS2]                        # counted text columns, own / foreign patches, a -inf bias, free
    forced = [[cols[(b + s) % len(cols)] for s in range(t_max)] for b in range(B)]
    r.forced = torch.tensor(forced)
    tab = i32(forced)
    hin, kw = p.h, dict(mode_table=i32(MODE_TABLE), step=st, logits=r.lg, gen_cfg=p.cfg, seen=p.seen, ban=p.ban)
    if packed:
        hin = torch.zeros((B + 15) // 16 * 16, D, device="cuda", dtype=p.h.dtype)
        ops.pack_rows(p.h, hin, B, to_packed=True)
        kw.update(table_packed=ops.pack_weight(p.E), rows=B)
    args = (hin, p.E, p.P, i32(p.off), r.pv, r.pi, EOS)
    more = dict(bias=p.bias_d if edits else None, decay=p.decay_d if edits else None, part_sum=None if head == "plain" else r.ps,
                forced=tab if head == "probe" else None, probe_val=r.probe if head == "probe" else None)
    if counts:
        ops.vrt_head_counts(*args, p.cnt_text, p.cnt_patch, p.near, p.cpen, **more, **kw)
    else:
        ops.vrt_head_bias(*args, **more, **kw)
    if head != "plain":                                               # the fold of the LSE partials: padt_greedy_step_lp
        hid = torch.zeros(B, 8, device="cuda", dtype=BF)
        z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
        r.tok = torch.full((B, t_max), -9, dtype=torch.int64, device="cuda")
        ops.greedy_step(r.pv, r.pi, nblk, hid, torch.zeros(t_max, B, 8, device="cuda", dtype=BF), torch.ones(B, dtype=torch.int32, device="cuda"),
                        r.tok, torch.zeros(B, dtype=torch.int64, device="cuda"), st.clone(), z(B), z(B), z(3, B), EOS, PAD, gen_cfg=p.cfg,
                        part_sum=r.ps, logprobs=r.lp)
    torch.cuda.synchronize()
    for name, f in fl.items():
        assert guards_ok(f), f"guard words around {name} overwritten"
    return r


def specification(p, step, edits=True):
    from padt_amd.generation import count_penalty_row
    a_t = float(p.decay[step]) if (edits and step < T_DECAY) else 0.0
    return count_penalty_row(p.base[MODE_TABLE[step]], counts=p.counts_full, frequency_penalty=p.f[:, None], presence_penalty=p.p[:, None],
                             near=p.near_full, suppression_penalty=p.sp[:, None], bias=p.bias if edits else None, penalty=PEN, seen=p.seen_b,
                             banned=p.ban_b, eos_ids=(EOS, EOS2), a_t=a_t)


@X16
@pytest.mark.parametrize("layout", list(LAYOUT_V))
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("head", ["plain", "lse", "probe"])
def test_head_counts_is_the_specification_bit_for_bit(ops, problem, dt, layout, B, head):
    p = problem[(layout, B, dt)]
    V = p.V
    worst, dead = 0.0, 0
    for step in STEPS:
        for edits in ((True, False) if step in (0, 4) else (True,)):  # with and without bias / decay (null pointers under the EDIT flag)
            r = run(ops, p, layout == "packed", head, step, edits=edits)
            want = specification(p, step, edits)
            got = r.lg.cpu()
            assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(want).any())
            assert torch.equal(bits(got), bits(want)), f"step {step} edits {edits}: the written row is not the specification"
            best, idx = first_argmax(r.pv, r.pi, r.nblk, B)
            wbest = want.max(-1).values
            live = wbest > -INF                                       # a row whose every candidate ended at -inf has none
            dead += int((~live[:3]).sum())
            assert bool(live.all()) or MODE_TABLE[step] == 2
            widx = torch.stack([(want[b] == wbest[b]).nonzero()[0, 0] for b in range(B)])
            assert torch.equal(bits(best), bits(wbest)) and torch.equal(idx.long()[live], widx[live]), f"step {step}: partials"
            assert bool((idx[~live] == TS.SENTINEL).all())
            if head != "plain":
                assert torch.equal(r.tok[:, step].cpu()[live], widx[live]) and bool((r.tok[:, step].cpu()[~live] == PAD).all())
                worst = max(worst, within(r.lp[:, step].cpu()[live], ref_logprob(want, widx)[live]))
            if head == "probe":                                       # the probe value of a forced column whose count is > 0 carries the edit
                col = r.forced[:, step]
                has = col >= 0
                assert torch.equal(bits(r.probe.cpu()[has]), bits(want[torch.arange(B)[has], col[has]])), f"step {step}: probe_val"
                assert bool(torch.isnan(r.probe.cpu()[~has]).all())
            if step == 0 and edits:
                off = run(ops, p, layout == "packed", head, step, counts=False)
                assert not torch.equal(bits(off.lg), bits(r.lg)), "precondition: the counts change the row"
                assert float(want[0, 0]) != float(off.lg[0, 0]) and float(off.lg[0, 0]) > -INF      # the probe head's forced column of row 0
                assert bool((got[1, V + 5: V + 17][p.near_full[1, V + 5: V + 17] > 0] == -INF).all())      # penalty = +inf: -inf
                assert bool((got[0, V: V + 5] > -INF).any())
    assert dead >= 1, "precondition: row 2 has no candidate at the own-patches-only step (every patch suppressed with +inf)"
    print(f"\n[head_counts {head} B={B} {layout} {dt}] largest |LSE fold - fp64 log-softmax| {worst:.3e}")


def test_entry_points_validate_their_arguments(ops):
    from padt_amd._lib import load
    lib = load()
    P_ = 4096                                                         # fake non-null pointers: the calls are refused on the host
    call = lambda fn, ct=P_, ld=64, cp=P_, nr=P_, pen=P_, batch=2: fn(
        0, P_, 64, P_, 64, P_, 4, P_, 0, P_, 0, 0, P_, P_, batch, 64, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, ct, ld, cp, nr, pen)
    for fn in (lib.padt_vrt_head_counts, lib.padt_vrt_head_counts_f16):
        for bad in (dict(ct=0), dict(cp=0), dict(nr=0), dict(pen=0), dict(ld=62), dict(ld=60), dict(ct=P_ + 2)):
            assert call(fn, **bad) == -1 and b"padt_vrt_head_counts" in lib.padt_last_error(), bad
        assert call(fn, batch=0, ct=0) == 0
    upd = lambda tokens=P_, ld_tok=8, ld=52, vocab=50, near=P_, batch=3: lib.padt_count_update(0, tokens, ld_tok, P_, P_, P_, P_, P_, P_, ld, vocab,
                                                                                                P_, near, 13, batch)
    for bad in (dict(tokens=0), dict(near=0), dict(ld_tok=0), dict(ld=49), dict(vocab=0)):
        assert upd(**bad) == -1 and b"padt_count_update" in lib.padt_last_error(), bad
    assert upd(batch=0, tokens=0) == 0


# ------------------------------------------------------------------------------------------------------------ end to end
T_NEW, TEXT = TL.T_NEW, TL.TEXT
assert_same_run = SB.assert_same_run
GRIDS = [(5, 6), (4, 4)]                                              # two_ragged's merged patch grids (h/2, w/2) of [1, 10, 12] and [1, 8, 8]


@pytest.fixture(scope="module", params=["fp16", "bf16"])
def setup(request):
    """the model on one operand twin: every end-to-end test that takes it runs on both"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model(operands=request.param)
    return cfg, U, model, TL.two_ragged(cfg, U, seed=REPEAT_SEED)


class SpecProcessor:
    """The two specification functions as a caller's ``logits_processor``: count_state over each row's generated tokens — up to, and without,
    the token that ended it with an EOS id — then count_penalty_row's count and neighbourhood edits on the row the head wrote."""

    def __init__(self, model, L, grids, f=None, p=None, supp=None, bias=None, penalty=1.0, decay=None):
        """bias (a dict id → value), penalty and decay = (start, factor): the whole chain in the specified order — bias, repetition penalty,
        counts, neighbourhood, EOS decay — for a run whose own repetition penalty is 1 and that has no bias or decay of its own"""
        cfg = model.config
        self.bias, self.penalty, self.decay = bias, penalty, decay
        self.V, self.L, self.grids = cfg.vocab_size, L, grids
        B = len(grids)
        self.f, self.p, self.supp = f or [0.0] * B, p or [0.0] * B, supp or [None] * B
        listed = model.generation_config.eos_token_id                 # every id that ends a row: the config's and the generation config's
        self.eos = {int(cfg.eos_token_id)} | ({int(listed)} if isinstance(listed, int) else {int(e) for e in listed or ()})
        self.off = [0]
        for hp, wp in grids:
            self.off.append(self.off[-1] + hp * wp)

    def __call__(self, input_ids, scores):
        from padt_amd.generation import count_penalty_row, count_state
        from padt_amd.generation import decay_table
        out = scores.clone()
        n_cols = scores.shape[1]
        t = input_ids.shape[1] - self.L
        a_t = float(decay_table(self.decay, t + 1)[t]) if self.decay is not None else 0.0
        bias = None
        if self.bias is not None:
            bias = torch.zeros(n_cols, device=scores.device)
            for c, val in self.bias.items():
                bias[c] = val
        for b in range(scores.shape[0]):
            gen = input_ids[b, self.L:].tolist()
            n = next((i for i, t in enumerate(gen) if t in self.eos), len(gen))
            s = self.supp[b]
            count, near = count_state(gen, n, self.V, self.off[b], self.off[b + 1], self.grids[b], None if s is None else s[0])
            cvec = torch.zeros(n_cols, dtype=torch.int64)
            for c, k in count.items():
                cvec[c] = k
            nvec = torch.zeros(n_cols, dtype=torch.int64)
            nvec[self.V + self.off[b]: self.V + self.off[b + 1]] = torch.tensor(near, dtype=torch.int64)
            out[b] = count_penalty_row(scores[b], counts=cvec.to(scores.device), frequency_penalty=self.f[b], presence_penalty=self.p[b],
                                       near=nvec.to(scores.device), suppression_penalty=0.0 if s is None else s[1], bias=bias,
                                       penalty=self.penalty, seen=None if self.penalty == 1.0 else self.seen_mask(input_ids[b], n_cols),
                                       eos_ids=sorted(self.eos), a_t=a_t)
        return out


    @staticmethod
    def seen_mask(ids, n_cols):
        m = torch.zeros(n_cols, dtype=torch.bool, device=ids.device)
        m[ids] = True                                                 # HF's rule: every id of the row so far, prompt and padding included
        return m


REPEAT_SEED = 91                                                      # the batch whose free run repeats a token, on both operand twins: asserted below


def free_run_that_repeats(model, kw, gen):
    """→ the free run's tokens, which repeat a token in some row: the precondition under which a frequency penalty changes the run."""
    L = kw["input_ids"].shape[1]
    tok = model.generate(**gen, **kw).sequences[:, L:].cpu()
    assert any(len(set(r.tolist())) < len(r) for r in tok), f"precondition: the free run repeats no token: {tok.tolist()}"
    return tok


CP_MODES = {
    "greedy": dict(),
    "eager_steps": dict(use_graph=False),
    "sampling_with_a_warper": dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=11, min_p=0.05),
    "repetition_penalty_and_bans": dict(repetition_penalty=1.2, no_repeat_ngram_size=3, suppress_tokens=[22]),
}


@pytest.mark.parametrize("mode", list(CP_MODES))
def test_count_penalties_are_the_specification_on_the_hooked_loop(setup, mode):
    cfg, U, model, kw = setup
    gen = dict(dict(max_new_tokens=T_NEW, schedule=TEXT, output_scores=True, repetition_penalty=1.0), **CP_MODES[mode])
    free_tok = free_run_that_repeats(model, kw, dict(max_new_tokens=T_NEW, schedule=TEXT))
    L = kw["input_ids"].shape[1]
    got = model.generate(frequency_penalty=2.0, presence_penalty=1.0, **gen, **kw)
    assert got.past_key_values.mode.counts and not got.past_key_values.mode.processors
    spec = SpecProcessor(model, L, GRIDS, f=[2.0, 2.0], p=[1.0, 1.0])
    hooked = model.generate(logits_processor=[spec], **gen, **kw)
    assert hooked.past_key_values.mode.processors and not hooked.past_key_values.mode.counts
    assert_same_run(got, hooked)
    if mode == "greedy":
        assert not torch.equal(got.sequences[:, L:].cpu(), free_tok), "precondition: the penalties change the run"
    per_row = model.generate(frequency_penalty=[2.0, -1.0], presence_penalty=[0.0, 1.5], **gen, **kw)      # per-row values
    assert_same_run(per_row, model.generate(logits_processor=[SpecProcessor(model, L, GRIDS, f=[2.0, -1.0], p=[0.0, 1.5])], **gen, **kw))


def test_forced_tokens_count_and_token_logprobs(setup):
    cfg, U, model, kw = setup
    L = kw["input_ids"].shape[1]
    table = [[25, 25, 25], [35, 36, 35]]                              # then three free steps
    gen = dict(max_new_tokens=6, schedule=TEXT[:6], forced_tokens=table, output_token_logprobs=True, frequency_penalty=1.5, presence_penalty=0.5)
    scored = model.generate(output_scores=True, **gen, **kw)
    assert scored.past_key_values.mode.forced and scored.past_key_values.mode.counts      # the session's mode is the last call's: read it now
    fused = model.generate(**gen, **kw)                                # the probe head with the counts: no row in memory
    assert fused.past_key_values.mode.counts and fused.scores is None
    base = model.generate(output_scores=True, **dict(gen, frequency_penalty=None, presence_penalty=None), **kw)
    assert torch.equal(fused.sequences, scored.sequences)
    spec = SpecProcessor(model, L, GRIDS, f=[1.5, 1.5], p=[0.5, 0.5])
    hooked = model.generate(output_scores=True, logits_processor=[spec], **dict(gen, frequency_penalty=None, presence_penalty=None), **kw)
    assert_same_run(scored, hooked)
    # the forced prefix is the same with and without: the rows differ by the edit alone — a forced token counts like a selected one
    for t, n25 in ((1, 1), (2, 2)):
        f32 = lambda x: torch.tensor(x, dtype=torch.float32)
        want = (base.scores[t][0, 25].cpu() - f32(1.5) * f32(float(n25))) - f32(0.5)
        assert torch.equal(bits(scored.scores[t][0, 25].cpu()), bits(want))
    tok = scored.sequences[:, L:].cpu()
    ref = torch.stack([ref_logprob(scored.scores[t], tok[:, t]) for t in range(tok.shape[1])], 1)
    d = max(within(fused.token_logprobs, ref), within(scored.token_logprobs, ref), within(hooked.token_logprobs, ref))
    assert float(fused.token_logprobs[0, 2]) < float(base.token_logprobs[0, 2])
    print(f"\n[forced + counts] largest |token_logprobs - log_softmax(scores)| {d:.3e}")


def test_merged_decode_group_with_different_values_per_batch(setup):
    cfg, U, model, _ = setup
    from padt_amd import pipeline
    proc = SB.make_processor(cfg, U)
    batches = []
    for s, g in enumerate([[[1, 8, 8], [1, 10, 12]], [[1, 6, 10], [1, 8, 8]]]):
        grid, pix, ids, am = U.synthetic_batch(cfg, g, n_pre=5 + 3 * s, n_post=7, seed=100 + s, ragged=True)
        batches.append((ids.cuda(), am.cuda(), pix.cuda(), grid))
    T = 10
    sched = ["t"] * 3 + ["v"] * 2 + ["t"] * 2 + ["v"] * 2 + ["e"]
    vals = [dict(frequency_penalty=2.0, presence_penalty=[1.0, 0.0], patch_suppression=(1, INF)),
            dict(frequency_penalty=[0.5, -1.0], presence_penalty=2.0, patch_suppression=[None, (0, 3.0)])]
    gen = dict(max_new_tokens=T, schedule=sched, output_token_logprobs=True)
    alone = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], **v_, **gen) for b, v_ in zip(batches, vals)]
    plain = [pipeline.rec_batch(model, proc, b[0].clone(), *b[1:], **gen) for b in batches]
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)
    got = []
    for b, v_ in zip(batches, vals):
        got += runner.submit(b[0].clone(), *b[1:], **v_, **gen)
    got += runner.flush()
    assert runner.n_groups == 1 and len(got) == 2, "batches with different VALUES share a decode group"
    changed = 0
    for (d0, c0, l0, v0), (d1, c1, l1, v1), (_, cp, _, vp) in zip(alone, got, plain):
        assert c0 == c1 and v0 == v1, "tokens of the merged group differ from the batch alone"
        # a batch's patch columns sit in other 16-column blocks of the merged table, so the LSE partials regroup: the bound of
        # test_token_logprobs_gpu's merged-group test, for the same reason
        within(d1["token_logprobs"], d0["token_logprobs"])
        changed += (c0, v0) != (cp, vp)
    assert changed >= 1, "precondition: the edits change a batch's run"
    runner = pipeline.PipelinedRunner(model, proc, depth=2, merge=2)      # a batch with the feature and one without: groups of their own
    out = runner.submit(batches[0][0].clone(), *batches[0][1:], **vals[0], **gen)
    out += runner.submit(batches[1][0].clone(), *batches[1][1:], **gen)
    out += runner.flush()
    assert runner.n_groups == 2 and len(out) == 2
    assert out[0][1] == alone[0][1] and out[1][1] == plain[1][1]


def object_automaton():
    from padt_amd.generation import TokenAutomaton as TA
    return TA.from_sequences([[TA.TEXT, TA.VRT, TA.VRT, TA.TEXT, TA.VRT, TA.VRT]])      # from_sequences appends the EOS edge


def windows_hit(tok, V, lo, grid, radius):
    """does a VRT token of the second object (tokens 4, 5) lie within `radius` of one of the first object's (tokens 1, 2)?"""
    wp = grid[1]
    first = [divmod(int(t) - V - lo, wp) for t in tok[1:3]]
    second = [divmod(int(t) - V - lo, wp) for t in tok[4:6]]
    return any(max(abs(y - y0), abs(x - x0)) <= radius for y, x in second for y0, x0 in first)


def test_patch_suppression_keeps_the_second_object_off_the_first(setup):
    cfg, U, model, kw = setup
    V, L = cfg.vocab_size, kw["input_ids"].shape[1]
    A = object_automaton()
    gen = dict(max_new_tokens=7, token_automaton=A, output_scores=True)
    free = model.generate(**gen, **kw)
    ftok = free.sequences[:, L:].cpu()
    offs = [0, GRIDS[0][0] * GRIDS[0][1]]
    assert bool((ftok[:, [1, 2, 4, 5]] >= V).all()) and bool((ftok[:, [0, 3]] < V).all())       # the shape the automaton fixes
    assert any(windows_hit(ftok[b], V, offs[b], GRIDS[b], 1) for b in range(2)), \
        "precondition: without suppression a second object lands inside the first one's windows"
    got = model.generate(patch_suppression=(1, INF), **gen, **kw)
    assert got.past_key_values.mode.counts and got.past_key_values.mode.automaton
    tok = got.sequences[:, L:].cpu()
    for b in range(2):
        assert not windows_hit(tok[b], V, offs[b], GRIDS[b], 1), f"row {b}: the second object sits on the first one's patches"
    assert not bool(torch.isnan(torch.stack(got.scores)).any())
    hooked = model.generate(logits_processor=[SpecProcessor(model, L, GRIDS, supp=[(1, INF), (1, INF)])], **gen, **kw)
    assert_same_run(got, hooked)
    soft = model.generate(patch_suppression=[(2, 0.75), None], **gen, **kw)                     # a finite penalty, one row only
    assert_same_run(soft, model.generate(logits_processor=[SpecProcessor(model, L, GRIDS, supp=[(2, 0.75), None])], **gen, **kw))
    assert torch.equal(soft.sequences[1], free.sequences[1])


def test_off_is_off(setup):
    from padt_amd.generation import StepMode
    cfg, U, model, kw = setup
    gen = dict(max_new_tokens=T_NEW, schedule=TEXT, output_scores=True, output_token_logprobs=True)
    base = model.generate(**gen, **kw)
    sess = base.past_key_values
    mode, n_graphs = sess.mode, len(sess.graphs)
    assert mode == StepMode(keep_scores=True, token_logprobs=True) and not mode.counts
    on = model.generate(frequency_penalty=2.0, presence_penalty=1.0, patch_suppression=(1, INF), **gen, **kw)
    assert on.past_key_values is sess and sess.mode == mode._replace(counts=True) and len(sess.graphs) == n_graphs + 1
    model.generate(frequency_penalty=[0.5, 0.25], **gen, **kw)
    assert len(sess.graphs) == n_graphs + 1, "one captured graph serves every value"
    for off in (dict(), dict(frequency_penalty=None, presence_penalty=None, patch_suppression=None),
                dict(frequency_penalty=0.0, presence_penalty=[0.0, 0.0], patch_suppression=[None, None])):
        out = model.generate(**off, **gen, **kw)                      # after a call with the options: the parent's step, nothing left behind
        assert out.past_key_values is sess and sess.mode == mode and len(sess.graphs) == n_graphs + 1
        assert_same_run(base, out)
        assert torch.equal(bits(base.token_logprobs), bits(out.token_logprobs))
    plain = model.generate(max_new_tokens=T_NEW, schedule=TEXT, **kw)
    assert plain.past_key_values.mode == StepMode()
    with pytest.raises(NotImplementedError, match="output_logits"):
        model.generate(frequency_penalty=1.0, output_logits=True, max_new_tokens=4, **kw)


def test_reference_precision_keeps_the_same_head():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model(precision="reference")
    kw = TL.two_ragged(cfg, U)
    L = kw["input_ids"].shape[1]
    gen = dict(max_new_tokens=T_NEW, schedule=TEXT, output_scores=True)
    got = model.generate(frequency_penalty=2.0, presence_penalty=1.0, **gen, **kw)
    assert got.past_key_values.mode.counts and got.past_key_values.mode.reference
    assert_same_run(got, model.generate(logits_processor=[SpecProcessor(model, L, GRIDS, f=[2.0, 2.0], p=[1.0, 1.0])], **gen, **kw))


def test_counts_with_bias_repetition_penalty_and_decay_in_the_specified_order(setup):
    """mode.counts together with mode.bias: the counts head reads the session's bias vector and decay table too.  The hooked reference runs
    without any built-in edit (penalty 1, no bias, no decay) and applies the whole chain itself, in the specified order."""
    cfg, U, model, kw = setup
    L = kw["input_ids"].shape[1]
    eos = cfg.eos_token_id
    lb = {21: 7.25, 22: 5.0, 1500: 3.125, eos: 4.0, 30: -INF}
    decay = (2, 1.5)
    gen = dict(max_new_tokens=T_NEW, schedule=TEXT, output_scores=True)
    got = model.generate(frequency_penalty=[2.0, 0.5], presence_penalty=1.0, logit_bias=lb, exponential_decay_length_penalty=decay,
                         repetition_penalty=1.3, **gen, **kw)
    mode = got.past_key_values.mode
    assert mode.counts and mode.bias and not mode.processors
    spec = SpecProcessor(model, L, GRIDS, f=[2.0, 0.5], p=[1.0, 1.0], bias=lb, penalty=1.3, decay=decay)
    hooked = model.generate(logits_processor=[spec], repetition_penalty=1.0, exponential_decay_length_penalty=(0, 1.0), **gen, **kw)
    assert_same_run(got, hooked)
    no_counts = model.generate(logit_bias=lb, exponential_decay_length_penalty=decay, repetition_penalty=1.3, **gen, **kw)
    assert not torch.equal(no_counts.sequences, got.sequences), "precondition: the count edits change the biased run"
    assert bool((got.scores[0][:, 30] == -INF).all())


def test_bf16_rerun_keeps_the_three_arguments():
    """operands="auto": a batch whose SwiGLU hidden exceeds fp16's range is re-run on the bf16 twin WITH the batch's own penalties and
    suppression pairs — the result is the bf16 model's own run under them (the weight edit is test_range_guard_gpu.py's `llm_swiglu` case)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import padt_amd
    from padt_amd.modeling import PaDTForConditionalGeneration
    import parity_util as U
    cfg = padt_amd.small_test_config()
    w = U.bf16_weights(cfg, seed=21, std=0.05)
    for name, idx, val in (("model.layers.0.self_attn.o_proj.weight", (7, slice(None)), 8192.0), ("model.layers.1.mlp.gate_proj.weight", (3, 7), 32.0),
                           ("model.layers.1.mlp.up_proj.weight", (3, 7), 32.0)):
        w[name] = w[name].clone()
        w[name][idx] = val
    grid, pix, ids, am = U.synthetic_batch(cfg, [[1, 8, 8], [1, 10, 12]], n_pre=5, n_post=8, ragged=True, seed=41)
    kw = dict(input_ids=ids.cuda(), attention_mask=am.cuda(), pixel_values=pix.cuda(), image_grid_thw=grid)
    gen = dict(max_new_tokens=8, schedule=["t"] * 2 + ["v"] * 2 + ["t"] * 2 + ["v"] * 2)
    three = dict(frequency_penalty=[2.0, 0.5], presence_penalty=1.0, patch_suppression=[(1, INF), None])
    ref = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="bf16")
    free = ref.generate(**gen, **kw)
    want = ref.generate(**three, **gen, **kw)
    assert not torch.equal(want.sequences, free.sequences), "precondition: the three arguments change the bf16 model's run"
    auto = PaDTForConditionalGeneration(cfg, w, device="cuda", operands="auto")
    with pytest.warns(RuntimeWarning, match="re-run on the bf16"):
        got = auto.generate(**three, **gen, **kw)
    assert auto.overflow_reruns == 1 and torch.equal(got.sequences, want.sequences)
