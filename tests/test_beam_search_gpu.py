"""generate(beam_width=, n_best=, beam_length_penalty=, beam_early_stopping=) on the device.

Kernel level: padt_beam_step in lock-step with generation.beam_step, bit for bit, on crafted candidate tables (ties across and within
beams, EOS ids inside and outside the first K, -inf tails, dead beams, a sample done on entry, the last step), every state array between
guard words; padt_beam_reorder_kv against its contract on poisoned packed caches, over the whole buffers; padt_beam_finalize against
generation.beam_backtrace.

End to end, on the small synthetic model and the two ragged samples of the other generate suites, with an EOS logit_bias chosen from a free
run's own scores so that hypotheses finish at different lengths, and a schedule with a VRT run: width 1 against the greedy call; width 3
against a beam search driven from the host with beam_step over forced top_logprobs calls; every returned hypothesis re-scored with
score_completions and decoded with vl_decode; captured against eager steps; image_index and prefix= against the expanded call; the
refusals.  Without the feature generate() refuses beam_width as an unknown keyword and ops has none of the three bindings."""
import math
import types

import pytest
import torch

import test_forced_tokens_gpu as FT
import test_token_logprobs_gpu as TL
from padt_amd.generation import BEAM_EARLY, StepMode, beam_backtrace, beam_keep, beam_len_table, beam_new_state, beam_step

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD, GUARD_WORD = 4, 0x5A5A5A5A
i32 = TL.i32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


class Guarded:
    """an allocator for ops.BeamState whose every array sits between two runs of guard words"""

    def __init__(self):
        self.flats = {}

    def __call__(self, name, n, dt):
        flat = torch.full((2 * GUARD + n,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.flats[name] = flat
        view = flat[GUARD: GUARD + n].view(dt)
        view.zero_()
        return view

    def ok(self):
        return all(bool((f[:GUARD] == GUARD_WORD).all()) and bool((f[-GUARD:] == GUARD_WORD).all()) for f in self.flats.values())


# ------------------------------------------------------------------------------------------------------------ the beam step
STEP_V, STEP_T, STEP_D = 40, 7, 64           # text columns, the buffers' t_max (the call's last step is 5), hidden width
STEP_PATCHES = (4, 0, 6)                     # patches of the three samples; every beam row owns a copy
STEP_EOS = {1: (3,), 2: (3, 17)}
STEP_CASES = [(2, 1, 1.0, False), (3, 1, 0.7, True), (4, 1, 2.0, "never"), (2, 2, 0.7, "never"), (3, 2, 1.0, False), (4, 2, 0.0, True)]


def crafted_candidates(K, keep, eos, seed):
    """top_val / top_idx [3 * K][STEP_T][keep] as padt_topk_logprob_rows_f32 leaves them (descending, distinct columns, -1 / -inf tails), in
    SESSION columns (row r's patch j is STEP_V + vrt_off[r] + j) → (val, idx, vrt_off).  Values are multiples of 0.25, so sums are exact and
    ties abound, across beams and within one; EOS ids are placed at ranks inside and outside the first K; some rows run out of finite
    candidates early (sample 1's only live row at step 0 has ONE: K - 1 dead beams)."""
    g = torch.Generator().manual_seed(seed)
    R = 3 * K
    vrt_off = [0]
    for b in range(3):
        for _ in range(K):
            vrt_off.append(vrt_off[-1] + STEP_PATCHES[b])
    val = torch.full((R, STEP_T, keep), -INF)
    idx = torch.full((R, STEP_T, keep), -1, dtype=torch.int32)
    for r in range(R):
        b = r // K
        for t in range(STEP_T):
            n = keep
            u = float(torch.rand(1, generator=g))
            if u < 0.2:
                n = int(torch.randint(0, keep, (1,), generator=g))          # a -inf tail, possibly no candidate at all
            if b == 1 and t == 0:
                n = 1
            v = -0.25 * torch.randint(0, 12, (n,), generator=g).float()
            v = torch.sort(v, descending=True).values
            cols = torch.randperm(STEP_V + STEP_PATCHES[b], generator=g)[:n].tolist()
            cols = [c if c < STEP_V else c + vrt_off[r] for c in cols]
            for e in eos:                                                    # an EOS id at a random rank, in about half of the rows
                if b == 1 and t == 0:
                    continue
                if n and e not in cols and float(torch.rand(1, generator=g)) < 0.5:
                    cols[int(torch.randint(0, n, (1,), generator=g))] = e
            val[r, t, :n] = v
            idx[r, t, :n] = torch.tensor(cols, dtype=torch.int32)
    return val, idx, vrt_off


def lockstep(ops, K, n_eos, penalty, early, seed=3, rep_lp=True):
    """runs padt_beam_step for 6 steps next to generation.beam_step; asserts every array after every step → what the finalize test needs"""
    eos = STEP_EOS[n_eos]
    keep = beam_keep(K, n_eos)
    B, R, T_LAST, PAD = 3, 3 * K, 5, 39
    val, idx, vrt_off = crafted_candidates(K, keep, eos, seed + 10 * K + n_eos)
    alloc = Guarded()
    st = ops.BeamState(B, K, STEP_T, "cuda", own=alloc)
    table = beam_len_table(penalty, STEP_T)
    st.len_table.copy_(table)
    st.cfg.copy_(ops.beam_cfg_tensor(K, keep, BEAM_EARLY[early], T_LAST, early == "never" and penalty > 0))
    st.flags[2, 1] = 1                                                       # sample 2 is done on entry
    spec = [beam_new_state(K) for _ in range(B)]
    spec[2]["done"] = True
    gen_cfg = ops.gen_cfg_tensor(1.0, eos[1:], "cuda")
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(STEP_T, R, STEP_D, generator=g).to(torch.bfloat16).cuda()
    hflat = torch.full((2 * GUARD * STEP_D + STEP_T * R * STEP_D,), 0x5A5A, dtype=torch.int16, device="cuda")
    hbuf = hflat[GUARD * STEP_D: GUARD * STEP_D + STEP_T * R * STEP_D].view(torch.bfloat16).view(STEP_T, R, STEP_D)
    top_idx, top_val = idx.cuda(), val.cuda()
    # the log-probs the step REPORTS for its candidates (padt_beam_cand_lp's in a generate): other values than the ones it adds
    reported = (val - 0.001 * torch.rand(val.shape, generator=g)) if rep_lp else None
    unf, cur = torch.ones(R, dtype=torch.int32, device="cuda"), torch.full((R,), -7, dtype=torch.int64, device="cuda")
    step = i32([0])
    slot, lens, pos3, err = i32([20 + r for r in range(R)]), i32([21 + r for r in range(R)]), i32([[5 + r for r in range(R)]] * 3), i32([0])
    vo = i32(vrt_off)
    rec = dict(tok=[], parent=[], lp=[])
    seen = dict(dead=0, tie=0, fin_out=0, fin_in=0, done=0)
    for t in range(6):
        advance = t > 0
        ops.beam_step(st, top_idx, top_val, hidden[t].contiguous(), hbuf, unf, cur, step, slot, lens, pos3, vo, eos[0], PAD, STEP_V,
                      STEP_V + vrt_off[-1], advance=advance, gen_cfg=gen_cfg, err=err,
                      rep_lp=reported[:, t].contiguous().cuda() if rep_lp else None)
        torch.cuda.synchronize()
        assert alloc.ok() and bool((hflat[:GUARD * STEP_D] == 0x5A5A).all()) and bool((hflat[-GUARD * STEP_D:] == 0x5A5A).all())
        assert int(step) == t + 1 and int(err) == 0
        w_tok, w_par, w_lp, w_cur = [], [], [], []
        for b in range(B):
            rows = range(b * K, (b + 1) * K)
            was_done = spec[b]["done"]
            # the spec reads patch-local columns: row r's own patch j is STEP_V + j
            loc = [[(c if c < STEP_V else c - vrt_off[r]) for c in idx[r, t].tolist()] for r in rows]
            tok, par, lp, info = beam_step(spec[b], val[b * K: (b + 1) * K, t].tolist(), loc, t, keep, eos, table, T_LAST, early, pad=PAD,
                                           length_penalty=penalty, cand_rep=reported[b * K: (b + 1) * K, t].tolist() if rep_lp else None)
            w_tok += tok
            w_par += par
            w_lp += lp
            for c in range(K):                                             # the token as the column of the PARENT's copy of the prototypes
                live = spec[b]["live"][c] != -INF and not was_done
                w_cur.append(tok[c] if tok[c] < STEP_V or not live else tok[c] + vrt_off[b * K + par[c]])
            if not was_done:
                vs = [val[b * K + p, t, r].item() for p, r in info["order"]]
                seen["tie"] += len(set(vs)) < len(vs)
                seen["dead"] += sum(1 for x in spec[b]["live"] if x == -INF) if not spec[b]["done"] else 0
                seen["fin_in"] += sum(1 for i, f in enumerate(info["finishing"]) if f and i < K)
                seen["fin_out"] += sum(1 for i, f in enumerate(info["finishing"]) if f and i >= K)
                seen["done"] += spec[b]["done"]
        rec["tok"].append(w_tok), rec["parent"].append(w_par), rec["lp"].append(w_lp)
        f32 = lambda x: torch.tensor(x, dtype=torch.float32)
        assert torch.equal(st.beam_tok[t].cpu(), torch.tensor(w_tok, dtype=torch.int32)), t
        assert torch.equal(st.beam_parent[t].cpu(), torch.tensor(w_par, dtype=torch.int32)), t
        assert torch.equal(bits(st.beam_lp[t].cpu()), bits(f32(w_lp))), t
        assert torch.equal(st.perm.cpu(), torch.tensor(w_par, dtype=torch.int32)), t
        assert cur.cpu().tolist() == w_cur, t
        assert torch.equal(bits(st.live.cpu()), bits(f32([s["live"] for s in spec]))), t
        for j, name in enumerate(("st_score", "st_end", "st_parent", "st_tok", "st_lp")):
            want = [[e[j] for e in s["store"]] for s in spec]
            got = getattr(st, name).cpu()
            if got.dtype == torch.float32:
                assert torch.equal(bits(got), bits(f32(want))), (t, name)
            else:
                assert got.tolist() == want, (t, name)
        assert st.sent.cpu().tolist() == [[int(x) for x in s["sent"]] for s in spec], t
        flags = st.flags.cpu().tolist()
        assert [f[1] for f in flags] == [int(s["done"]) for s in spec], t
        assert all(f[0] == int(s["open"]) for f, s in zip(flags[:2], spec[:2])), t
        assert unf.cpu().tolist() == [0 if spec[r // K]["done"] else 1 for r in range(R)], t
        assert torch.equal(bits(hbuf[t]), bits(hidden[t])), t                # the step's hidden rows, every row
        assert bool((hflat[GUARD * STEP_D + (t + 1) * R * STEP_D: -GUARD * STEP_D] == 0x5A5A).all()), t      # and nothing past them
        adv = t                                                            # steps that advanced so far
        assert slot.cpu().tolist() == [20 + r + adv for r in range(R)] and lens.cpu().tolist() == [21 + r + adv for r in range(R)]
        assert pos3.cpu().tolist() == [[5 + r + adv for r in range(R)]] * 3
    return types.SimpleNamespace(st=st, spec=spec, rec=rec, hbuf=hbuf, hidden=hidden, K=K, seen=seen, pad=PAD, alloc=alloc)


@pytest.mark.parametrize("K,n_eos,penalty,early", STEP_CASES, ids=[f"K{k}-eos{n}-lp{p:g}-{e}" for k, n, p, e in STEP_CASES])
def test_beam_step_kernel_is_beam_step(ops, K, n_eos, penalty, early):
    r = lockstep(ops, K, n_eos, penalty, early)
    print(f"\n[beam step K={K}] seen {r.seen}")
    assert r.seen["dead"] and r.seen["fin_in"] and r.seen["done"], r.seen     # dead beams, finished hypotheses, a sample done
    assert all(s["done"] for s in r.spec)                                    # the last step finishes every sample
    assert all(not any(s["sent"]) for s in r.spec[2:])                       # the sample done on entry never moved


def test_the_crafted_tables_reach_every_case(ops):
    """... and the step without reported log-probs records the values it adds"""
    tot = dict(tie=0, fin_out=0)
    for K, n_eos, penalty, early in STEP_CASES:
        r = lockstep(ops, K, n_eos, penalty, early, rep_lp=False)
        for k in tot:
            tot[k] += r.seen[k]
    assert tot["tie"] > 0 and tot["fin_out"] > 0, tot


def test_beam_step_flags_a_column_outside_the_rows_table(ops):
    K, keep = 2, 4
    st = ops.BeamState(1, K, 3, "cuda")
    st.cfg.copy_(ops.beam_cfg_tensor(K, keep, 0, 2, False))
    top_idx = torch.full((K, 3, keep), -1, dtype=torch.int32)
    top_val = torch.full((K, 3, keep), -INF)
    top_idx[0, 0, :3] = torch.tensor([5, STEP_V + 2, STEP_V + 3])            # row 0 owns patches 0 .. 1: column V + 2 is row 1's, V + 3 nobody's
    top_val[0, 0, :3] = torch.tensor([-1.0, -2.0, -3.0])
    hidden, hbuf = torch.zeros(K, 8, dtype=torch.bfloat16, device="cuda"), torch.zeros(3, K, 8, dtype=torch.bfloat16, device="cuda")
    unf, cur, step, err = i32([1, 1]), torch.zeros(K, dtype=torch.int64, device="cuda"), i32([0]), i32([0])
    ops.beam_step(st, top_idx.cuda(), top_val.cuda(), hidden, hbuf, unf, cur, step, i32([4, 4]), i32([5, 5]), i32([[1, 1]] * 3), i32([0, 2, 4]),
                  3, 0, STEP_V, STEP_V + 4, advance=False, gen_cfg=None, err=err)
    assert int(err) == 1 and st.beam_tok[0].cpu().tolist() == [5, 0] and st.live.cpu().tolist() == [[-1.0, -INF]]
    # a config that does not describe the launch is reported and ends the sample
    st.cfg.copy_(ops.beam_cfg_tensor(K + 1, keep, 0, 2, False))
    err.zero_()
    ops.beam_step(st, top_idx.cuda(), top_val.cuda(), hidden, hbuf, unf, cur, step, i32([4, 4]), i32([5, 5]), i32([[1, 1]] * 3), i32([0, 2, 4]),
                  3, 0, STEP_V, STEP_V + 4, advance=False, gen_cfg=None, err=err)
    assert int(err) == 1 and unf.cpu().tolist() == [0, 0]


def test_candidate_log_probs_are_the_greedy_steps_fold(ops):
    """padt_beam_cand_lp on the LSE head's partials: the arg-max candidate gets padt_greedy_step_lp's bits, every other column
    (score - M) - log S with that S; -inf for a missing candidate and a -inf score"""
    g = torch.Generator().manual_seed(21)
    V, D, counts = 96, 256, (6, 4, 7)
    for dt in (torch.bfloat16, torch.float16):
        E = torch.randn(V, D, generator=g).to(dt).cuda()
        P = torch.randn(sum(counts), D, generator=g).to(dt).cuda()
        h = torch.randn(3, D, generator=g).to(dt).cuda()
        r = TL.fused(ops, h, E, P, [0, 6, 10, 17], packed=False, t_max=3, step=1)
        n_cols, keep = V + sum(counts), 5
        best = r.tok[:, 1].to(torch.int32)
        top_idx = torch.full((3, 3, keep), -1, dtype=torch.int32, device="cuda")
        top_idx[:, 1, 0] = best
        top_idx[:, 1, 1] = torch.tensor([4, 50, 95], dtype=torch.int32)
        top_idx[:, 1, 2] = torch.tensor([V + 1, V + 7, V + 12], dtype=torch.int32)      # own patch columns
        top_idx[:, 1, 3] = torch.tensor([V + 8, 2, V + 2], dtype=torch.int32)           # rows 0 and 2: another sample's patch, -inf in the row
        flat = torch.full((2 * GUARD + 3 * keep,), GUARD_WORD, dtype=torch.int32, device="cuda")
        out = flat[GUARD: GUARD + 3 * keep].view(torch.float32).view(3, keep)
        assert ops.beam_cand_lp(r.pv, r.pi, r.ps, r.nblk, r.lg, n_cols, top_idx, i32([1]), out) is out
        torch.cuda.synchronize()
        assert bool((flat[:GUARD] == GUARD_WORD).all()) and bool((flat[-GUARD:] == GUARD_WORD).all())
        assert torch.equal(bits(out[:, 0]), bits(r.lp[:, 1])), dt                        # the greedy step's own value
        lg = r.lg[:, :n_cols]
        M, logS = lg.max(1).values, -out[:, 0]
        for j in (1, 2, 3):
            v = lg.gather(1, top_idx[:, 1, j: j + 1].long())[:, 0]
            want = torch.where(v == -INF, v, (v - M) - logS)
            assert torch.equal(bits(out[:, j]), bits(want)), (dt, j)
        assert float(out[0, 3]) == -INF and float(out[2, 3]) == -INF and bool((out[:, 4] == -INF).all())


# ------------------------------------------------------------------------------------------------------------ the caches follow the beams
RE_K, RE_S, RE_D, RE_LAYERS = 3, 96, 128, 2
RE_P0 = (17, 40)
RE_PERMS = {"identity": ((0, 1, 2), (0, 1, 2)), "cycle": ((1, 2, 0), (2, 0, 1)), "002": ((0, 0, 2), (0, 0, 2)), "111": ((1, 1, 1), (1, 1, 1)),
            "one sample done": ((2, 2, 1), (0, 1, 2))}


def poisoned(shape, g):
    """random 16-bit patterns, NaNs and infinities included: the kernel moves bits"""
    return torch.randint(-2 ** 15, 2 ** 15 - 1, shape, generator=g, dtype=torch.int32).to(torch.int16)


@pytest.mark.parametrize("count", [0, 1, 15, 31])
@pytest.mark.parametrize("Hkv", [1, 2])
def test_reorder_moves_the_generated_slots_and_nothing_else(ops, Hkv, count):
    g = torch.Generator().manual_seed(100 * Hkv + count)
    R = 2 * RE_K
    for name, perms in RE_PERMS.items():
        k_rm = [poisoned((R, Hkv, RE_S, RE_D), g) for _ in range(RE_LAYERS)]              # row-major K (R, Hkv, S, D)
        v_rm = [poisoned((R, Hkv, RE_D, RE_S), g) for _ in range(RE_LAYERS)]              # transposed V (R, Hkv, D, S)
        kp = [ops.pack_k_cache(x.view(torch.bfloat16)).cuda().contiguous() for x in k_rm]
        vp = [ops.pack_vt_cache(x.view(torch.bfloat16)).cuda().contiguous() for x in v_rm]
        table = ops.beam_kv_table(kp, vp)
        perm = i32([p for s in perms for p in s])
        p0 = i32([RE_P0[r // RE_K] for r in range(R)])
        slot = i32([RE_P0[r // RE_K] + count for r in range(R)])
        ops.beam_reorder_kv(table, perm, p0, slot, 2, RE_K, Hkv, RE_D, RE_S, 32, rows=R)
        torch.cuda.synchronize()
        for layer in range(RE_LAYERS):
            k_new = ops.unpack_k_cache(kp[layer]).cpu().view(torch.int16)
            v_new = ops.unpack_vt_cache(vp[layer]).cpu().view(torch.int16).transpose(2, 3)      # → (R, Hkv, S, D) like K
            for what, new, old, tile in (("K", k_new, k_rm[layer], 16), ("V", v_new, v_rm[layer].transpose(2, 3), 32)):
                for b in range(2):
                    lo, hi = RE_P0[b], RE_P0[b] + count
                    moved = perms[b] != (0, 1, 2) and count > 0
                    t_lo, t_hi = (lo // tile * tile, -(-hi // tile) * tile) if moved else (0, 0)      # the touched tiles' slots
                    for c in range(RE_K):
                        child, parent = b * RE_K + c, b * RE_K + perms[b][c]
                        where = (name, what, layer, b, c)
                        if moved:
                            assert torch.equal(new[child, :, lo:hi], old[parent, :, lo:hi]), where      # the range: the parent's former bits
                            edge = list(range(t_lo, lo)) + list(range(hi, t_hi))
                            if edge:                                          # inside a touched tile, outside the range: child's or parent's
                                e_new, e_c, e_p = new[child][:, edge], old[child][:, edge], old[parent][:, edge]
                                assert bool(((e_new == e_c) | (e_new == e_p)).all()), where
                        assert torch.equal(new[child, :, :t_lo], old[child, :, :t_lo]), where         # everything else: bit-unchanged
                        assert torch.equal(new[child, :, t_hi:], old[child, :, t_hi:]), where


def test_reorder_refuses_what_it_cannot_move(ops):
    from padt_amd import _lib
    t = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    z = i32([0] * 9)
    for kw in (dict(head_dim=64), dict(s_max=80), dict(K=9)):
        a = dict(dict(K=2, head_dim=128, s_max=96), **kw)
        with pytest.raises(_lib.PaDTHipError, match="padt_beam_reorder_kv"):
            ops.beam_reorder_kv(t, z, z, z, 1, a["K"], 1, a["head_dim"], a["s_max"], 8)


# ------------------------------------------------------------------------------------------------------------ the back-trace
@pytest.mark.parametrize("K,n_eos,penalty,early,n_best", [(3, 1, 0.7, True, 3), (4, 2, 0.0, True, 2), (2, 1, 1.0, False, 1)])
def test_finalize_is_beam_backtrace(ops, K, n_eos, penalty, early, n_best):
    r = lockstep(ops, K, n_eos, penalty, early)
    B = 3
    counts = [STEP_PATCHES[i // n_best] for i in range(B * n_best)]
    off = [sum(counts[:i]) for i in range(B * n_best)]
    fin = ops.beam_finalize(r.st, n_best, r.hbuf, i32(off), r.pad, STEP_V)
    torch.cuda.synchronize()
    assert r.alloc.ok()
    some = 0
    for b in range(B):
        toks = [row[b * K: (b + 1) * K] for row in r.rec["tok"]]
        pars = [row[b * K: (b + 1) * K] for row in r.rec["parent"]]
        lps = [row[b * K: (b + 1) * K] for row in r.rec["lp"]]
        for j, h in enumerate(beam_backtrace(r.spec[b]["store"], toks, pars, lps, n_best)):
            i, n = b * n_best + j, h["length"]
            some += n > 0
            assert int(fin["lengths"][i]) == n
            assert torch.equal(bits(fin["scores"][i: i + 1].cpu()), bits(torch.tensor([h["score"]], dtype=torch.float32)))
            want_tok = [x + off[i] if x >= STEP_V else x for x in h["tokens"]] + [r.pad] * (STEP_T - n)
            assert fin["tokens"][i].cpu().tolist() == want_tok, (b, j)
            assert torch.equal(bits(fin["logprobs"][i].cpu()), bits(torch.tensor(h["logprobs"] + [0.0] * (STEP_T - n), dtype=torch.float32)))
            assert fin["src_row"][i].cpu().tolist() == [row for _, row in h["rows"]] + [-1] * (STEP_T - n)
            for t, row in h["rows"]:                                         # the hidden row that produced token t, from the step's stash
                assert torch.equal(bits(fin["hidden"][t, i]), bits(r.hidden[t, b * K + row])), (b, j, t)
            assert bool((bits(fin["hidden"][n:, i]) == 0).all())
    assert some >= 2                                                         # two samples finished hypotheses; the third returns empty ones
    assert int(fin["lengths"][2 * n_best]) == 0 and float(fin["scores"][2 * n_best]) == -INF


# ------------------------------------------------------------------------------------------------------------ end to end
T_NEW = 8
SCHED = ["t", "t", "v", "v", "t", "t", "t", "e"]              # a VRT run followed by text (what parseVRTintoCompletion closes an object on), EOS forced last
EOS_LIFTS = (1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0)              # on top of the greedy bias, for the wide searches (see `three`)


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, U, model = TL.small_model()
    kw = TL.two_ragged(cfg, U)
    L = kw["input_ids"].shape[1]
    eos = int(cfg.eos_token_id)
    # the EOS bias from a free run's own scores: just below the smallest gap between a text step's best score and its EOS score over the
    # first five steps — no greedy row ends there, and the EOS column is among the K best candidates of that step
    free = model.generate(max_new_tokens=T_NEW, schedule=SCHED, output_scores=True, **kw)
    gaps = []
    for t in range(5):
        for b in range(2):
            row = free.scores[t][b]
            if math.isfinite(float(row[eos])):
                gaps.append(float(row.max() - row[eos]))
    bias = min(gaps) - 0.05
    gen = dict(max_new_tokens=T_NEW, schedule=SCHED, logit_bias={eos: bias})
    e = types.SimpleNamespace(cfg=cfg, U=U, model=model, kw=kw, L=L, eos=eos, gen=gen, bias=bias, grid=kw["image_grid_thw"], V=cfg.vocab_size)
    e.n_patch = [int(g[1]) * int(g[2]) // 4 for g in e.grid.tolist()]
    print(f"\n[beam search] EOS bias {bias:.3f} (gaps {min(gaps):.3f} .. {max(gaps):.3f})")
    return e


def expanded(e, n):
    """the batch with every row repeated n times in place, sharing its image through image_index → (kw, the rows' patch offsets)"""
    kw = dict(e.kw, input_ids=e.kw["input_ids"].repeat_interleave(n, 0), attention_mask=e.kw["attention_mask"].repeat_interleave(n, 0),
              image_index=[b for b in range(2) for _ in range(n)])
    off = [0]
    for b in range(2):
        for _ in range(n):
            off.append(off[-1] + e.n_patch[b])
    return kw, off


def beam(e, gen=None, **kw):
    out = e.model.generate(**dict(gen or e.gen, output_token_logprobs=True, **kw), **e.kw)
    out["gen"] = gen or e.gen
    sess = out.past_key_values
    out["step_mode"] = sess.mode
    # the session's records, before another call on the same session starts over
    out["records"] = {k: getattr(sess.beam, k).clone().cpu() for k in ("beam_tok", "beam_parent", "st_end")}
    return out


def hidden_bits(out, n=None):
    return bits(out.hidden_states.last_layer_rows()[:n])


@pytest.fixture(scope="module")
def width_one(E):
    return E.model.generate(**E.gen, output_token_logprobs=True, **E.kw), beam(E, beam_width=1, beam_early_stopping=True)


def test_width_one_with_early_stopping_is_the_greedy_call(E, width_one):
    """(a) beam_width=1, beam_early_stopping=True: the store's one entry is the greedy row — sequences and hidden rows bit for bit (the
    token log-probs: the test below)."""
    e = E
    greedy, one = width_one
    assert one["step_mode"] == StepMode(bias=True, top_k=2, beam=1, token_logprobs=True)
    tok, lens = greedy.sequences[:, e.L:].cpu(), one.sequence_lengths.cpu().tolist()
    print(f"\n[width 1] greedy {tok.tolist()}\n[width 1] beam   {one.sequences[:, e.L:].cpu().tolist()} lengths {lens}")
    n = one.sequences.shape[1] - e.L
    assert n == max(lens) and torch.equal(one.sequences, greedy.sequences[:, : e.L + n])
    hb, hg = one.hidden_states.last_layer_rows(), greedy.hidden_states.last_layer_rows()
    for b, l in enumerate(lens):
        assert torch.equal(bits(hb[:l, b]), bits(hg[:l, b])), b
        assert bool((one.sequences[b, e.L + l:] == e.cfg.pad_token_id).all())
    print(f"[width 1] largest |token_logprobs - greedy's| {TL.within(one.token_logprobs, greedy.token_logprobs[:, :n]):.3e}")


def test_width_one_token_log_probs_are_the_greedy_calls_bit_for_bit(E, width_one):
    """(a), the token log-probs.  The log-probs a beam step REPORTS are padt_beam_cand_lp's: the greedy step's fold of the LSE head's block
    partials, not the top-k kernel's (v - M) - log S over column chunks, which rounds differently (by 1.0e-07 in 1 of these 16 entries) and
    which the search adds — so the host-driven search below is met in its scores and this call in its token log-probs, both to the bit."""
    e = E
    greedy, one = width_one
    n = one.sequences.shape[1] - e.L
    d = (one.token_logprobs - greedy.token_logprobs[:, :n]).abs().max().item()
    print(f"\n[width 1] largest |token_logprobs - greedy's| {d:.3e}, {int((bits(one.token_logprobs) != bits(greedy.token_logprobs[:, :n])).sum())} entries differ")
    assert torch.equal(bits(one.token_logprobs), bits(greedy.token_logprobs[:, :n])), f"token log-probs differ from the greedy call's by up to {d:.3e}"


def host_beam_search(e, gen, K, n_best, penalty, early):
    """the same search driven from the host with parent-commit features only: every step ONE forced call over the B * K live hypotheses with
    top_logprobs=keep gives each hypothesis' next candidates, generation.beam_step selects → per sample (state, toks, parents, lps)"""
    keep = beam_keep(K, 1)
    kw, off = expanded(e, K)
    table = beam_len_table(penalty, T_NEW)
    R = 2 * K
    states = [beam_new_state(K) for _ in range(2)]
    hyp = [[] for _ in range(R)]                                      # each row's live hypothesis, patch-local
    rec = [dict(tok=[], parent=[], lp=[]) for _ in range(2)]
    for t in range(T_NEW):
        forced = None
        if t:
            forced = [[x + off[r] if x >= e.V else x for x in hyp[r]] for r in range(R)]
        out = e.model.generate(**dict(gen, max_new_tokens=t + 1), forced_tokens=forced, top_logprobs=keep, **kw)
        ids, val = out.top_token_ids[:, t].cpu(), out.top_logprobs[:, t].cpu()
        new = [None] * R
        for b in range(2):
            rows = list(range(b * K, (b + 1) * K))
            loc = [[int(c) - off[r] if int(c) >= e.V else int(c) for c in ids[r].tolist()] for r in rows]
            tok, par, lp, _ = beam_step(states[b], val[rows].tolist(), loc, t, keep, (e.eos,), table, T_NEW - 1, early, pad=e.cfg.pad_token_id,
                                        length_penalty=penalty)
            rec[b]["tok"].append(tok), rec[b]["parent"].append(par), rec[b]["lp"].append(lp)
            for c in range(K):
                new[b * K + c] = hyp[b * K + par[c]] + [tok[c]]
        hyp = new
        if all(s["done"] for s in states):
            break
    return states, rec


def check_against_host(e, out, K, n_best, penalty, early, tag):
    states, rec = host_beam_search(e, out["gen"], K, n_best, penalty, early)
    recs = out["records"]
    off = [0]
    for b in range(2):
        for _ in range(n_best):
            off.append(off[-1] + e.n_patch[b])
    lengths, scores = out.sequence_lengths.cpu().tolist(), out.sequences_scores.cpu()
    gen = out.sequences[:, e.L:].cpu()
    for b in range(2):
        n_t = len(rec[b]["tok"])
        rows = slice(b * K, (b + 1) * K)
        assert recs["beam_tok"][:n_t, rows].tolist() == rec[b]["tok"], (tag, b, "tokens")
        assert recs["beam_parent"][:n_t, rows].tolist() == rec[b]["parent"], (tag, b, "parents")
        assert recs["st_end"][b].tolist() == [s[1] for s in states[b]["store"]], (tag, b, "finish steps")
        for j, h in enumerate(beam_backtrace(states[b]["store"], rec[b]["tok"], rec[b]["parent"], rec[b]["lp"], n_best)):
            i = b * n_best + j
            want = [x + off[i] if x >= e.V else x for x in h["tokens"]]
            print(f"[{tag}] sample {b} #{j}: score {h['score']:.6f} length {h['length']} tokens {want}")
            assert lengths[i] == h["length"] and gen[i, : h["length"]].tolist() == want, (tag, b, j)
            assert bool((gen[i, h["length"]:] == e.cfg.pad_token_id).all())
            assert float(scores[i]) == h["score"], (tag, b, j, float(scores[i]), h["score"])          # the same fp32 values in the same order
            TL.within(out.token_logprobs[i, : h["length"]], torch.tensor(h["logprobs"]))      # reported: the greedy step's fold, not the top-k kernel's
    assert gen.shape[1] == max(lengths)
    return states


@pytest.fixture(scope="module")
def three(E):
    """the K = 3, n_best = 3 call every test below reads; nothing here is modified by a test.  Under the default length penalty (the mean
    log-prob) a hypothesis that ends early must win its EOS step by about what a text step costs, or the store only ever holds full-length
    hypotheses; much more, and it holds nothing else.  The EOS bias is the first of EOS_LIFTS above the greedy one under which the returned
    hypotheses have different lengths and one of them holds a VRT run; early stopping "never", so that the search outlives a full store."""
    e = E
    for lift in EOS_LIFTS:
        gen = dict(e.gen, logit_bias={e.eos: e.bias + lift})
        out = beam(e, gen=gen, beam_width=3, n_best=3, beam_early_stopping="never")
        lengths = out.sequence_lengths.cpu().tolist()
        print(f"\n[beam search] EOS lift {lift}: lengths {lengths}")
        if len(set(lengths)) > 1 and bool((out.sequences[:, e.L:] >= e.V).any()):
            return out
    raise AssertionError("precondition: no EOS bias gives hypotheses of different lengths with a VRT run among them")


def test_three_beams_against_the_host_driven_search(E, three):
    """(b) tokens, parents, finish steps and scores of the device search equal the host-driven one"""
    e, out = E, three
    assert out["step_mode"] == StepMode(bias=True, top_k=6, beam=3, token_logprobs=True) and out.sequences.shape[0] == 6
    states = check_against_host(e, out, 3, 3, 1.0, "never", "K=3")
    lengths = out.sequence_lengths.cpu().tolist()
    assert len(set(lengths)) > 1 and max(lengths) > min(lengths), f"precondition: the hypotheses finish at different lengths: {lengths}"
    assert bool((out.sequences[:, e.L:] >= e.V).any()), "precondition: a hypothesis holds VRT tokens"
    assert all(all(s["sent"]) for s in states)
    sc = out.sequences_scores.view(2, 3).cpu()
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())                      # best first


def rescored(e, out, n_best):
    kw, _ = expanded(e, n_best)
    lengths = out.sequence_lengths.cpu().tolist()
    comp = [out.sequences[i, e.L: e.L + l].cpu().tolist() for i, l in enumerate(lengths)]
    gen = {k: v for k, v in out["gen"].items() if k != "max_new_tokens"}
    return e.model.score_completions(kw["input_ids"], kw["attention_mask"], kw["pixel_values"], kw["image_grid_thw"], comp,
                                     image_index=kw["image_index"], max_tokens=lengths, **gen), lengths, kw


def row_index_bound(e, out, n_best):
    """the fallback bound of the re-scoring test: twice the largest difference between two forced runs of the same rows at different row
    indices (the batch reversed), from features the parent commit has"""
    kw, _ = expanded(e, n_best)
    lengths = out.sequence_lengths.cpu().tolist()
    comp = [out.sequences[i, e.L: e.L + l].cpu().tolist() for i, l in enumerate(lengths)]
    gen = {k: v for k, v in out["gen"].items() if k != "max_new_tokens"}
    off, n = [0], len(comp)
    for b in range(2):
        for _ in range(n_best):
            off.append(off[-1] + e.n_patch[b])
    a = e.model.score_completions(kw["input_ids"], kw["attention_mask"], kw["pixel_values"], kw["image_grid_thw"], comp,
                                  image_index=kw["image_index"], max_tokens=lengths, **gen)
    # reversed: row i sits at n - 1 - i; its VRT ids move to that row's range
    r_off = [0]
    for i in reversed(range(n)):
        r_off.append(r_off[-1] + e.n_patch[i // n_best])
    rev = [[x - off[i] + r_off[n - 1 - i] if x >= e.V else x for x in comp[i]] for i in reversed(range(n))]
    flip = lambda t: t.flip(0)
    ids_local = kw["input_ids"].clone()
    for i in range(n):
        m = ids_local[i] >= e.V
        ids_local[i][m] -= off[i]
    ids_rev = flip(ids_local).clone()
    for j in range(n):
        m = ids_rev[j] >= e.V
        ids_rev[j][m] += r_off[j]
    b = e.model.score_completions(ids_rev, flip(kw["attention_mask"]), kw["pixel_values"], kw["image_grid_thw"], rev,
                                  image_index=list(reversed(kw["image_index"])), max_tokens=list(reversed(lengths)), **gen)
    d = 0.0
    for i, l in enumerate(lengths):
        d = max(d, float((a.token_logprobs[i, :l] - b.token_logprobs[n - 1 - i, :l]).abs().max()))
    return 2.0 * d


def test_rescoring_every_hypothesis_returns_its_hidden_rows(E, three):
    """(c) score_completions keeps an unpermuted cache: the rows of a hypothesis whose cache was permuted under it come back bit for bit,
    its token log-probs within test_token_logprobs_gpu.py's bound (their equality is the test below)."""
    e, out = E, three
    ref, lengths, _ = rescored(e, out, 3)
    assert all(torch.equal(ref.sequences[i, e.L: e.L + l], out.sequences[i, e.L: e.L + l]) for i, l in enumerate(lengths))
    hb, hr = out.hidden_states.last_layer_rows(), ref.hidden_states.last_layer_rows()
    for i, l in enumerate(lengths):
        assert torch.equal(bits(hb[:l, i]), bits(hr[:l, i])), f"hidden rows of hypothesis {i} differ from the forced re-run's"
        TL.within(out.token_logprobs[i, :l], ref.token_logprobs[i, :l])


def test_rescoring_every_hypothesis_returns_its_log_probs(E, three):
    """(c), the token log-probs: EQUAL, bit for bit, for every returned hypothesis — what padt_beam_cand_lp is there for.  Printed next to
    it, as a figure only: twice the largest difference between two forced runs of the same rows at different row indices (the rows
    reversed; measured on the MI355X: 2.09e-07), the bound equality would have fallen back to."""
    e, out = E, three
    ref, lengths, _ = rescored(e, out, 3)
    d_lp = max(float((out.token_logprobs[i, :l] - ref.token_logprobs[i, :l]).abs().max()) for i, l in enumerate(lengths))
    print(f"\n[re-score] largest |token_logprobs - score_completions'| {d_lp:.3e}; twice the row-index dependence of two forced runs "
          f"{row_index_bound(e, out, 3):.3e}")
    for i, l in enumerate(lengths):
        assert torch.equal(bits(out.token_logprobs[i, :l]), bits(ref.token_logprobs[i, :l])), \
            f"token log-probs of hypothesis {i} differ from score_completions' (largest difference {d_lp:.3e})"


def test_the_n_best_rows_decode_to_the_forced_reruns_boxes(E, three):
    """(d) parseVRTintoCompletion + vl_decode on the returned rows, image_grid_thw repeated"""
    e, out = E, three
    ref, lengths, kw = rescored(e, out, 3)
    grid = e.grid[[0, 0, 0, 1, 1, 1]]
    fa, da = FT.decode_objects(e.model, e.cfg, e.U, out, grid, e.L)
    fb, db = FT.decode_objects(e.model, e.cfg, e.U, ref, grid, e.L)
    assert [len(f) for f in fa] == [len(f) for f in fb] and sum(len(f) for f in fa) > 0, "precondition: the hypotheses decode objects"
    for k in ("pred_boxes", "pred_score", "pred_mask"):
        assert torch.equal(da[k], db[k]), k
    assert out.past_logit_mask.shape == ref.past_logit_mask.shape and torch.equal(out.past_logit_mask, ref.past_logit_mask)
    assert torch.equal(bits(out.past_image_embeds), bits(ref.past_image_embeds))


def same_beams(a, b, what):
    assert torch.equal(a.sequences, b.sequences), what
    assert torch.equal(bits(a.sequences_scores), bits(b.sequences_scores)) and torch.equal(a.sequence_lengths, b.sequence_lengths), what
    assert torch.equal(bits(a.token_logprobs), bits(b.token_logprobs)), what
    assert torch.equal(hidden_bits(a), hidden_bits(b)), what


def test_eager_steps_equal_the_captured_call_and_one_graph_serves_every_penalty(E, three):
    """(e)"""
    e = E
    sess = three.past_key_values
    g3 = three["gen"]
    eager = beam(e, gen=g3, beam_width=3, n_best=3, beam_early_stopping="never", use_graph=False)
    same_beams(three, eager, "captured / eager")
    n_graphs = len(sess.graphs)
    assert StepMode(bias=True, top_k=6, beam=3, token_logprobs=True) in sess.graphs
    other = beam(e, gen=g3, beam_width=3, n_best=2, beam_length_penalty=0.0, beam_early_stopping=True)
    assert other.past_key_values is sess and len(sess.graphs) == n_graphs      # the width's graph, replayed over another table and config
    same_beams(other, beam(e, gen=g3, beam_width=3, n_best=2, beam_length_penalty=0.0, beam_early_stopping=True, use_graph=False), "second call")
    check_against_host(e, other, 3, 2, 0.0, True, "K=3 lp=0 early")
    dflt = beam(e, gen=g3, beam_width=3, n_best=1, beam_length_penalty=2.0)
    assert len(sess.graphs) == n_graphs
    check_against_host(e, dflt, 3, 1, 2.0, False, "K=3 lp=2")
    # a plain call afterwards is the plain call
    plain = e.model.generate(**e.gen, **e.kw)
    assert plain.past_key_values.mode == StepMode(bias=True) and "sequences_scores" not in plain


def test_image_index_and_prefix_give_the_expanded_calls_result():
    """(f)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_prefix_cache_gpu as PC
    from prefix_cache_util import prefix_case
    cfg, U, model = TL.small_model()
    c = prefix_case(cfg)
    gen = dict(max_new_tokens=6, schedule=["t", "t", "v", "v", "t", None], beam_width=2, n_best=2, output_token_logprobs=True)
    full = model.generate(input_ids=c["q_ids"].cuda(), attention_mask=c["q_am"].cuda(), pixel_values=c["q_pix_x"].cuda(),
                          image_grid_thw=c["q_grid_x"], **gen)
    shared = model.generate(**gen, **PC.index_kw(c))
    same_beams(full, shared, "expanded / image_index")
    assert full.sequences.shape[0] == 12 and torch.equal(bits(full.past_image_embeds), bits(shared.past_image_embeds))
    # prefix=: its prompt pass runs at another row count, so the runs are equal up to the tile GEMM's rounding seen through the network —
    # test_prefix_cache_gpu.py's bounds for a prefix call against the image_index call, per quantity; the searches agree on these inputs
    handle = model.encode_prefix(*PC.prefix_inputs(c))
    with PC.no_vit(model):
        pref = model.generate(**gen, **PC.prefix_kw(c, handle))
    assert torch.equal(shared.sequences, pref.sequences) and torch.equal(shared.sequence_lengths, pref.sequence_lengths)
    assert torch.equal(shared.past_logit_mask, pref.past_logit_mask) and torch.equal(shared.past_high_res_image_embeds, pref.past_high_res_image_embeds)
    mx, rms = PC.rel_err(shared.hidden_states.last_layer_rows(), pref.hidden_states.last_layer_rows())
    assert rms < PC.tol(model, 2e-2, 3e-3) and mx < PC.tol(model, 8e-2, 1.2e-2), (mx, rms)
    # the log-probs, from the hidden-row difference actually there: a logit is a table row times the hidden row, so it moves by at most
    # |table row| x |difference of the hidden rows| (Cauchy-Schwarz; the two runs' prototype rows differ too: |difference of the table
    # rows| x |hidden row| on top) plus the fp32 accumulation's own rounding, D x 2^-24 of the largest logit; a log-softmax moves by at most
    # twice what its row moves by, and a mean of log-probs by no more than they do
    plain = model.generate(max_new_tokens=6, schedule=gen["schedule"], output_scores=True, **PC.index_kw(c))
    top = max(x[torch.isfinite(x)].abs().max().item() for x in plain.scores)
    hs, hp = shared.hidden_states.last_layer_rows().float(), pref.hidden_states.last_layer_rows().float()
    ps, pp = shared.past_image_embeds.float(), pref.past_image_embeds.float()
    w_max = max(model.W["llm.head"].float().norm(dim=1).max().item(), ps.norm(dim=1).max().item(), pp.norm(dim=1).max().item())
    d_logit = (w_max * (hs - hp).norm(dim=-1).max().item() + (ps - pp).norm(dim=1).max().item() * hs.norm(dim=-1).max().item()
               + cfg.hidden_size * 2.0 ** -24 * top)
    dl = (shared.token_logprobs - pref.token_logprobs).abs().max().item()
    ds = (shared.sequences_scores - pref.sequences_scores).abs().max().item()
    print(f"\n[prefix] max |d token log-prob| {dl:.3e}, max |d score| {ds:.3e}, bound {2 * d_logit:.3e}; hidden rows rel err max {mx:.3e} "
          f"rms {rms:.3e}, largest logit {top:.3e}")
    assert dl <= 2 * d_logit and ds <= 2 * d_logit


def test_rec_batch_and_the_pipelined_runner_carry_the_option(E, three):
    """The option through rec_batch and PipelinedRunner.submit(merge=2), between two plain batches: B x n_best completions and objects, the
    direct call's scores and log-probs and its rows' boxes bit for bit; the beam batch is a decode group of its own and the plain batches
    around it are what they are alone."""
    import padt_amd
    from padt_amd import pipeline
    e = E
    proc = padt_amd.VisonTextProcessingClass(e.U.FakeProcessor(e.cfg, 64), 2)
    proc.model_embed_token_size = e.cfg.vocab_size
    gen = {k: v for k, v in three["gen"].items() if k != "max_new_tokens"}
    on = dict(gen, beam_width=3, n_best=3, beam_early_stopping="never", output_token_logprobs=True)
    args = lambda: (e.kw["input_ids"].clone(), e.kw["attention_mask"], e.kw["pixel_values"], e.grid)
    decoded, completions, labels, vrts = pipeline.rec_batch(e.model, proc, *args(), max_new_tokens=T_NEW, **on)
    _, want = FT.decode_objects(e.model, e.cfg, e.U, three, e.grid[[0, 0, 0, 1, 1, 1]], e.L)
    assert len(completions) == len(labels) == len(vrts) == 6 and decoded["pred_boxes"].shape[0] > 0
    for k in ("pred_boxes", "pred_score", "pred_mask"):
        assert torch.equal(decoded[k], want[k]), k
    assert decoded["sample_idx"] == want["sample_idx"]
    assert torch.equal(bits(decoded["sequences_scores"]), bits(three.sequences_scores))
    assert torch.equal(decoded["sequence_lengths"], three.sequence_lengths)
    assert torch.equal(bits(decoded["token_logprobs"]), bits(three.token_logprobs))
    alone = pipeline.rec_batch(e.model, proc, *args(), max_new_tokens=T_NEW, **gen)
    assert len(alone[1]) == 2 and "sequences_scores" not in alone[0]
    runner = pipeline.PipelinedRunner(e.model, proc, depth=2, merge=2)
    got = []
    for kw in (gen, on, gen):
        got += runner.submit(*args(), max_new_tokens=T_NEW, **kw)
    got += runner.flush()
    assert len(got) == 3 and [len(g[1]) for g in got] == [2, 6, 2]
    for g, ref in zip(got, (alone, (decoded, completions, labels, vrts), alone)):
        assert g[1] == ref[1] and g[2] == ref[2] and g[3] == ref[3]
        for k in ("pred_boxes", "pred_score", "pred_mask"):
            assert torch.equal(g[0][k], ref[0][k]), k
    assert torch.equal(bits(got[1][0]["sequences_scores"]), bits(three.sequences_scores)) and "sequences_scores" not in got[0][0]


def test_the_refusals_hold_on_a_real_model(E):
    """(g)"""
    e = E
    for name, kw in (("do_sample", dict(do_sample=True, seed=1)), ("repetition_penalty", dict(repetition_penalty=1.3)),
                     ("no_repeat_ngram_size", dict(no_repeat_ngram_size=2)), ("forced_tokens", dict(forced_tokens=[[5], [6]])),
                     ("stop_sequences", dict(stop_sequences=[[4, 5]])), ("frequency_penalty", dict(frequency_penalty=0.5)),
                     ("top_logprobs", dict(top_logprobs=2)), ("output_patch_logprobs", dict(output_patch_logprobs=True)),
                     ("output_scores", dict(output_scores=True)), ("logits_processor", dict(logits_processor=[lambda i, s: s]))):
        with pytest.raises(NotImplementedError, match=r"beam_width[\s\S]*" + name):
            e.model.generate(**e.gen, beam_width=2, **kw, **e.kw)
    with pytest.raises(NotImplementedError, match="num_beams"):
        e.model.generate(**e.gen, num_beams=2, **e.kw)
    with pytest.raises(ValueError, match="n_best"):
        e.model.generate(**e.gen, beam_width=2, n_best=3, **e.kw)
    with pytest.raises(ValueError, match="beam_width"):
        e.model.generate(**e.gen, n_best=1, **e.kw)
    with pytest.raises(NotImplementedError, match="beam_width=9"):
        e.model.generate(**e.gen, beam_width=9, **e.kw)
    _, _, ref_model = TL.small_model(precision="reference")
    with pytest.raises(NotImplementedError, match=r"beam_width[\s\S]*precision"):
        ref_model.generate(**e.gen, beam_width=2, **e.kw)
