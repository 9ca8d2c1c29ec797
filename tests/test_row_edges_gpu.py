"""The row and glue kernels (csrc/elementwise.hip, the row passes of csrc/decoder_hp.hip) on strided windows in poisoned buffers, the
row locality of non-finite values, and one trip round every capped grid-stride loop.

The parity tests (test_kernels_gpu.py, test_kernels_f16_gpu.py, test_decoder_hp_gpu.py) hand these kernels contiguous, tightly sized
tensors with D = 1280 or 2048: a tail read one vector too far lands on the next row's finite numbers, a stray store lands in allocator
slack, all strides are equal.  Here every operand is a WINDOW (tests/edge_util.py): NaN around the inputs, a sentinel around the outputs
(-1234 for floats and int32, the byte 0xA5 for uint8), every 2-D window of a launch at a row stride of its own.  Two rules hold for
every case:
  * index, offset and size tensors are NEVER poisoned — idx, ids, img_index, slot, sample, lens, dst_*, pos3: their values are addresses.
    They are passed contiguous and in range.
  * every window keeps edge_util's margins (256 rows, 128 elements), so a kernel that overruns by a whole vector or row still stays
    inside its allocation and fails an assertion instead of faulting.
Every window case goes through three(): (1) the NaN-poisoned run meets the reference; (2) it is bit-identical to the zero-filled run;
(3) nothing outside any output window changed.  Tolerances are the ones each kernel's parity test uses, unchanged: close_bf16 / close_f16
at ulps = 1, close_f32, rel_err < 2e-6 and split_close for the fp32 / split kernels of decoder_hp (rope_half_f32: 1e-6, row_rstd: 2e-6 of
the largest value, as their parity tests), bit equality for everything that only moves data, for add_rows against (a.float() +
b.float()).to(dt) and for the casts.  References are the plain torch statement in fp32 / fp64 on the device, on the operands given.

Shapes.  x16 grid: rows {1, 5, 37} x D {8, 520, 1280} — five rows leave the last block one live wave of four, D = 8 is one lane, 520 one
full 512-column pass plus one lane; fp32 grid: rows {1, 5, 37} x D {4, 260, 1280}.

Locality (test_nonfinite_values_stay_in_their_row): contiguous clean 9-row operands, one planted value in row r in {0, 2, 8} (first row,
a row with live neighbours in its block, the lone row of the last block).  NaN: every element of row r of every output is NaN; +inf: row
r of every output holds a non-finite value (RMSNorm: inf x rstd 0 = NaN at the plant, 0 elsewhere in the row, as the torch statement);
every other row is bit-identical to the clean run.  One exception is stated, not hidden: row_rstd of a row with +inf is rsqrt(inf) = 0,
finite, in the kernel as in the torch statement — the test asserts that 0 (the GEMM it scales turns the inf accumulator into NaN).
quant_rows_fp8 reports a non-finite row through its row scale (NaN, asserted); the e4m3 codes of row r themselves are bytes without a
non-finite meaning and are asserted only for the other rows (bit-identical).

Grid-stride wrap (test_grid_stride_loops_wrap): each capped grid (the cap is named next to its case, read from the entry point) gets one
contiguous case just past cap x 256 work items with a ragged remainder.  The largest (swiglu_split) holds 400 MB of operands; no case
needs more than 1 GB, so none is left out.
"""
import pytest
import torch

from edge_util import MIN_COLS, Failures, same_bits, three
from test_decoder_hp_gpu import join, rel_err, split_close, split_ref
from test_kernels_f16_gpu import close_f16
from test_kernels_gpu import close_bf16, close_f32

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
X16 = pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
X16_GRID = [(r, d) for r in (1, 5, 37) for d in (8, 520, 1280)]
F32_GRID = [(r, d) for r in (1, 5, 37) for d in (4, 260, 1280)]
gelu, silu = torch.nn.functional.gelu, torch.nn.functional.silu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from padt_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------ helpers
def rnd(dt, *shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


def wgt(dt, D, seed=0):
    return (1 + 0.1 * rnd(F32, D, seed=seed)).to(dt)


def blank(rows, cols, dt):
    return torch.full((rows, cols), 3, dtype=dt, device="cuda")


def i32(v):
    return torch.as_tensor(v, dtype=torch.int32).cuda().contiguous()


def close16(out, ref, what, ulps=1.0):
    (close_bf16 if out.dtype == BF else close_f16)(out, ref, what, ulps=ulps)


def distinct(*ts):
    lds = [t.stride(0) for t in ts if t is not None and t.dim() == 2]
    assert len(set(lds)) == len(lds), lds


def rms_ref(s, w, eps=1e-6):
    return w.float() * s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + eps)


# ------------------------------------------------------------------------------------------------------------ norms
@X16
def test_rmsnorm_on_windows(ops, dt):
    """padt_rmsnorm: plain, + GELU, + the repeat-4 add (5 and 37 rows: the last add row serves one row), and D smaller than the window
    (the 16 columns behind D hold 100: read, they would change the statistics)."""
    fails = Failures()
    for rows, D in X16_GRID:
        x, w = rnd(dt, rows, D, seed=1), wgt(dt, D, seed=2)
        add = rnd(dt, (rows + 3) // 4, D, seed=3)
        wide = torch.cat([x, torch.full((rows, 16), 100.0, dtype=dt, device="cuda")], dim=1)
        s_add = x.float() + add.float().repeat_interleave(4, 0)[:rows]
        for var in ("plain", "gelu", "add", "D < width"):
            if var == "add" and rows == 1:
                continue
            ref = {"plain": rms_ref(x.float(), w), "gelu": gelu(rms_ref(x.float(), w)), "add": rms_ref(s_add, w), "D < width": rms_ref(x.float(), w)}[var]
            tag = f"rmsnorm {var} {rows}x{D}"

            def body(ar):
                X, W, Y = ar.inp(wide if var == "D < width" else x), ar.inp(w), ar.out(blank(rows, D, dt))
                A = ar.inp(add) if var == "add" else None
                distinct(X, Y, A)
                ops.rmsnorm(X, W, out=Y, add=A, add_div=4 if var == "add" else 1, D=D, gelu=var == "gelu")
                return {"y": Y}
            three(fails, tag, body, lambda got: close16(got["y"], ref, tag))
    fails.done()


@X16
def test_layernorm_row_rstd_quant_rows_on_windows(ops, dt):
    """padt_layernorm, padt_row_rstd (fp32 vector output), padt_quant_rows_fp8 with and without the folded norm (uint8 codes in a byte-sentinel
    window at a stride of its own, fp32 row scales in a vector window)."""
    fails = Failures()
    for rows, D in X16_GRID:
        x, w, b = rnd(dt, rows, D, seed=4), wgt(dt, D, seed=5), rnd(dt, D, seed=6)
        xf = x.float()
        ln_ref = torch.nn.functional.layer_norm(xf, (D,), w.float(), b.float(), 1e-5)
        tag = f"layernorm {rows}x{D}"

        def body(ar):
            X, W, Bv, Y = ar.inp(x), ar.inp(w), ar.inp(b), ar.out(blank(rows, D, dt))
            distinct(X, Y)
            ops.layernorm(X, W, Bv, out=Y, eps=1e-5)
            return {"y": Y}
        three(fails, tag, body, lambda got: close16(got["y"], ln_ref, tag))

        rstd_ref = torch.rsqrt(xf.pow(2).mean(-1) + 1e-6)
        tag = f"row_rstd {rows}x{D}"

        def body(ar):
            return {"rstd": ops.row_rstd(ar.inp(x), eps=1e-6, out=ar.out(torch.full((rows,), 3.0, device="cuda")))}

        def check(got):
            err = (got["rstd"] - rstd_ref).abs().max().item()
            assert err <= 2e-6 * rstd_ref.abs().max().item(), f"{tag}: max err {err:.3e}"
        three(fails, tag, body, check)

        q_ref, sc_ref, _ = ops.quantize_fp8_rows(x)
        for eps in (None, 1e-6):
            tag = f"quant_rows_fp8 {rows}x{D} norm_eps={eps}"

            def body(ar):
                X, Q, RS = ar.inp(x), ar.out(blank(rows, D, torch.uint8)), ar.out(torch.full((rows,), 3.0, device="cuda"))
                distinct(X, Q)
                ops.quant_rows_fp8(X, norm_eps=eps, out=Q, rs=RS)
                return {"q": Q, "rs": RS}

            def check(got):
                assert torch.equal(got["q"], q_ref), f"{tag}: {int((got['q'] != q_ref).sum())} codes differ"
                want = sc_ref if eps is None else sc_ref * rstd_ref
                if eps is None:
                    assert torch.equal(got["rs"], want), f"{tag}: row scales differ"
                else:
                    assert bool(((got["rs"] - want).abs() <= 2e-6 * want.abs()).all()), f"{tag}: row scale x rstd"
            three(fails, tag, body, check)
    fails.done()


@X16
def test_rmsnorm_f32_on_windows(ops, dt):
    fails = Failures()
    for rows, D in F32_GRID:
        x, w = rnd(F32, rows, D, scale=2.0, seed=7), wgt(dt, D, seed=8)
        ref = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w.float()
        tag = f"rmsnorm_f32 {rows}x{D}"

        def body(ar):
            X, W, Y = ar.inp(x), ar.inp(w), ar.out(blank(rows, D, dt))
            distinct(X, Y)
            ops.rmsnorm_f32(X, W, out=Y, eps=1e-6)
            return {"y": Y}
        three(fails, tag, body, lambda got: close16(got["y"], ref, tag))
    fails.done()


def test_layernorm_f32_on_windows(ops):
    """padt_layernorm_f32: fp32 rows, bf16 weight and bias, against the fp64 statement."""
    fails = Failures()
    for rows, D in F32_GRID:
        x, w, b = rnd(F32, rows, D, scale=2.0, seed=9) + 0.5, wgt(BF, D, seed=10), rnd(BF, D, seed=11)
        ref = torch.nn.functional.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-5)
        tag = f"layernorm_f32 {rows}x{D}"

        def body(ar):
            X, W, Bv, Y = ar.inp(x), ar.inp(w), ar.inp(b), ar.out(blank(rows, D, F32))
            distinct(X, Y)
            ops.layernorm_f32(X, W, Bv, eps=1e-5, out=Y)
            return {"y": Y}

        def check(got):
            assert rel_err(got["y"], ref) < 2e-6, f"{tag}: rel err {rel_err(got['y'], ref):.2e}"
        three(fails, tag, body, check)
    fails.done()


@pytest.mark.parametrize("x_f32", [True, False], ids=["x32", "x16"])
def test_norm_split_on_windows(ops, x_f32):
    """padt_norm_split with every stage on (gather, repeat-4 add, norm, GELU, pos with pos_rows = 5; y0 fp32, y1 split at chunk D and
    D / 4; D = 260 with chunk 260) and the pass-through form."""
    rows, src_rows = 37, 50
    fails = Failures()
    for D, chunk in ((1280, 1280), (1280, 320), (260, 260)):
        x = rnd(F32, src_rows, D, seed=12)
        if not x_f32:
            x = x.to(BF)
        idx = i32(torch.randint(0, src_rows, (rows,), generator=torch.Generator().manual_seed(3)))
        add, w, pos = rnd(F32, (rows + 3) // 4, D, seed=13), wgt(BF, D, seed=14), rnd(F32, 5, D, seed=15)
        ar_rows = torch.arange(rows, device="cuda")
        xs = x.double()[idx.long()] + add.double()[ar_rows // 4]
        ref0 = gelu(xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double())
        ref1 = ref0 + pos.double()[ar_rows % 5]
        tag = f"norm_split all stages D={D} chunk={chunk}"

        def body(ar):
            X, A, W, P = ar.inp(x), ar.inp(add), ar.inp(w), ar.inp(pos)
            Y0, Y1 = ar.out(blank(rows, D, F32)), ar.out(blank(rows, 2 * D, BF))
            distinct(X, A, P, Y0, Y1)
            ops.norm_split(X, W, eps=1e-6, act=1, idx=idx, add=A, add_div=4, pos=P, y0_mode=ops.OUT_F32, y1_mode=ops.OUT_SPLIT, chunk=chunk,
                           y0=Y0, y1=Y1)
            return {"y0": Y0, "y1": Y1}

        def check(got):
            assert rel_err(got["y0"], ref0) < 2e-6, f"{tag}: y0 rel err {rel_err(got['y0'], ref0):.2e}"
            split_close(join(got["y1"], D, chunk), ref1, tag + " y1")
        three(fails, tag, body, check)
    x = rnd(F32, rows, 260, seed=16)
    tag = "norm_split pass-through"

    def body(ar):
        X, Y0 = ar.inp(x if x_f32 else x.to(BF)), ar.out(blank(rows, 520, BF))
        ops.norm_split(X, y0=Y0)
        return {"y0": Y0}

    def check(got):
        assert torch.equal(got["y0"], split_ref(x if x_f32 else x.to(BF).float())), f"{tag}: not the exact split of the input"
    three(fails, tag, body, check)
    fails.done()


def test_swiglu_split_on_windows(ops):
    fails = Failures()
    for rows in (1, 37):
        for I in (4, 260):
            gu = rnd(F32, rows, 2 * I, scale=2.0, seed=17)
            ref = silu(gu[:, :I].double()) * gu[:, I:].double()
            tag = f"swiglu_split {rows}x{I}"

            def body(ar):
                G, Y = ar.inp(gu), ar.out(blank(rows, 2 * I, BF))
                distinct(G, Y)
                ops.swiglu_split(G, I, out=Y)
                return {"y": Y}
            three(fails, tag, body, lambda got: split_close(join(got["y"], I), ref, tag))
    fails.done()


# ------------------------------------------------------------------------------------------------------------ adds, casts, gathers
@X16
def test_add_rows_and_casts_on_windows(ops, dt):
    fails = Failures()
    for rows, b_rows in ((5, 5), (24, 8), (37, 5)):                  # plain add; rows a multiple of b_rows; rows % b_rows != 0
        for D in (8, 520):
            a, b = rnd(dt, rows, D, seed=18), rnd(dt, b_rows, D, seed=19)
            ref = (a.float() + b.float()[torch.arange(rows, device="cuda") % b_rows]).to(dt)
            tag = f"add_rows {rows}x{D} b_rows={b_rows}"

            def body(ar):
                A, Bw, Y = ar.inp(a), ar.inp(b), ar.out(blank(rows, D, dt))
                distinct(A, Bw, Y)
                ops.add_rows(A, Bw, out=Y)
                return {"y": Y}

            def check(got):
                assert same_bits(got["y"], ref), f"{tag}: {int((got['y'] != ref).sum())} elements differ from (a + b).to(dt)"
            three(fails, tag, body, check)
    s = ops.stream_scale(dt)
    for rows, D in X16_GRID:
        x = rnd(F32, rows, D, scale=3.0, seed=20)
        for D_pad in (D, D + 8):
            for scale in (1.0, s):
                ref = torch.zeros(rows, D_pad, dtype=dt, device="cuda")
                ref[:, :D] = x.to(dt) if scale == 1.0 else (x * scale).to(dt)
                tag = f"cast_f32_x16 {rows}x{D} D_pad={D_pad} scale={scale}"

                def body(ar):
                    X, Y = ar.inp(x), ar.out(blank(rows, D_pad, dt))
                    distinct(X, Y)
                    ops.cast_f32_x16(X, D_pad, out=Y, scale=scale)
                    return {"y": Y}

                def check(got):
                    assert same_bits(got["y"], ref), f"{tag}: {int((got['y'] != ref).sum())} elements differ (pad columns must be +0)"
                three(fails, tag, body, check)
        x16 = rnd(dt, rows, D, seed=21)
        tag = f"cast_x16_f32 {rows}x{D}"

        def body(ar):
            X, Y = ar.inp(x16), ar.out(blank(rows, D, F32))
            distinct(X, Y)
            ops.cast_x16_f32(X, out=Y)
            return {"y": Y}

        def check(got):
            assert same_bits(got["y"], x16.float()), f"{tag}: not x.float()"
        three(fails, tag, body, check)
    fails.done()


@X16
def test_gather_scatter_rows_on_windows(ops, dt):
    """padt_gather_rows (16-bit rows), padt_gather_rows_f32 (also D = 41, no multiple of 4), padt_scatter_rows_f32.  Repeated indices; D
    smaller than the source's width; the scatter's destination rows not named by idx keep their bits."""
    fails = Failures()
    n_src, n = 20, 37
    idx = i32(torch.randint(0, n_src, (n,), generator=torch.Generator().manual_seed(5)))
    assert idx.unique().numel() < n                                  # repeated indices
    for sdt, width, D in ((dt, 520, 520), (dt, 528, 520), (dt, 8, 8), (F32, 260, 260), (F32, 48, 41), (F32, 41, 41)):
        src = rnd(sdt, n_src, width, seed=22)
        tag = f"gather_rows {sdt} width {width} D={D}"

        def body(ar):
            S, Y = ar.inp(src), ar.out(blank(n, D, sdt))
            distinct(S, Y)
            ops.gather_rows(S, idx, out=Y, D=D)
            return {"y": Y}

        def check(got):
            assert same_bits(got["y"], src[idx.long(), :D].contiguous()), f"{tag}: not src[idx]"
        three(fails, tag, body, check)
    if dt == BF:                                                     # fp32 only: once
        n_dst = 50
        where = i32(torch.randperm(n_dst, generator=torch.Generator().manual_seed(6))[:n])
        for width, D in ((260, 260), (264, 260), (4, 4)):
            src, dst0 = rnd(F32, n, width, seed=23), rnd(F32, n_dst, D, seed=24)
            ref = dst0.clone()
            ref[where.long()] = src[:, :D]
            tag = f"scatter_rows_f32 width {width} D={D}"

            def body(ar):
                S, Y = ar.inp(src), ar.out(dst0)
                distinct(S, Y)
                ops.scatter_rows_f32(S, where, Y, D=D)
                return {"y": Y}

            def check(got):
                assert same_bits(got["y"], ref), f"{tag}: {int((got['y'] != ref).sum())} elements differ (rows not in idx must keep their bits)"
            three(fails, tag, body, check)
    fails.done()


@X16
@pytest.mark.parametrize("M", [5, 16, 37])
def test_pack_rows_on_windows(ops, dt, M):
    """padt_pack_rows both ways: the row-major side a strided window, the packed side a slab of ceil(M / 16) blocks.  Rows < M are
    asserted against the layout statement packed[block][chunk][row % 16][8] = rows[16 block + row % 16][8 chunk ..]; the stale rows of
    the last block hold the poison on the way in, and nothing outside the blocks may change on the way out."""
    K, M16 = 520, (M + 15) // 16 * 16
    x = rnd(dt, M, K, seed=25)
    fails = Failures()

    def unpacked(img):
        return img.view(M16 // 16, K // 8, 16, 8).permute(0, 2, 1, 3).reshape(M16, K)[:M]

    def body(ar):
        X, P = ar.inp(x), ar.out(blank(M16, K, dt), slab=True)
        ops.pack_rows(X, P, M, to_packed=True)
        return {"rows": unpacked(P)}
    three(fails, f"pack_rows to packed M={M}", body, lambda got: _bits_eq(got["rows"], x, "packed rows < M"))

    def body(ar):
        full = torch.full((M16, K), float("nan") if ar.poison else 0.0, dtype=dt, device="cuda")
        full[:M] = x
        img = full.view(M16 // 16, 16, K // 8, 8).permute(0, 2, 1, 3).contiguous().view(M16, K)
        P, Y = ar.inp(img, slab=True), ar.out(blank(M, K, dt))
        ops.pack_rows(P, Y, M, to_packed=False)
        return {"rows": Y}
    three(fails, f"pack_rows to row-major M={M}", body, lambda got: _bits_eq(got["rows"], x, "unpacked rows"))
    fails.done()


def _bits_eq(got, ref, what):
    assert same_bits(got.contiguous(), ref.contiguous()), f"{what}: {int((got != ref).sum())} of {ref.numel()} elements differ"


@X16
def test_embed_tokens_on_slabs(ops, dt):
    """padt_embed_tokens takes no strides: both tables, image_embeds and out are slabs.  ids from all three sources, the error flag
    stays 0; with one id = V + n_proto the flag becomes 1 and every other row is what it was."""
    V, NP, NI, D, T = 40, 7, 6, 520, 37
    E, P, I = rnd(dt, V, D, seed=26), rnd(dt, NP, D, seed=27), rnd(dt, NI, D, seed=28)
    ids = torch.randint(0, V + NP, (T,), generator=torch.Generator().manual_seed(7)).cuda()
    ids[3], ids[4] = V - 1, V + NP - 1
    img = torch.full((T,), -1, dtype=torch.int32)
    img[10:10 + NI] = torch.arange(NI, dtype=torch.int32)
    img = img.cuda()
    ref = torch.cat([E, P])[ids]
    ref[10:10 + NI] = I
    fails = Failures()
    for bad in (False, True):
        ids_in = ids.clone()
        if bad:
            ids_in[20] = V + NP
        tag = f"embed_tokens{' with an id past the table' if bad else ''}"

        def body(ar):
            out = ar.out(blank(T, D, dt), slab=True)
            err = ar.out(torch.zeros(1, dtype=torch.int32, device="cuda"))
            ops.embed_tokens(ids_in, img, ar.inp(E, slab=True), ar.inp(P, slab=True), ar.inp(I, slab=True), out=out, err_flag=err)
            return {"out": out, "err": err}

        def check(got):
            assert int(got["err"]) == (1 if bad else 0), f"{tag}: error flag {int(got['err'])}"
            keep = torch.arange(T, device="cuda") != 20 if bad else torch.ones(T, dtype=torch.bool, device="cuda")
            _bits_eq(got["out"][keep], ref[keep], tag)
        three(fails, tag, body, check)
    fails.done()


@pytest.mark.parametrize("xdt", [F32, BF, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("rpf", [1, 4])
def test_check_finite_on_windows(ops, xdt, rpf):
    """padt_check_finite, all three kinds: a clean window surrounded by NaN leaves every flag 0 (the most direct over-read detector
    here); one planted inf sets exactly its row's flag."""
    rows, cols = 37, 260 if xdt == F32 else 520
    x = rnd(xdt, rows, cols, seed=29)
    n_flags = (rows + rpf - 1) // rpf
    fails = Failures()
    for plant in (None, (0, 0), (36, cols - 1), (17, cols // 2)):
        xp = x.clone()
        want = torch.zeros(n_flags, dtype=torch.int32, device="cuda")
        if plant is not None:
            xp[plant] = float("inf")
            want[plant[0] // rpf] = 1
        tag = f"check_finite {xdt} rows_per_flag={rpf} inf at {plant}"

        def body(ar):
            flags = ar.out(torch.zeros(n_flags, dtype=torch.int32, device="cuda"))
            ops.check_finite(ar.inp(xp), flags, rows_per_flag=rpf)
            return {"flags": flags}

        def check(got):
            assert torch.equal(got["flags"], want), f"{tag}: flags {got['flags'].nonzero().view(-1).tolist()}, want {want.nonzero().view(-1).tolist()}"
        three(fails, tag, body, check)
    fails.done()


# ------------------------------------------------------------------------------------------------------------ rotary
def rope_ref(x, cos, sin, H, D):
    """fp32 rotate-half over the first H * D columns of x, cos / sin (T, >= D / 2)"""
    T, half = x.shape[0], D // 2
    ref = x.float().clone()
    v = ref[:, : H * D].view(T, H, D)
    c, s = cos[:, None, :half], sin[:, None, :half]
    x1, x2 = v[..., :half].clone(), v[..., half:].clone()
    v[..., :half] = x1 * c - x2 * s
    v[..., half:] = x2 * c + x1 * s
    return ref


def _tables(T, width, seed):
    """cos / sin (T, width): the leading columns of ONE (T, 64) draw, so that tables of different widths hold the same angles"""
    ang = torch.rand(T, 64, generator=torch.Generator().manual_seed(seed)).cuda()[:, :width] * 50
    return ang.cos().contiguous(), ang.sin().contiguous()


@X16
def test_rope_half_vector_and_scalar_paths_on_windows(ops, dt):
    """padt_rope_half in place on a window with 16 pass-through columns behind the heads.  (H, D) = (3, 80) at aligned strides takes the
    16-byte kernel; the scalar kernel is reached by D = 72 (D % 16), D = 40, a table stride of 299 (no
    multiple of 4; table widths 41 and 42) and an x window that starts 4 elements in (8-byte aligned).  The D = 80 data gives the same
    bits through both kernels (common.h: "the SAME two roundings at every rope site")."""
    T, H = 37, 3
    fails = Failures()
    got80 = {}
    for name, D, width, ld_cs, c0 in (("vector", 80, 40, None, MIN_COLS), ("scalar D=72", 72, 36, None, MIN_COLS), ("scalar D=40", 40, 20, None, MIN_COLS),
                                      ("scalar ld_cs=299 width 41", 80, 41, 299, MIN_COLS), ("scalar ld_cs=299 width 42", 80, 42, 299, MIN_COLS),
                                      ("scalar x 4 elements in", 80, 40, None, MIN_COLS + 4)):
        x = rnd(dt, T, H * D + 16, seed=30)
        cos, sin = _tables(T, width, 31)
        ref = rope_ref(x, cos, sin, H, D)
        tag = f"rope_half {name}"

        def body(ar):
            X = ar.out(x, c0=c0)
            Cs = ar.inp(cos, ld=ld_cs)
            Sn = ar.inp(sin, ld=Cs.stride(0))                        # the entry point takes ONE table stride
            assert X.stride(0) % 8 == 0 and X.data_ptr() % 16 == (8 if c0 != MIN_COLS else 0) and Cs.stride(0) % 4 == (3 if ld_cs else 0)
            ops.rope_half_(X, Cs, Sn, H, D)
            return {"x": X}

        def check(got, name=name, D=D, ref=ref, tag=tag):
            close16(got["x"], ref, tag)
            assert same_bits(got["x"][:, H * D:], x[:, H * D:]), f"{tag}: the columns behind the heads changed"
            if D == 80:
                got80[name] = got["x"].clone()
        three(fails, tag, body, check)
    with fails.step("rope_half: D = 80 through the vector and the scalar kernel"):
        for name, v in got80.items():
            assert same_bits(v, got80["vector"]), f"{name}: {int((v != got80['vector']).sum())} elements differ from the vector kernel's"
        assert len(got80) == 4
    fails.done()


def test_rope_half_f32_on_windows(ops):
    T, H, D = 37, 3, 80
    x = rnd(F32, T, H * D + 16, seed=32)
    cos, sin = _tables(T, 41, 33)
    ref = x.double()
    ref[:, : H * D] = _rope64(x[:, : H * D], cos, sin, H, D)
    fails = Failures()

    def body(ar):
        X, Cs = ar.out(x), ar.inp(cos, ld=299)
        Sn = ar.inp(sin, ld=299)
        ops.rope_half_f32_(X, Cs, Sn, H, D)
        return {"x": X}

    def check(got):
        assert rel_err(got["x"], ref) < 1e-6, f"rope_half_f32: rel err {rel_err(got['x'], ref):.2e}"
        assert same_bits(got["x"][:, H * D:], x[:, H * D:])
    three(fails, "rope_half_f32", body, check)
    fails.done()


# ------------------------------------------------------------------------------------------------------------ llm_qkv_post
def mrope_ref(x, pos, inv, sec):
    """x (T, H, D) → fp32 mRoPE: angle of pair d = pos[axis(d)][t] * inv[d], axis by the sections over D / 2"""
    D = x.shape[-1]
    half = D // 2
    axis = torch.tensor([0] * sec[0] + [1] * sec[1] + [2] * (half - sec[0] - sec[1]), device="cuda")
    ang = pos.float()[axis].T * inv[None, :]                         # (T, half)
    c, s = ang.cos()[:, None], ang.sin()[:, None]
    x = x.float()
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


SECTIONS = {128: (16, 24, 24), 64: (8, 12, 12), 72: (12, 12, 12)}


def qkv_case(ops, fails, dt, Hq, Hkv, D, form, k_pack, packed, q_ld_odd, results=None, mis=None):
    """One launch of padt_llm_qkv_post.  form "slot": T = 11 tokens of two samples at listed slots; "lens": one token per sample at
    slot lens[b].  qkv, q_out and k_pack are windows, the caches slabs of random bits whose unaddressed slots must survive.
    mis: "qkv" / "q" / "k_pack" — that window starts 4 elements in (an 8-byte-aligned base at strides that are multiples of 8)."""
    B, S = (2, 32) if form == "slot" else (5, 32)
    T = 11 if form == "slot" else B
    sec = SECTIONS[D]
    qkv = rnd(dt, T, (Hq + 2 * Hkv) * D, seed=40)
    pos = i32(torch.randint(0, 600, (3, T), generator=torch.Generator().manual_seed(8)))
    inv = (1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))).cuda()
    if form == "slot":
        sample, slot, lens = i32([0] * 6 + [1] * 5), i32([3, 4, 5, 6, 7, 31] + [0, 1, 2, 16, 17]), None
        b_of, s_of = sample.tolist(), slot.tolist()
    else:
        sample, slot, lens = None, None, i32([0, 7, 31, 16, 15])
        b_of, s_of = list(range(B)), lens.tolist()
    kc0, vt0 = rnd(dt, B * Hkv * S, D, seed=41), rnd(dt, B * Hkv * D, S, seed=42)
    qr = mrope_ref(qkv[:, : Hq * D].view(T, Hq, D), pos, inv, sec).reshape(T, -1)
    kr = mrope_ref(qkv[:, Hq * D: (Hq + Hkv) * D].view(T, Hkv, D), pos, inv, sec)
    vv = qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)
    tag = f"llm_qkv_post Hq{Hq} Hkv{Hkv} D{D} {form}{' k_pack' if k_pack else ''}{' packed caches' if packed else ''}{' odd ld_q' if q_ld_odd else ''}" \
          f"{f' {mis} 4 elements in' if mis else ''}"

    def body(ar):
        X = ar.inp(qkv, c0=MIN_COLS + (4 if mis == "qkv" else 0))
        Q = ar.out(blank(T, Hq * D, dt), ld=MIN_COLS + Hq * D + MIN_COLS + 4 if q_ld_odd else None, c0=MIN_COLS + (4 if mis == "q" else 0))
        KP = ar.out(blank(T, Hkv * D, dt), c0=MIN_COLS + (4 if mis == "k_pack" else 0)) if k_pack else None
        KC, VT = ar.out(kc0, slab=True), ar.out(vt0, slab=True)
        distinct(X, Q, KP)
        assert (Q.stride(0) % 8 != 0) == q_ld_odd
        for name, t in (("qkv", X), ("q", Q), ("k_pack", KP)):
            assert t is None or t.data_ptr() % 16 == (8 if mis == name else 0)
        assert mis is None or all(t is None or t.stride(0) % 8 == 0 for t in (X, Q, KP))
        ops.llm_qkv_post(X, pos, inv, Q, KC.view(B, Hkv, S, D), VT.view(B, Hkv, D, S), Hq, Hkv, D, S, sec, sample=sample, slot=slot, lens=lens,
                         k_pack=KP, cache_packed=packed)
        out = {"q": Q, "kc": KC, "vt": VT}
        if k_pack:
            out["kp"] = KP
        return out

    def check(got):
        close16(got["q"], qr, tag + " q")
        kc, vt = got["kc"].view(B, Hkv, S, D), got["vt"].view(B, Hkv, D, S)
        kc_init, vt_init = kc0.view(B, Hkv, S, D), vt0.view(B, Hkv, D, S)
        if packed:
            kc, vt, kc_init, vt_init = ops.unpack_k_cache(kc), ops.unpack_vt_cache(vt), ops.unpack_k_cache(kc_init), ops.unpack_vt_cache(vt_init)
        want_v, hit = vt_init.clone(), torch.zeros(B, S, dtype=torch.bool, device="cuda")
        for t in range(T):
            want_v[b_of[t], :, :, s_of[t]] = vv[t]
            hit[b_of[t], s_of[t]] = True
        _bits_eq(vt, want_v, tag + " V^T cache")
        k_new = torch.stack([kc[b_of[t], :, s_of[t]] for t in range(T)])                       # (T, Hkv, D)
        close16(k_new, kr, tag + " k in the cache")
        _bits_eq(kc.transpose(1, 2)[~hit], kc_init.transpose(1, 2)[~hit], tag + " unaddressed K slots")
        if k_pack:
            _bits_eq(got["kp"].view(T, Hkv, D), k_new, tag + " k_pack vs the cache")
        if results is not None:
            results[tag] = (got["q"].clone(), k_new.clone())
    three(fails, tag, body, check)
    return tag


@X16
def test_llm_qkv_post_on_windows(ops, dt):
    """Slot-list and lens forms, k_pack on and off, row-major and fragment-packed caches at (Hq, Hkv, D) = (4, 2, 128) and (3, 1, 64); the
    scalar branch through a q_out stride that is no multiple of 8, through D = 72 on row-major caches, and — at strides and a head width
    the 16-byte branch accepts — through a qkv, q_out or k_pack window that starts 4 elements in (an 8-byte-aligned base: the entry
    point's alignment terms alone decide); the D = 128 data gives identical bits through both branches."""
    fails = Failures()
    res = {}
    for Hq, Hkv, D in ((4, 2, 128), (3, 1, 64)):
        for form in ("slot", "lens"):
            for k_pack in (False, True):
                for packed in (False, True):
                    qkv_case(ops, fails, dt, Hq, Hkv, D, form, k_pack, packed, False, res if (D == 128 and form == "slot" and k_pack and not packed) else None)
    t_vec = list(res)[0] if res else None
    qkv_case(ops, fails, dt, 4, 2, 128, "slot", True, False, True, res)
    for mis in ("qkv", "q", "k_pack"):
        qkv_case(ops, fails, dt, 4, 2, 128, "slot", True, False, False, res, mis=mis)
    qkv_case(ops, fails, dt, 4, 2, 128, "lens", False, True, True)
    qkv_case(ops, fails, dt, 3, 1, 72, "slot", True, False, False)
    qkv_case(ops, fails, dt, 3, 1, 72, "lens", False, False, False)
    with fails.step("llm_qkv_post: scalar and vector branch, same bits at D = 128"):
        assert len(res) == 5 and t_vec in res, list(res)
        for t, (q_s, k_s) in res.items():
            _bits_eq(q_s, res[t_vec][0], t + ": q")
            _bits_eq(k_s, res[t_vec][1], t + ": k")
    fails.done()


@X16
def test_llm_qkv_post_shared_on_windows(ops, dt):
    """padt_llm_qkv_post_shared: fan-out of every token's roped K / V to cache slots and join-buffer rows, a skipped destination (sample
    out of range, join row -1), both cache forms, vector and scalar branch (odd q_out stride; D = 72; a qkv, q_out, k_join or v_join
    window that starts 4 elements in) with identical bits at D = 128."""
    fails = Failures()
    res = {}
    for Hq, Hkv, D, packed, q_ld_odd, mis in ((4, 2, 128, False, False, None), (4, 2, 128, True, False, None), (4, 2, 128, False, True, None),
                                              (3, 1, 64, False, False, None), (3, 1, 64, True, False, None), (3, 1, 72, False, False, None),
                                              (4, 2, 128, False, False, "qkv"), (4, 2, 128, False, False, "q"), (4, 2, 128, False, False, "kj"),
                                              (4, 2, 128, False, False, "vj")):
        B, S, T, n_join = 3, 32, 5, 9
        sec = SECTIONS[D]
        qkv = rnd(dt, T, (Hq + 2 * Hkv) * D, seed=43)
        pos = i32(torch.randint(0, 600, (3, T), generator=torch.Generator().manual_seed(9)))
        inv = (1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))).cuda()
        off = [0, 2, 3, 3, 6, 8]                                       # token 2 has no destination
        d_sample = [0, 1, 2, 0, 1, 7, 2, 0]                           # destination 5: sample 7 is out of range → its cache write is skipped
        d_slot = [4, 4, 31, 5, 5, 0, 16, 15]
        d_row = [0, 1, 8, 2, -1, 3, 4, 5]                             # destination 4: no join row
        kc0, vt0 = rnd(dt, B * Hkv * S, D, seed=44), rnd(dt, B * Hkv * D, S, seed=45)
        qr = mrope_ref(qkv[:, : Hq * D].view(T, Hq, D), pos, inv, sec).reshape(T, -1)
        kr = mrope_ref(qkv[:, Hq * D: (Hq + Hkv) * D].view(T, Hkv, D), pos, inv, sec)
        vv = qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)
        tok_of = [t for t in range(T) for _ in range(off[t + 1] - off[t])]
        tag = f"llm_qkv_post_shared Hq{Hq} Hkv{Hkv} D{D}{' packed caches' if packed else ''}{' odd ld_q' if q_ld_odd else ''}" \
              f"{f' {mis} 4 elements in' if mis else ''}"

        def body(ar, mis=mis, q_ld_odd=q_ld_odd):
            c0 = lambda name: MIN_COLS + (4 if mis == name else 0)
            X = ar.inp(qkv, c0=c0("qkv"))
            Q = ar.out(blank(T, Hq * D, dt), ld=MIN_COLS + Hq * D + MIN_COLS + 4 if q_ld_odd else None, c0=c0("q"))
            KJ, VJ = ar.out(blank(n_join, Hkv * D, dt), c0=c0("kj")), ar.out(blank(n_join, Hkv * D, dt), c0=c0("vj"))
            KC, VT = ar.out(kc0, slab=True), ar.out(vt0, slab=True)
            distinct(X, Q, KJ, VJ)
            for name, t in (("qkv", X), ("q", Q), ("kj", KJ), ("vj", VJ)):
                assert t.data_ptr() % 16 == (8 if mis == name else 0) and (q_ld_odd or t.stride(0) % 8 == 0)
            ops.llm_qkv_post_shared(X, pos, inv, Q, KC.view(B, Hkv, S, D), VT.view(B, Hkv, D, S), KJ, VJ, i32(off), i32(d_sample), i32(d_slot),
                                    i32(d_row), Hq, Hkv, D, S, sec, cache_packed=packed)
            return {"q": Q, "kj": KJ, "vj": VJ, "kc": KC, "vt": VT}

        def check(got, tag=tag, D=D, packed=packed, q_ld_odd=q_ld_odd, mis=mis):
            close16(got["q"], qr, tag + " q")
            kc, vt = got["kc"].view(B, Hkv, S, D), got["vt"].view(B, Hkv, D, S)
            kc_init, vt_init = kc0.view(B, Hkv, S, D), vt0.view(B, Hkv, D, S)
            if packed:
                kc, vt, kc_init, vt_init = ops.unpack_k_cache(kc), ops.unpack_vt_cache(vt), ops.unpack_k_cache(kc_init), ops.unpack_vt_cache(vt_init)
            want_v, hit = vt_init.clone(), torch.zeros(B, S, dtype=torch.bool, device="cuda")
            want_vj, k_rows = blank(n_join, Hkv * D, dt), {}
            for n, t in enumerate(tok_of):
                if d_sample[n] < B:
                    want_v[d_sample[n], :, :, d_slot[n]] = vv[t]
                    hit[d_sample[n], d_slot[n]] = True
                    k_rows.setdefault(t, []).append(kc[d_sample[n], :, d_slot[n]])
                if 0 <= d_row[n] < n_join:
                    want_vj[d_row[n]] = vv[t].reshape(-1)
                    k_rows.setdefault(t, []).append(got["kj"][d_row[n]].view(Hkv, D))
            _bits_eq(vt, want_v, tag + " V^T cache")
            _bits_eq(got["vj"], want_vj, tag + " v_join")
            for t, rows in k_rows.items():
                close16(rows[0], kr[t], f"{tag} k of token {t}")
                for r in rows[1:]:
                    _bits_eq(r, rows[0], f"{tag}: every destination of token {t} receives the same K bits")
            _bits_eq(kc.transpose(1, 2)[~hit], kc_init.transpose(1, 2)[~hit], tag + " unaddressed K slots")
            used = sorted(r for r in d_row if r >= 0)
            free = [r for r in range(n_join) if r not in used]
            _bits_eq(got["kj"][free], blank(len(free), Hkv * D, dt), tag + " unaddressed k_join rows")
            if D == 128 and not packed:
                res["odd ld_q" if q_ld_odd else (mis or "vector")] = (got["q"].clone(), got["kj"].clone())
        three(fails, tag, body, check)
    with fails.step("llm_qkv_post_shared: scalar and vector branch, same bits at D = 128"):
        assert set(res) == {"vector", "odd ld_q", "qkv", "q", "kj", "vj"}, list(res)
        for name, (q_s, k_s) in res.items():
            _bits_eq(q_s, res["vector"][0], name + ": q")
            _bits_eq(k_s, res["vector"][1], name + ": k_join")
    fails.done()


# ------------------------------------------------------------------------------------------------------------ locality
def _row_outputs(ops, name, dt, x):
    """the outputs of one one-wave-per-row kernel on the contiguous 9-row input x (fp32 for the *_f32 kernels and norm_split)"""
    D = x.shape[1]
    w16, b16 = wgt(dt, D, seed=50), rnd(dt, D, seed=51)
    if name == "rmsnorm":
        return {"y": ops.rmsnorm(x, w16), "gelu": ops.rmsnorm(x, w16, gelu=True), "add": ops.rmsnorm(x, w16, add=rnd(dt, 3, D, seed=52), add_div=4)}
    if name == "layernorm":
        return {"y": ops.layernorm(x, w16, b16)}
    if name == "row_rstd":
        return {"rstd": ops.row_rstd(x).view(-1, 1)}
    if name == "quant_rows_fp8":
        q, rs = ops.quant_rows_fp8(x)
        q2, rs2 = ops.quant_rows_fp8(x, norm_eps=1e-6)
        return {"rs": rs.view(-1, 1), "rs norm": rs2.view(-1, 1), "codes": q, "codes norm": q2}
    if name == "rmsnorm_f32":
        return {"y": ops.rmsnorm_f32(x, w16)}
    if name == "layernorm_f32":
        return {"y": ops.layernorm_f32(x, wgt(BF, D, seed=50), rnd(BF, D, seed=51))}
    assert name == "norm_split"
    y0, y1 = ops.norm_split(x, wgt(BF, D, seed=50), act=1, add=rnd(F32, 3, D, seed=52), add_div=4, pos=rnd(F32, 5, D, seed=53),
                            y0_mode=ops.OUT_F32, y1_mode=ops.OUT_SPLIT)
    return {"y0": y0, "y1": y1}


ROW_KERNELS = [("rmsnorm", "x16"), ("layernorm", "x16"), ("row_rstd", "x16"), ("quant_rows_fp8", "x16"), ("rmsnorm_f32", "x16"),
               ("layernorm_f32", "bf16"), ("norm_split", "bf16")]


@pytest.mark.parametrize("name,dt", [(n, t) for n, k in ROW_KERNELS for t in ([BF, F16] if k == "x16" else [BF])],
                         ids=lambda v: v if isinstance(v, str) else {BF: "bf16", F16: "fp16"}[v])
def test_nonfinite_values_stay_in_their_row(ops, name, dt):
    """The module docstring has the rules.  D = 520 (fp32 inputs: 260): the plant sits in the tail pass of the row loop."""
    f32_in = name in ("rmsnorm_f32", "layernorm_f32", "norm_split")
    D = 260 if f32_in else 520
    x = rnd(F32 if f32_in else dt, 9, D, seed=54)
    clean = _row_outputs(ops, name, dt, x)
    for k, o in clean.items():
        assert o.dtype == torch.uint8 or torch.isfinite(o.float()).all(), f"{name} {k}: the clean run is not finite"
    fails = Failures()
    for r in (0, 2, 8):
        for val in (float("nan"), float("inf")):
            xp = x.clone()
            xp[r, D - 3] = val
            got = _row_outputs(ops, name, dt, xp)
            for k, o in got.items():
                with fails.step(f"{name} {k}: {val} at x[{r}, {D - 3}]"):
                    keep = torch.arange(9, device="cuda") != r
                    assert same_bits(o[keep], clean[k][keep]), f"rows {sorted(set((o != clean[k]).nonzero()[:, 0].tolist()) - {r})} changed too"
                    if o.dtype == torch.uint8:
                        continue                                     # e4m3 codes: the row is reported through its scale
                    row = o[r].float()
                    if val != val:
                        assert bool(torch.isnan(row).all()), f"{int((~torch.isnan(row)).sum())} of {row.numel()} outputs of the row are not NaN"
                    elif name == "row_rstd":
                        assert row.item() == 0.0, f"rsqrt(mean(inf)) = 0 expected, got {row.item()}"
                    else:
                        assert bool((~torch.isfinite(row)).any()), "the row with +inf is all finite"
    fails.done()


# ------------------------------------------------------------------------------------------------------------ grid-stride wrap
def _past(cap, per_row):
    """→ a row count whose rows x per_row work items lie just past cap x 256 (one block's worth of threads takes a second trip) and
    are no multiple of 256"""
    rows = cap * 256 // per_row + 3
    assert rows * per_row > cap * 256 and (rows * per_row) % 256 != 0, (cap, per_row, rows)
    return rows


WRAP = ["sigmoid_f32_", "pack_rows", "check_finite", "gather_rows x16", "gather_rows f32", "scatter_rows_f32", "add_rows", "cast_f32_x16",
        "cast_x16_f32", "embed_tokens", "swiglu_split", "rope_half vector", "rope_half scalar", "rope_half_f32_", "mask_scatter", "pack_results",
        "resample_pass_u8"]


@pytest.mark.parametrize("name", WRAP)
def test_grid_stride_loops_wrap(ops, name):
    """One contiguous case per capped grid, against the torch statement on the device.  Each cap is the `if (blocks > cap)` of the named
    entry point (csrc/elementwise.hip unless stated)."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(11)
    randn = lambda *s: torch.randn(*s, device=dev, generator=g)
    if name == "sigmoid_f32_":                                       # padt_sigmoid_f32: 4096 blocks, one element per thread
        x = randn(4096 * 256 + 77)
        got = ops.sigmoid_f32_(x.clone())
        close_f32(got, torch.sigmoid(x), name)                       # as the parity test
    elif name == "pack_rows":                                        # padt_pack_rows: 4096 blocks, one 8-element chunk per thread
        K = 8200
        M = _past(4096, K // 8)
        M16 = (M + 15) // 16 * 16
        x = randn(M, K).to(BF)
        img = torch.zeros(M16, K, dtype=BF, device=dev)
        ops.pack_rows(x, img, M, to_packed=True)
        _bits_eq(img.view(M16 // 16, K // 8, 16, 8).permute(0, 2, 1, 3).reshape(M16, K)[:M], x, "packed")
        back = torch.zeros(M, K, dtype=BF, device=dev)
        ops.pack_rows(img, back, M, to_packed=False)
        _bits_eq(back, x, "unpacked")
    elif name == "check_finite":                                     # padt_check_finite: 8192 blocks, one 16-byte vector per thread
        cols = 4100
        rows = _past(8192, cols // 4)
        x = randn(rows, cols)
        flags = torch.zeros(rows, dtype=torch.int32, device=dev)
        assert int(ops.check_finite(x, flags, rows_per_flag=1).sum()) == 0
        x[rows - 1, cols - 1] = float("inf")
        x[0, 0] = float("nan")
        assert ops.check_finite(x, flags, rows_per_flag=1).nonzero().view(-1).tolist() == [0, rows - 1]
    elif name in ("gather_rows x16", "gather_rows f32"):             # padt_gather_rows / padt_gather_rows_f32: 16384 blocks, a chunk / an element per thread
        x16 = name.endswith("x16")
        D = 8200 if x16 else 1025
        n = _past(16384, D // 8 if x16 else D)
        src = randn(64, D).to(BF if x16 else F32)
        idx = torch.randint(0, 64, (n,), device=dev, generator=g).to(torch.int32)
        _bits_eq(ops.gather_rows(src, idx), src[idx.long()], name)
    elif name == "scatter_rows_f32":                                 # padt_scatter_rows_f32: 16384 blocks, 4 floats per thread
        D = 4100
        n = _past(16384, D // 4)
        src, dst = randn(n, D), torch.zeros(n + 5, D, device=dev)
        where = torch.randperm(n + 5, device=dev, generator=g)[:n].to(torch.int32)
        ref = dst.clone()
        ref[where.long()] = src
        _bits_eq(ops.scatter_rows_f32(src, where, dst), ref, name)
    elif name == "add_rows":                                         # padt_add_rows: 16384 blocks, a chunk per thread
        D = 8200
        n = _past(16384, D // 8)
        a, b = randn(n, D).to(BF), randn(7, D).to(BF)
        _bits_eq(ops.add_rows(a, b), (a.float() + b.float()[torch.arange(n, device=dev) % 7]).to(BF), name)
    elif name == "cast_f32_x16":                                     # padt_cast_f32_bf16: 32768 blocks, one element of D_pad per thread
        D, D_pad = 2042, 2050
        rows = _past(32768, D_pad)
        x = randn(rows, D)
        got = ops.cast_f32_x16(x, D_pad)
        _bits_eq(got[:, :D], x.to(BF), name)
        assert not got[:, D:].any()
    elif name == "cast_x16_f32":                                     # padt_cast_bf16_f32: 16384 blocks, a chunk per thread
        D = 8200
        x = randn(_past(16384, D // 8), D).to(F16)
        _bits_eq(ops.cast_x16_f32(x), x.float(), name)
    elif name == "embed_tokens":                                     # padt_embed_tokens: 16384 blocks, a chunk per thread
        V, NP, D = 40, 7, 8200
        T = _past(16384, D // 8)
        E, P = randn(V, D).to(BF), randn(NP, D).to(BF)
        ids = torch.randint(0, V + NP, (T,), device=dev, generator=g)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _bits_eq(ops.embed_tokens(ids, None, E, P, None, err_flag=err), torch.cat([E, P])[ids], name)
        assert int(err) == 0
    elif name == "swiglu_split":                                     # padt_swiglu_split (csrc/decoder_hp.hip): 32768 blocks, 4 columns per thread
        I = 8200
        rows = _past(32768, I // 4)
        gu = randn(rows, 2 * I)
        got = join(ops.swiglu_split(gu, I), I)
        for r0 in range(0, rows, 1024):                              # the fp64 statement in slices: the same bound, less memory
            s = slice(r0, r0 + 1024)
            split_close(got[s], silu(gu[s, :I].double()) * gu[s, I:].double(), f"{name} rows {r0}..")
    elif name in ("rope_half vector", "rope_half scalar", "rope_half_f32_"):
        # padt_rope_half: 32768 blocks (16-byte kernel, 8 pairs per thread) / 16384 blocks (scalar kernel, one pair per thread);
        # padt_rope_half_f32 (csrc/decoder_hp.hip): 32768 blocks, one pair per thread
        H, D = (16, 80) if name == "rope_half vector" else (4, 72)
        cap, per = {"rope_half vector": (32768, H * D // 16), "rope_half scalar": (16384, H * D // 2), "rope_half_f32_": (32768, H * D // 2)}[name]
        T = _past(cap, per)
        x = randn(T, H * D)
        x = x if name == "rope_half_f32_" else x.to(BF)
        ang = torch.rand(T, D // 2, device=dev, generator=g) * 50
        cos, sin = ang.cos(), ang.sin()
        y = x.clone()
        (ops.rope_half_f32_ if name == "rope_half_f32_" else ops.rope_half_)(y, cos, sin, H, D)
        step = 8192
        for r0 in range(0, T, step):
            s = slice(r0, r0 + step)
            if name == "rope_half_f32_":
                ref = _rope64(x[s], cos[s], sin[s], H, D)
                assert rel_err(y[s], ref) < 1e-6, f"{name} rows {r0}..: rel err {rel_err(y[s], ref):.2e}"
            else:
                close_bf16(y[s], rope_ref(x[s], cos[s], sin[s], H, D), f"{name} rows {r0}..")
    elif name == "mask_scatter":                                     # padt_mask_scatter: 16384 blocks, one logit (16 per patch) per thread
        dm, gh, gw = 8, 64, 64
        n_obj = 16384 * 256 // 16 // (gh * gw) + 1
        N = n_obj * gh * gw - 5                                      # the last object's grid is 5 patches short of its last row
        assert N * 16 > 16384 * 256 and (N * 16) % 256 != 0
        e2, tok = randn(4 * N, 4 * dm).to(BF), randn(n_obj, dm).to(BF)
        cu = torch.arange(n_obj + 1, dtype=torch.int32) * gh * gw
        cu[-1] = N
        masks = torch.full((n_obj, 4 * gh, 4 * gw), 7.0, device=dev)
        ops.mask_scatter(e2, tok, cu.cuda(), torch.full((n_obj,), gw, dtype=torch.int32, device=dev), masks, n_obj, N, dm)
        lg = (e2.float().view(N, 2, 2, 2, 2, dm) * tok.float()[torch.arange(N, device=dev) // (gh * gw)][:, None, None, None, None]).sum(-1)
        full = torch.full((n_obj * gh * gw, 2, 2, 2, 2), 7.0, device=dev)
        full[:N] = lg                                                # (patch, a, b, c, d) → plane[4 row + 2 a + c][4 col + 2 b + d]
        ref = full.view(n_obj, gh, gw, 2, 2, 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(n_obj, 4 * gh, 4 * gw)
        close_f32(masks, ref, name, rel=1e-5)                        # as test_mask_scatter
    elif name == "pack_results":                                     # padt_pack_results: 8192 blocks, one 32-bit word per thread
        from padt_amd import pipeline
        n, cap, mhw, H, Wd = 33, 33, 256, 250, 252
        assert 4 + 8 * cap + cap * mhw * mhw > 8192 * 256
        gc = torch.Generator().manual_seed(12)
        dec = {"pred_boxes": torch.rand(n, 4, generator=gc), "pred_score": torch.randn(n, 1, generator=gc), "pred_mask": torch.randn(n, H, Wd, generator=gc),
               "sample_idx": [i % 3 for i in range(n)], "pred_mask_valid_hw": (torch.full((n,), H - 4), torch.full((n,), Wd - 8))}
        ref = pipeline.pack_results(dec, cap, mhw, "cpu")
        devd = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in dec.items()}
        devd["pred_mask_valid_hw"] = tuple(t.cuda() for t in dec["pred_mask_valid_hw"])
        dirty = torch.full((ref.numel(),), 77, dtype=torch.int32, device=dev)
        assert torch.equal(pipeline.pack_results(devd, cap, mhw, dev, out=dirty).cpu(), ref)
    else:                                                            # padt_resample_pass_u8 (csrc/resize.hip): 16384 blocks, one output byte per thread
        import numpy as np
        from PIL import Image
        from padt_amd import preprocess as P
        H, W, ow = 1200, 900, 1171
        assert H * ow * 3 > 16384 * 256 and (H * ow * 3) % 256 != 0
        img = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((ow, H), resample=Image.BICUBIC))
        got = P.ImageFrontEnd("cuda", dtype=torch.float32).resize_device(torch.from_numpy(img).cuda(), ow, H, "bicubic").cpu().numpy()
        assert np.array_equal(got, ref), int((got != ref).sum())


def _rope64(x, cos, sin, H, D):
    T, half = x.shape[0], D // 2
    v = x.double().reshape(T, H, D)
    c, s = cos.double()[:, None, :half], sin.double()[:, None, :half]
    return torch.cat([v[..., :half] * c - v[..., half:] * s, v[..., half:] * c + v[..., :half] * s], -1).reshape(T, H * D)


# ------------------------------------------------------------------------------------------------------------ rejections
def test_misaligned_and_misshapen_operands_are_rejected_before_any_launch(ops):
    """Every entry point of csrc/elementwise.hip and csrc/decoder_hp.hip that moves 16-byte vectors returns -1 with its rule (PaDTHipError
    through ops) for a base pointer that is only 8-byte aligned (a view x[:, 4:] of a 16-bit tensor whose stride and D still satisfy the
    multiple-of-8 rules), for a D and for a stride that break its multiple; padt_rope_half and the two llm_qkv_post entries take their
    scalar path instead (tested above).  A rejected call launches nothing: every output still holds its fill."""
    from padt_amd._lib import PaDTHipError
    z16 = lambda r, c: torch.zeros(r, c, dtype=BF, device="cuda")
    z32 = lambda r, c: torch.zeros(r, c, device="cuda")
    x16, x32 = z16(8, 48), z32(8, 48)
    off16, off32 = x16[:, 4:36], x32[:, 2:34]                        # stride 48, 32 columns, base + 8 bytes
    assert off16.data_ptr() % 16 == 8 and off32.data_ptr() % 16 == 8
    w16, w_off = z16(1, 48)[0, :32], z16(1, 48)[0, 4:36]
    idx = torch.zeros(8, dtype=torch.int32, device="cuda")
    ids = torch.zeros(8, dtype=torch.int64, device="cuda")
    flags = torch.zeros(8, dtype=torch.int32, device="cuda")
    pos3, inv16 = torch.zeros(3, 8, dtype=torch.int32, device="cuda"), torch.ones(24, device="cuda")
    outs = []

    def o16(r=8, c=32, off=False, ld=48):
        t = torch.full((r, ld), 5.0, dtype=BF, device="cuda")
        outs.append(t)
        return t[:, 4:4 + c] if off else t[:, :c]

    def o32(r=8, c=32, off=False):
        t = torch.full((r, 48), 5.0, device="cuda")
        outs.append(t)
        return t[:, 2:2 + c] if off else t[:, :c]
    ok16, ok32 = x16[:, :32], x32[:, :32]
    odd16 = torch.zeros(8, 44, dtype=BF, device="cuda")[:, :32]      # stride 44: no multiple of 8
    odd32 = torch.zeros(8, 46, device="cuda")[:, :32]                # stride 46: no multiple of 4
    table = [
        ("rmsnorm x", lambda: ops.rmsnorm(off16, w16, out=o16()), "padt_rmsnorm"),
        ("rmsnorm add", lambda: ops.rmsnorm(ok16, w16, out=o16(), add=off16), "padt_rmsnorm"),
        ("rmsnorm w", lambda: ops.rmsnorm(ok16, w_off, out=o16()), "padt_rmsnorm"),
        ("rmsnorm y", lambda: ops.rmsnorm(ok16, w16, out=o16(off=True)), "padt_rmsnorm"),
        ("rmsnorm D", lambda: ops.rmsnorm(ok16, w16, out=o16(), D=28), "multiples of 8"),
        ("rmsnorm ldx", lambda: ops.rmsnorm(odd16, w16, out=o16()), "multiples of 8"),
        ("rmsnorm ldy", lambda: ops.rmsnorm(ok16, w16, out=o16(ld=44)), "multiples of 8"),
        ("rmsnorm ld_add", lambda: ops.rmsnorm(ok16, w16, out=o16(), add=odd16), "multiples of 8"),
        ("rmsnorm add_div", lambda: ops.rmsnorm(ok16, w16, out=o16(), add=ok16, add_div=0), "padt_rmsnorm"),
        ("layernorm x", lambda: ops.layernorm(off16, w16, w16, out=o16()), "padt_layernorm"),
        ("layernorm w", lambda: ops.layernorm(ok16, w_off, w16, out=o16()), "padt_layernorm"),
        ("layernorm b", lambda: ops.layernorm(ok16, w16, w_off, out=o16()), "padt_layernorm"),
        ("layernorm y", lambda: ops.layernorm(ok16, w16, w16, out=o16(off=True)), "padt_layernorm"),
        ("layernorm ldx", lambda: ops.layernorm(odd16, w16, w16, out=o16()), "multiples of 8"),
        ("layernorm ldy", lambda: ops.layernorm(ok16, w16, w16, out=o16(ld=44)), "multiples of 8"),
        ("layernorm D", lambda: ops.layernorm(x16[:, :28], w16, w16, out=o16(c=28)), "multiples of 8"),
        ("gather_rows src", lambda: ops.gather_rows(off16, idx, out=o16()), "padt_gather_rows"),
        ("gather_rows dst", lambda: ops.gather_rows(ok16, idx, out=o16(off=True)), "padt_gather_rows"),
        ("gather_rows D", lambda: ops.gather_rows(ok16, idx, out=o16(), D=28), "multiples of 8"),
        ("gather_rows ld_src", lambda: ops.gather_rows(odd16, idx, out=o16()), "multiples of 8"),
        ("gather_rows ld_dst", lambda: ops.gather_rows(ok16, idx, out=o16(ld=44)), "multiples of 8"),
        ("add_rows a", lambda: ops.add_rows(off16, ok16, out=o16()), "padt_add_rows"),
        ("add_rows b", lambda: ops.add_rows(ok16, off16, out=o16()), "padt_add_rows"),
        ("add_rows y", lambda: ops.add_rows(ok16, ok16, out=o16(off=True)), "padt_add_rows"),
        ("add_rows lda", lambda: ops.add_rows(odd16, ok16, out=o16()), "multiples of 8"),
        ("add_rows ldb", lambda: ops.add_rows(ok16, odd16, out=o16()), "multiples of 8"),
        ("add_rows ldy", lambda: ops.add_rows(ok16, ok16, out=o16(ld=44)), "multiples of 8"),
        ("add_rows D", lambda: ops.add_rows(x16[:, :28], x16[:, :28], out=o16(c=28)), "multiples of 8"),
        ("add_rows b_rows", lambda: ops.add_rows(ok16, ok16[:0], out=o16()), "b_rows >= 1"),
        ("embed_tokens table", lambda: ops.embed_tokens(ids, None, z16(9, 32).view(-1)[4:260].view(8, 32), None, None, out=o16(c=48).view(-1)[:256].view(8, 32)), "padt_embed_tokens"),
        ("embed_tokens proto", lambda: ops.embed_tokens(ids, None, z16(8, 32), z16(9, 32).view(-1)[4:260].view(8, 32), None, out=o16(c=48).view(-1)[:256].view(8, 32)), "padt_embed_tokens"),
        ("embed_tokens image_embeds", lambda: ops.embed_tokens(ids, idx, z16(8, 32), None, z16(9, 32).view(-1)[4:260].view(8, 32), out=o16(c=48).view(-1)[:256].view(8, 32)), "padt_embed_tokens"),
        ("embed_tokens out", lambda: ops.embed_tokens(ids, None, z16(8, 32), None, None, out=o16(c=48).view(-1)[4:260].view(8, 32)), "padt_embed_tokens"),
        ("embed_tokens D", lambda: ops.embed_tokens(ids, None, z16(8, 28), None, None, out=o16(c=48).view(-1)[:224].view(8, 28)), "multiple of 8"),
        ("row_rstd x", lambda: ops.row_rstd(off16, out=o32(1, 8)[0]), "padt_row_rstd"),
        ("pack_rows src", lambda: ops.pack_rows(z16(16, 48)[:, 4:36], o16(16), 16), "padt_pack_rows"),
        ("pack_rows dst", lambda: ops.pack_rows(z16(16, 48)[:, :32], o16(16, off=True), 16), "padt_pack_rows"),
        ("cast_x16_f32 x", lambda: ops.cast_x16_f32(off16, out=o32()), "padt_cast_bf16_f32"),
        ("cast_x16_f32 y", lambda: ops.cast_x16_f32(ok16, out=o32(off=True)), "padt_cast_bf16_f32"),
        ("rmsnorm_f32 x", lambda: ops.rmsnorm_f32(off32, w16, out=o16()), "padt_rmsnorm_f32"),
        ("rmsnorm_f32 ldx", lambda: ops.rmsnorm_f32(odd32, w16, out=o16()), "padt_rmsnorm_f32"),
        ("quant_rows_fp8 x", lambda: ops.quant_rows_fp8(off16), "padt_quant_rows_fp8"),
        ("check_finite x", lambda: ops.check_finite(off32, flags, rows_per_flag=1), "padt_check_finite"),
        ("check_finite cols", lambda: ops.check_finite(x32[:, :30], flags, rows_per_flag=1), "padt_check_finite"),
        ("scatter_rows_f32 src", lambda: ops.scatter_rows_f32(off32, idx[:1], o32()), "padt_scatter_rows_f32"),
        ("scatter_rows_f32 D", lambda: ops.scatter_rows_f32(ok32, idx[:1], o32(), D=30), "padt_scatter_rows_f32"),
        ("norm_split x", lambda: ops.norm_split(off32), "padt_norm_split"),
        ("norm_split ldx", lambda: ops.norm_split(odd32), "padt_norm_split"),
        ("swiglu_split gu", lambda: ops.swiglu_split(off32, 16, out=o16()), "padt_swiglu_split"),
        ("swiglu_split I", lambda: ops.swiglu_split(ok32, 15, out=o16()), "padt_swiglu_split"),
        ("layernorm_f32 x", lambda: ops.layernorm_f32(off32, w16, w16, out=o32()), "padt_layernorm_f32"),
        ("layernorm_f32 y", lambda: ops.layernorm_f32(ok32, w16, w16, out=o32(off=True)), "padt_layernorm_f32"),
        # the remaining width, chunk and head_dim rules, and the argument checks of the rotary / KV-cache entries
        ("quant_rows_fp8 K", lambda: ops.quant_rows_fp8(x16[:, :28]), "padt_quant_rows_fp8"),
        ("cast_x16_f32 D", lambda: ops.cast_x16_f32(x16[:, :28], out=o32(c=28)), "padt_cast_bf16_f32"),
        ("pack_rows K", lambda: ops.pack_rows(z16(16, 48)[:, :28], o16(16, c=28), 16), "padt_pack_rows"),
        ("norm_split chunk", lambda: ops.norm_split(ok32, chunk=12), "D % chunk == 0"),
        ("rope_half head_dim", lambda: ops.rope_half_(o16(), ok32, ok32, 1, 31), "head_dim must be even"),
        ("rope_half_f32 head_dim", lambda: ops.rope_half_f32_(o32(), ok32, ok32, 1, 31), "head_dim must be even"),
        ("llm_qkv_post without slot or lens", lambda: ops.llm_qkv_post(z16(8, 96), pos3, inv16, o16(), z16(8 * 32, 32), z16(8 * 32, 32), 1, 1, 32, 32,
                                                                      (4, 6, 6)), "need slot[] or lens[]"),
        ("llm_qkv_post packed caches", lambda: ops.llm_qkv_post(z16(8, 144), pos3, inv16, o16(c=48), z16(8 * 32, 48), z16(8 * 48, 32), 1, 1, 48, 32,
                                                               (8, 8, 8), lens=idx, cache_packed=True), "packed caches need head_dim % 32"),
    ]
    fails = Failures()
    for what, call, match in table:
        with fails.step(what):
            try:
                call()
            except PaDTHipError as e:
                assert match in str(e), f"message does not name the rule: {e}"
            else:
                raise AssertionError("accepted")
    torch.cuda.synchronize()
    with fails.step("a rejected call launches nothing"):
        assert int(flags.sum()) == 0
        for t in outs:
            assert bool((t == 5.0).all()), "an output of a rejected call was written"
    fails.done()
