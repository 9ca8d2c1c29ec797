"""tests/edge_util.py on the CPU: the windows hold their tensors, the poison is where it should be, and outside_unchanged sees one planted
element below, to the right of, and (split output) in the gap between the windows — the checks of tests/test_gemm_edges_gpu.py are only as
good as these.  Arena / Failures / three (shared by the GEMM, row and mask edge suites) run here on CPU tensors: a body that
over-reads by one element, writes one element outside its window, or depends on the poison is caught by the assertion meant for it."""
import pytest
import torch

from edge_util import (BYTE_SENTINEL, MIN_COLS, MIN_ROWS, SENTINEL, Arena, Failures, nan_fill, outside_is_nan, outside_unchanged, same_bits,
                       sentinel_of, three, window)

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.uint8]


def _t(dtype, *shape):
    g = torch.Generator().manual_seed(7)
    if dtype == torch.uint8:
        return torch.randint(0, 0x7F, shape, generator=g, dtype=torch.uint8)
    return torch.randn(*shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_view_holds_the_tensor_at_the_requested_stride(dtype):
    t = _t(dtype, 37, 24)
    backing, view = window(t, 256, 128, 300, 136, nan_fill(dtype))
    assert torch.equal(view, t) and view.shape == t.shape
    assert view.stride() == (128 + 24 + 136, 1) and backing.shape == (256 + 37 + 300, 288)
    assert view.data_ptr() == backing.data_ptr() + (256 * 288 + 128) * t.element_size()
    v = _t(dtype, 19)
    b1, v1 = window(v, 0, 128, 0, 160, nan_fill(dtype))
    assert torch.equal(v1, v) and b1.shape == (128 + 19 + 160,) and v1.data_ptr() == b1.data_ptr() + 128 * v.element_size()
    sb, sv = window(t, 256, 0, 256, 0, nan_fill(dtype))              # a slab: rows at their natural stride
    assert torch.equal(sv, t) and sv.stride() == (24, 1) and sb.shape == (256 + 37 + 256, 24)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_nan_backing_is_nan_everywhere_outside_the_window(dtype):
    t = _t(dtype, 5, 16)
    backing, view = window(t, 256, 128, 256, 128, nan_fill(dtype))
    spec = (256, 128, 5, 16)
    assert outside_is_nan(backing, spec)
    if dtype != torch.uint8:
        assert int(torch.isnan(backing).sum()) == backing.numel() - t.numel() and torch.isfinite(view.float()).all()
    backing[300, 3] = 0
    assert not outside_is_nan(backing, spec)
    b1, _ = window(_t(dtype, 9), 0, 128, 0, 128, nan_fill(dtype))
    assert outside_is_nan(b1, (128, 9))
    b1[-1] = 0
    assert not outside_is_nan(b1, (128, 9))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=str)
def test_outside_unchanged_sees_one_planted_element(dtype):
    rows, cols = 21, 12
    spec = (256, 128, rows, cols)

    def fresh():
        return window(_t(dtype, rows, cols), 256, 128, 256, 128, SENTINEL)
    backing, view = fresh()
    outside_unchanged(backing, spec, SENTINEL)
    view.fill_(3.0)                                                  # writes inside the window are not its business
    outside_unchanged(backing, spec, SENTINEL)
    for r, c in [(256 + rows, 128), (256 + rows, 128 + cols - 1),    # one row below the window
                 (256, 128 + cols), (256 + rows - 1, 128 + cols),    # one column to the right of it
                 (255, 128), (256, 127), (0, 0), (backing.shape[0] - 1, backing.shape[1] - 1)]:
        backing, _ = fresh()
        backing[r, c] = 1.0
        with pytest.raises(AssertionError, match="outside the window changed"):
            outside_unchanged(backing, spec, SENTINEL)
    # same value, other bits: -0.0 where the sentinel would be 0.0
    z, _ = window(_t(dtype, rows, cols), 256, 128, 256, 128, 0.0)
    outside_unchanged(z, spec, 0.0)
    z[256 + rows, 130] = -0.0
    with pytest.raises(AssertionError):
        outside_unchanged(z, spec, 0.0)


def test_outside_unchanged_guards_the_gap_of_a_split_output():
    """(hi | lo) rows with lo_off > N: the columns [N, lo_off) between the two halves are outside."""
    M, N, lo_off = 9, 8, 12
    split = [(256, 128, M, N), (256, 128 + lo_off, M, N)]
    backing, view = window(torch.zeros(M, lo_off + N), 256, 128, 256, 128, SENTINEL)
    with pytest.raises(AssertionError):                              # window() filled the gap with the tensor's zeros
        outside_unchanged(backing, split, SENTINEL)
    view[:, N:lo_off] = SENTINEL
    outside_unchanged(backing, split, SENTINEL)
    view[:, :N] = 1.0
    view[:, lo_off:] = 2.0
    outside_unchanged(backing, split, SENTINEL)
    for c in (N, lo_off - 1):
        view[4, c] = 5.0
        with pytest.raises(AssertionError, match="outside the window changed"):
            outside_unchanged(backing, split, SENTINEL)
        view[4, c] = SENTINEL
    outside_unchanged(backing, split, SENTINEL)


def test_vectors_and_margins():
    b, v = window(torch.arange(10.0), 0, 128, 0, 128, SENTINEL)
    outside_unchanged(b, (128, 10), SENTINEL)
    for i in (127, 138):
        b2 = b.clone()
        b2[i] = 0.0
        with pytest.raises(AssertionError):
            outside_unchanged(b2, (128, 10), SENTINEL)
    t = torch.zeros(4, 8)
    for bad in [(MIN_ROWS - 1, 128, 256, 128), (256, MIN_COLS - 1, 256, 128), (256, 128, MIN_ROWS - 1, 128), (256, 128, 256, MIN_COLS - 1),
                (256, 0, 256, 128)]:
        with pytest.raises(AssertionError):                          # a margin below one tile of the largest kernel is refused
            window(t, *bad, SENTINEL)
    with pytest.raises(AssertionError):
        window(torch.zeros(5), 0, 64, 0, 128, SENTINEL)


def test_same_bits():
    a = torch.tensor([1.0, float("nan"), 0.0])
    assert same_bits(a, a.clone()) and not same_bits(a, torch.tensor([1.0, float("nan"), -0.0]))
    assert same_bits(a.to(torch.bfloat16), a.to(torch.bfloat16)) and not same_bits(a.half(), torch.tensor([1.0, 2.0, 0.0]).half())
    a2 = torch.randn(6, 10)[:, 2:7]                                  # strided views compare by value
    assert same_bits(a2, a2.clone())


# ------------------------------------------------------------------------------------------------------------ Arena / Failures / three
def test_sentinels_per_type():
    assert sentinel_of(torch.uint8) == BYTE_SENTINEL == 0xA5 and nan_fill(torch.uint8) == 0x7F
    assert sentinel_of(torch.int32) == -1234 and isinstance(sentinel_of(torch.int32), int)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert sentinel_of(dt) == SENTINEL and torch.isfinite(torch.tensor(SENTINEL, dtype=dt))          # bf16 rounds it to -1232: bits are compared


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.float32, torch.bfloat16], ids=str)
def test_arena_output_windows_carry_their_types_sentinel(dtype):
    ar = Arena(True)
    t = torch.ones(5, 24).to(dtype)
    v = ar.out(t)
    backing, spec, fill = ar.outs[0]
    assert fill == sentinel_of(dtype) and backing.dtype == dtype and torch.equal(v, t)
    assert int((backing == fill).sum()) == backing.numel() - t.numel()
    ar.check()
    v.fill_(7)                                                       # inside: free
    ar.check()
    backing[MIN_ROWS + 5, MIN_COLS] = 7                              # the row below
    with pytest.raises(AssertionError, match="outside the window changed"):
        ar.check()
    backing[MIN_ROWS + 5, MIN_COLS] = fill
    backing[MIN_ROWS + 4, MIN_COLS + 24] = 7                         # one element to the right
    with pytest.raises(AssertionError, match="outside the window changed"):
        ar.check()
    ar1 = Arena(False)
    v1 = ar1.out(torch.zeros(9).to(dtype))
    ar1.check()
    ar1.outs[0][0][MIN_COLS + 9] = 1
    with pytest.raises(AssertionError):
        ar1.check()
    assert v1.numel() == 9


def test_arena_windows_strides_offsets_and_poison():
    ar = Arena(True)
    a, b, c = ar.inp(torch.ones(5, 24)), ar.inp(torch.ones(7, 24)), ar.out(torch.ones(5, 24))
    assert len({a.stride(0), b.stride(0), c.stride(0)}) == 3 and all(s % 16 == 0 for s in (a.stride(0), b.stride(0), c.stride(0)))
    assert a.storage_offset() == MIN_ROWS * a.stride(0) + MIN_COLS
    base = a.as_strided((MIN_ROWS + 5 + MIN_ROWS + 8, a.stride(0)), (a.stride(0), 1), 0)               # the whole backing
    assert int(torch.isnan(base).sum()) == base.numel() - 5 * 24
    z = Arena(False).inp(torch.ones(5, 24))
    assert float(z.as_strided((1,), (1,), 0)) == 0.0                 # zeros around the inputs of the second run
    u = ar.inp(torch.ones(4, 16, dtype=torch.uint8))
    assert int(u.as_strided((1,), (1,), 0)) == 0x7F
    # a window 4 elements in (8 bytes for a 16-bit type) and a row stride that is no multiple of 8
    w = ar.inp(torch.ones(3, 80, dtype=torch.bfloat16), c0=MIN_COLS + 4)
    assert w.storage_offset() % 8 == 4 and (w.data_ptr() - w.storage_offset() * 2) % 16 == 0 and w.data_ptr() % 16 == 8
    o = ar.out(torch.ones(3, 80, dtype=torch.bfloat16), ld=MIN_COLS + 80 + MIN_COLS + 4)
    assert o.stride(0) % 8 == 4
    ar.check()
    with pytest.raises(AssertionError):                              # a stride that leaves less than the margin behind the window
        ar.inp(torch.ones(3, 80), ld=MIN_COLS + 80 + MIN_COLS - 1)
    s = ar.out(torch.ones(32, 40), slab=True)                        # a slab: natural stride, whole sentinel rows around it
    assert s.stride(0) == 40 and ar.outs[-1][1] == (MIN_ROWS, 0, 32, 40)
    sp = ar.out(torch.full((4, 20), SENTINEL), spec=[(0, 0, 4, 8), (0, 12, 4, 8)])
    sp[:, :8] = 1.0
    ar.check()
    sp[2, 9] = 1.0                                                   # the gap of a split window is outside
    with pytest.raises(AssertionError):
        ar.check()


def test_three_catches_an_over_read_a_stray_store_and_a_wrong_result():
    x = torch.arange(12.0).view(3, 4)

    def run(body, check=lambda got: None):
        f = Failures()
        three(f, "case", body, check)
        return f.msgs

    def good(ar):
        X, Y = ar.inp(x), ar.out(torch.zeros(3, 4))
        Y.copy_(X * 2)
        return {"y": Y}
    assert run(good, lambda got: torch.testing.assert_close(got["y"], x * 2)) == []

    def over_read(ar):                                               # one element past the row end enters the sum
        X, Y = ar.inp(x), ar.out(torch.zeros(3, 1))
        wide = X.as_strided((3, 5), (X.stride(0), 1), X.storage_offset())
        Y.copy_(wide.sum(1, keepdim=True))
        return {"y": Y}
    msgs = run(over_read)
    assert len(msgs) == 1 and "case: 2" in msgs[0]                   # NaN run != zero run

    def stray_store(ar):
        X, Y = ar.inp(x), ar.out(torch.zeros(3, 4))
        Y.copy_(X)
        Y.as_strided((1,), (1,), Y.storage_offset() + 4).fill_(1.0)  # one element right of row 0
        return {"y": Y}
    msgs = run(stray_store)
    assert len(msgs) == 2 and all("case: 3" in m for m in msgs)      # both runs

    msgs = run(good, lambda got: torch.testing.assert_close(got["y"], x * 3))
    assert len(msgs) == 1 and "case: 1" in msgs[0]
    f = Failures()
    with f.step("a"):
        assert False, "boom"
    with pytest.raises(AssertionError, match=r"1 failed:\n\[a\] boom"):
        f.done()
