"""tests/edge_util.py on the CPU: the windows hold their tensors, the poison is where it should be, and outside_unchanged sees one planted
element below, to the right of, and (split output) in the gap between the windows — the checks of tests/test_gemm_edges_gpu.py are only as
good as these."""
import pytest
import torch

from edge_util import MIN_COLS, MIN_ROWS, SENTINEL, nan_fill, outside_is_nan, outside_unchanged, same_bits, window

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
