"""Strided windows in poisoned buffers: the operands of the "edges" GPU tests (tests/test_gemm_edges_gpu.py, test_row_edges_gpu.py,
test_mask_edges_gpu.py), the Arena that hands them out for one launch, and three(), the three assertions every window case makes.

A kernel is handed a row-strided VIEW of a larger allocation (the backing).  Everything of the backing outside the view holds one fill
value: NaN around an input (a read outside the operand's logical extent poisons an accumulator: 0 x NaN = NaN), a finite sentinel around
an output (a write outside the window changes its bits).  Plain torch, usable on the CPU; no GPU is needed to import this module.

Margins are a safety rule: window() refuses a backing with less than MIN_ROWS rows above and below the view and MIN_COLS elements to its
left and right — one full tile of the largest kernel — so that a kernel that overruns an operand by a whole tile still stays inside the
allocation and produces a failing assertion instead of a fault.  The one exception is a SLAB (c0 = cols_after = 0: rows at their natural
stride, for images whose row stride is fixed by their layout): there the MIN_ROWS whole rows on either side are the margin in both
directions.
"""
import contextlib

import torch

MIN_ROWS, MIN_COLS = 256, 128
SENTINEL = -1234.0                      # finite in bf16 (as -1232), fp16 and fp32, compared by its bits; no kernel of the tests produces it
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def nan_fill(dtype):
    """The poison of an input of type dtype: NaN, or for e4m3 bytes kept in uint8 the NaN code 0x7F."""
    return 0x7F if dtype == torch.uint8 else float("nan")


def _bits(t):
    return t.contiguous().view(_INT_OF[t.element_size()])


def same_bits(a, b):
    """Bitwise equality of two tensors of one type and shape (NaN == NaN of the same payload, +0 != -0)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return torch.equal(_bits(a), _bits(b))


def window(t, r0, c0, rows_after, cols_after, fill):
    """→ (backing, view): `backing` is a fresh tensor of t's type and device filled with `fill`, `view` a view of it that holds t.
    2-D t (rows, cols): backing (r0 + rows + rows_after, c0 + cols + cols_after), view = backing[r0:r0 + rows, c0:c0 + cols] (row stride =
    the backing's width).  1-D t (n,): backing (c0 + n + cols_after,), view = backing[c0:c0 + n]; r0 and rows_after must be 0."""
    if t.dim() == 1:
        assert r0 == 0 and rows_after == 0 and c0 >= MIN_COLS and cols_after >= MIN_COLS, (r0, c0, rows_after, cols_after)
        backing = torch.full((c0 + t.numel() + cols_after,), fill, dtype=t.dtype, device=t.device)
        view = backing[c0:c0 + t.numel()]
    else:
        assert t.dim() == 2 and r0 >= MIN_ROWS and rows_after >= MIN_ROWS, (t.shape, r0, rows_after)
        assert (c0 >= MIN_COLS and cols_after >= MIN_COLS) or (c0 == 0 and cols_after == 0), (c0, cols_after)
        rows, cols = t.shape
        backing = torch.full((r0 + rows + rows_after, c0 + cols + cols_after), fill, dtype=t.dtype, device=t.device)
        view = backing[r0:r0 + rows, c0:c0 + cols]
    view.copy_(t)
    return backing, view


def _inside(backing, view_spec):
    """bool mask of the backing's elements that belong to a window.  view_spec: one window or a list of windows (a split output has two);
    a window is (r0, c0, rows, cols) in a 2-D backing and (c0, n) in a 1-D one."""
    specs = [view_spec] if isinstance(view_spec[0], int) else list(view_spec)
    inside = torch.zeros(backing.shape, dtype=torch.bool, device=backing.device)
    for s in specs:
        if backing.dim() == 1:
            c0, n = s
            assert 0 < c0 and c0 + n < backing.numel(), ("window touches the ends of its allocation", s, backing.shape)
            inside[c0:c0 + n] = True
        else:
            r0, c0, rows, cols = s
            assert 0 < r0 and r0 + rows < backing.shape[0] and 0 <= c0 and c0 + cols <= backing.shape[1], (s, backing.shape)
            inside[r0:r0 + rows, c0:c0 + cols] = True
    return inside


def outside_unchanged(backing, view_spec, fill):
    """Assert, bitwise, that every element of `backing` outside the window(s) of view_spec still holds `fill`."""
    want = _bits(torch.full((1,), fill, dtype=backing.dtype, device=backing.device))
    bad = (_bits(backing).view(backing.shape) != want) & ~_inside(backing, view_spec)
    if bool(bad.any()):
        where = bad.nonzero()[:4].tolist()
        raise AssertionError(f"{int(bad.sum())} elements outside the window changed, first at {where} of a {tuple(backing.shape)} backing "
                             f"(window {view_spec})")


BYTE_SENTINEL = 0xA5                    # around a uint8 output: neither a mask byte (0 / 1) nor the e4m3 NaN code


def sentinel_of(dtype):
    """What surrounds an output window of type dtype: SENTINEL for the float types, the same number as an integer for int32 / int64, the
    byte 0xA5 for uint8."""
    if dtype == torch.uint8:
        return BYTE_SENTINEL
    return SENTINEL if dtype.is_floating_point else int(SENTINEL)


class Arena:
    """The windows of one launch.  poison: NaN (else zeros) around the inputs; the sentinel around the outputs either way.  Every 2-D window
    gets a row stride of its own (a multiple of 16 elements, which satisfies every entry point's stride rule)."""

    def __init__(self, poison):
        self.poison, self.outs, self.lds = poison, [], set()

    def _ld(self, cols, ld, c0=MIN_COLS):
        if ld is None:
            ld = (c0 + cols + MIN_COLS + 15) // 16 * 16
            while ld in self.lds:
                ld += 16
        self.lds.add(ld)
        return ld

    def _win(self, t, ld, slab, fill, c0=MIN_COLS):
        """c0: the column of the backing at which a 1-D / 2-D window starts (>= MIN_COLS; MIN_COLS + 4 makes a 16-bit window 8-byte aligned);
        ld: the row stride (any value that leaves MIN_COLS elements behind the window; default: a multiple of 16 no other window has)."""
        if t.dim() == 1:
            return window(t, 0, c0, 0, MIN_COLS + 8, fill) + ((c0, t.numel()),)
        if slab:                                                     # rows at their natural stride (fragment-packed images and buffers)
            return window(t, MIN_ROWS, 0, MIN_ROWS, 0, fill) + ((MIN_ROWS, 0) + tuple(t.shape),)
        ld = self._ld(t.shape[1], ld, c0)
        return window(t, MIN_ROWS, c0, MIN_ROWS + 8, ld - c0 - t.shape[1], fill) + ((MIN_ROWS, c0) + tuple(t.shape),)

    def inp(self, t, ld=None, slab=False, c0=MIN_COLS):
        return self._win(t, ld, slab, nan_fill(t.dtype) if self.poison else 0, c0)[1]

    def out(self, t, ld=None, slab=False, spec=None, c0=MIN_COLS):
        """t: the window's initial contents; spec: the windows inside it that may be written (default: all of it), relative to its corner."""
        fill = sentinel_of(t.dtype)
        backing, view, whole = self._win(t, ld, slab, fill, c0)
        if spec is not None:
            whole = [(whole[0] + r, whole[1] + c, rows, cols) for r, c, rows, cols in spec]
        self.outs.append((backing, whole, fill))
        return view

    def check(self):
        for backing, spec, fill in self.outs:
            outside_unchanged(backing, spec, fill)


class Failures:
    """Collects the failed assertions of a test that loops over epilogues / variants, so that one run shows all of them."""

    def __init__(self):
        self.msgs = []

    @contextlib.contextmanager
    def step(self, what):
        try:
            yield
        except AssertionError as e:
            self.msgs.append(f"[{what}] {str(e)[:600]}")

    def done(self):
        assert not self.msgs, f"{len(self.msgs)} failed:\n" + "\n".join(self.msgs)


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize()


def three(fails, what, body, check):
    """The three assertions of an operand-window case.  body(arena) → {name: result view}; check(results) compares with the reference."""
    got = {}
    for poison in (True, False):
        ar = Arena(poison)
        outs = body(ar)
        for v in outs.values():
            _sync(v)
        got[poison] = {k: v.clone() for k, v in outs.items()}
        with fails.step(f"{what}: 3 (outside the output windows, {'NaN' if poison else 'zero'} run)"):
            ar.check()
    with fails.step(f"{what}: 1 (reference)"):
        check(got[True])
    for k, v in got[True].items():
        with fails.step(f"{what}: 2 (bit-identical to the run with zeros around the operands)"):
            assert same_bits(v, got[False][k]), f"{k}: {int((v != got[False][k]).sum())} of {v.numel()} elements differ, " \
                                                f"{int((~torch.isfinite(v.float())).sum())} non-finite"


def outside_is_nan(backing, view_spec):
    """True when every element outside the window(s) is NaN (uint8 e4m3 backings: the byte 0x7F)."""
    out = ~_inside(backing, view_spec)
    if backing.dtype == torch.uint8:
        return bool((backing[out] == 0x7F).all())
    return bool(torch.isnan(backing[out]).all())
