"""tests/layouts.py on CPU tensors: the harness notices what it is for.  One violation is planted at a time -- a write one element before
the view, one after it, one into a padding column of a middle row, a default-NaN overwrite of a guard element, a changed input element --
and exactly the matching check fires; none fires on the clean layout.  (CPU test.)"""
import numpy as np
import pytest
import torch

import layouts as L

DTYPES = [torch.float64, torch.float32]
CASES = [((7,), None), ((5, 6), None), ((5, 6), 9), ((1, 6), 8)]      # (shape, ld)


def _source(shape, dtype):
    n = int(np.prod(shape))
    return (torch.arange(n, dtype=torch.float64).reshape(shape) * 0.37 - 1.0).to(dtype)


def _fires(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_poison_is_not_the_nan_arithmetic_makes(dtype):
    p = L.poisoned((4,), dtype, "cpu")
    assert bool(torch.isnan(p).all())
    default = torch.full((4,), float("nan"), dtype=dtype)
    made = torch.full((4,), float("inf"), dtype=dtype) - torch.full((4,), float("inf"), dtype=dtype)
    assert not bool((L.bits(p) == L.bits(default)).any()) and not bool((L.bits(p) == L.bits(made)).any())
    # the payload survives arithmetic: what a dot product makes of a poisoned element is still a NaN
    assert bool(torch.isnan(p * 2 + 1).all()) and bool(torch.isnan((p * torch.ones(4, dtype=dtype)).sum()))
    assert not bool(torch.equal(p, p))                    # why every comparison here is on integer views
    assert torch.equal(L.bits(p), L.bits(p.clone()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("shape,ld", CASES)
def test_placement(dtype, off, shape, ld):
    src = _source(shape, dtype)
    g = L.Guarded(src, off=off, ld=ld, device="cpu")
    es = src.element_size()
    assert g.flat.data_ptr() % 16 == 0
    assert g.view.data_ptr() % 16 == (off * es) % 16
    assert g.view.data_ptr() == g.flat.data_ptr() + (L.GUARD + off) * es
    assert tuple(g.view.shape) == tuple(shape) and torch.equal(g.view, src)
    if len(shape) == 2:
        assert g.view.stride(1) == 1 and (shape[0] == 1 or g.view.stride(0) == (ld or shape[1]))
        if ld is None:
            assert g.view.is_contiguous()
    # guards, the `off` elements and the padding columns are poison; the count of poisoned elements is the buffer less the view
    assert int((L.bits(g.flat) == L.poison_bits(dtype)).sum()) == g.flat.numel() - src.numel()
    assert int(g.inside.sum()) == src.numel()
    g.check_outside()
    g.check_unchanged()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("off", [0, 1])
def test_each_planted_violation_trips_exactly_its_check(dtype, off):
    src = _source((5, 6), dtype)

    def fresh():
        return L.Guarded(src, off=off, ld=9, device="cpu", name="A")
    g = fresh()
    assert not _fires(g.check_outside) and not _fires(g.check_unchanged)
    first, n, ld, d = g.start, 5, 9, 6
    plants = {
        "one element before the view": first - 1,
        "one element after the view": first + (n - 1) * ld + d,            # the last row's first padding column
        "one element after the buffer's rows": first + n * ld,
        "a padding column of a middle row": first + 2 * ld + d + 1,
    }
    for what, pos in plants.items():
        g = fresh()
        g.flat[pos] = 1.5
        assert _fires(g.check_outside), what
        assert g.outside_touched() == [pos], what
        g.flat[pos] = 0.0                                  # a stored zero is a store too (a zero-filled pad would hide it)
        assert _fires(g.check_outside), what
    # a kernel that stores its OWN NaN into a guard: an isnan test of the guard would pass, the bit comparison does not
    g = fresh()
    g.flat[first - 3] = float("nan")
    assert bool(torch.isnan(g.flat[:first]).all())
    assert _fires(g.check_outside) and g.outside_touched() == [first - 3]
    # ... and what arithmetic makes of two infinities
    g = fresh()
    g.flat[first - 3] = float("inf")
    g.flat[first - 3] -= float("inf")
    assert _fires(g.check_outside)
    # a changed input element: only check_unchanged
    g = fresh()
    g.view[3, 2] += 1
    assert not _fires(g.check_outside) and _fires(g.check_unchanged)
    # (check_unchanged is over the whole buffer: a write outside the view trips it as well)
    g = fresh()
    g.flat[first - 1] = 1.5
    assert _fires(g.check_unchanged)
    # a write into the view is what an output is for: not check_outside's business
    o = L.Guarded(shape=(5, 6), dtype=dtype, device="cpu", off=off)
    assert bool(torch.isnan(o.view).all()) and L.has_poison(o.view)
    o.view.copy_(src)
    assert not _fires(o.check_outside) and not L.has_poison(o.view) and _fires(o.check_unchanged)
    o.snapshot()
    assert not _fires(o.check_unchanged)


def test_vectors_and_index_lists():
    g = L.Guarded(_source((7,), torch.float32), off=1, device="cpu")
    g.flat[g.start + 7] = 2.0
    assert _fires(g.check_outside)
    idx = L.Guarded(np.arange(9, dtype=np.int64)[::-1].copy(), device="cpu")
    assert idx.is_index and int(idx.flat[:L.GUARD].abs().sum()) == 0 and int(idx.flat[-L.GUARD:].abs().sum()) == 0
    assert torch.equal(idx.view, torch.arange(8, -1, -1))
    idx.check_outside()
    idx.check_unchanged()
    idx.flat[0] = 5                                         # guards of valid indices: only check_unchanged can tell
    assert not _fires(idx.check_outside) and _fires(idx.check_unchanged)
    idx = L.Guarded(np.arange(9, dtype=np.int64), device="cpu")
    idx.view[4] = 0
    assert _fires(idx.check_unchanged)


def test_messages_say_where():
    g = L.Guarded(_source((5, 6), torch.float64), ld=9, device="cpu", name="table")
    assert g.describe(g.start - 2) == "2 element(s) before the view"
    assert g.describe(g.start + 2 * 9 + 7) == "row 2 column 7 (padding: d = 6, ld = 9)"
    assert g.describe(g.start + 5 * 9) == "1 element(s) after the buffer's last row"
    g.flat[g.start + 9 + 6] = 0.0
    with pytest.raises(AssertionError, match=r"table: 1 element\(s\) outside the view were written; the first at row 1 column 6"):
        g.check_outside("saga_init")
