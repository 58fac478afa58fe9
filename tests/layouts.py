"""Hostile memory layouts for the GPU tests: poisoned padding, guard bands around every buffer, bases off 16-byte alignment.

The poison is a NaN with a payload no arithmetic produces (0x7FF80000DEADBEEF / 0x7FC0BEEF), written through an integer view:
`torch.full(nan)` gives the default quiet NaN, which is also what inf - inf gives, so a kernel that stored a NaN of its own into a
guard would look like an untouched guard.  NaN payloads survive arithmetic, so a poisoned padding column that reaches a dot product
shows as a NaN in the result.  Every "unchanged" comparison is made on integer views: float equality is false on NaN.

A plain module (tests/test_layouts_host.py runs the same class on CPU tensors and plants the violations it is for)."""
import numpy as np

GUARD = 64                                             # elements on each side: 256 B / 512 B, multiples of 16
POISON64 = 0x7FF80000DEADBEEF
POISON32 = 0x7FC0BEEF


def _torch():
    import torch
    return torch


def int_dtype(dtype):
    """the integer type of the same width: the type every bit comparison is made in"""
    torch = _torch()
    return {torch.float64: torch.int64, torch.float32: torch.int32, torch.int64: torch.int64}[dtype]


def poison_bits(dtype):
    """the fill of guards and padding as an integer: the poison NaN for the real types, the valid index 0 for int64 index lists
    (an out-of-range sentinel could send a prefetch to a wild address)"""
    torch = _torch()
    return {torch.float64: POISON64, torch.float32: POISON32, torch.int64: 0}[dtype]


def bits(t):
    """integer view of a contiguous tensor"""
    return t.view(int_dtype(t.dtype))


def poisoned(shape, dtype, device):
    """a new contiguous tensor of `shape`, every element the poison"""
    torch = _torch()
    t = torch.empty(shape, dtype=dtype, device=device)
    bits(t).fill_(poison_bits(dtype))
    return t


def as_torch_dtype(dtype):
    torch = _torch()
    if isinstance(dtype, torch.dtype):
        return dtype
    return {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64}[np.dtype(dtype)]


class Guarded:
    """A 1-D or 2-D tensor placed inside a poisoned flat buffer of its dtype: `guard` elements on each side, the base `off` elements
    further in (off = 1: sizeof(T) off 16-byte alignment), rows at stride ld >= d with the columns [d, ld) poisoned.

        .view               what is handed to the library
        .check_outside()    every element outside the view still has the poison bits
        .check_unchanged()  the whole buffer has the bits it had after construction (inputs)

    `t` None with `shape` and `dtype`: an output, the view poisoned too (what the call leaves unwritten stays visible)."""

    def __init__(self, t=None, off=0, ld=None, guard=GUARD, device=None, shape=None, dtype=None, name=""):
        torch = _torch()
        if t is not None:
            if isinstance(t, np.ndarray):
                t = torch.from_numpy(np.ascontiguousarray(t))
            shape, dtype = tuple(t.shape), t.dtype
            device = t.device if device is None else device
        else:
            shape, dtype = tuple(int(s) for s in shape), as_torch_dtype(dtype)
        assert len(shape) in (1, 2) and off >= 0 and guard >= 0
        self.name, self.off, self.guard, self.shape = name, int(off), int(guard), shape
        if len(shape) == 1:
            n, d, self.ld = 1, shape[0], shape[0]
            assert ld is None or ld == shape[0]
        else:
            n, d = shape
            self.ld = d if ld is None else int(ld)
            assert self.ld >= d
        self.start = self.guard + self.off
        span = n * self.ld                             # (the last row's padding columns belong to the buffer)
        self.flat = poisoned((self.start + span + self.guard,), dtype, device)
        body = self.flat[self.start:self.start + span]
        if len(shape) == 1:
            self.view = body
        else:
            self.view = body.view(n, self.ld)[:, :d]
        self.inside = torch.zeros(self.flat.numel(), dtype=torch.bool, device=device)
        if len(shape) == 1:
            self.inside[self.start:self.start + span] = True
        else:
            self.inside[self.start:self.start + span].view(n, self.ld)[:, :d] = True
        if t is not None:
            self.view.copy_(t)
        self.snapshot()

    def snapshot(self):
        """take the buffer as it is now for what check_unchanged() compares with"""
        self._orig = bits(self.flat).clone()
        return self

    @property
    def is_index(self):
        return self.flat.dtype == _torch().int64

    def outside_touched(self):
        """flat positions outside the view whose bits are not the fill any more"""
        torch = _torch()
        bad = (bits(self.flat) != poison_bits(self.flat.dtype)) & ~self.inside
        return torch.nonzero(bad).flatten().tolist()

    def check_outside(self, what=""):
        if self.is_index:                              # guards of valid indices: nothing to tell a store by
            return
        bad = self.outside_touched()
        assert not bad, (f"{what}: {self.name or 'buffer'}: {len(bad)} element(s) outside the view were written; the first at "
                         f"{self.describe(bad[0])}")

    def check_unchanged(self, what=""):
        torch = _torch()
        now = bits(self.flat)
        if torch.equal(now, self._orig):
            return
        bad = torch.nonzero(now != self._orig).flatten().tolist()
        raise AssertionError(f"{what}: {self.name or 'buffer'}: {len(bad)} element(s) of an input changed; the first at {self.describe(bad[0])}")

    def describe(self, pos):
        """a flat position in words: guard before / after, or (row, column) with padding columns named"""
        rel = pos - self.start
        if rel < 0:
            return f"{-rel} element(s) before the view"
        n = 1 if len(self.shape) == 1 else self.shape[0]
        if rel >= n * self.ld:
            return f"{rel - n * self.ld + 1} element(s) after the buffer's last row"
        i, j = divmod(rel, self.ld)
        d = self.shape[-1]
        return f"row {i} column {j}" + (f" (padding: d = {d}, ld = {self.ld})" if j >= d else "")


def has_poison(t):
    """a NaN anywhere in an output (the poison, or what arithmetic made of it)"""
    torch = _torch()
    if not hasattr(t, "detach"):
        return bool(np.isnan(np.asarray(t, dtype=np.float64)).any())
    return bool(torch.isnan(t).any())
