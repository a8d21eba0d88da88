"""Caller-built buffer layouts for the layout tests (no GPU, no torch).

include/mvmatch.h leaves every offset table but ``ext_offs`` to the caller:
entry ``s`` is read on its own, so regions may lie in any order, with gaps
between them and at any residue the buffer's required multiple allows.  The
plans (``PairwisePlan`` / ``TripletPlan`` / ``LsapPlan``) produce one such
layout only.  ``layout`` turns a list of region sizes into the offsets of one
of these families:

``tight``      regions back to back in order (offsets rounded up to ``unit``):
               the plan's layout
``gaps``       a gap of 1-37 units in front of every region and behind the last
``reversed``   the ``gaps`` layout with region s+1 below region s in memory
``phase1/2/3`` gapped, every offset = r (mod 4)
``off_line``   gapped, every offset = 4 (mod 32): 16-byte aligned float32
               regions that are not 128-byte aligned

``unit`` keeps a required multiple (16 keys for ``bm32``, the row pitch for
pitched ``dist``); the phase families need unit 1, ``off_line`` a unit that
divides 4.  ``image`` builds what a buffer must hold after a launch (a
sentinel everywhere but the regions), ``first_diff`` says where a buffer
departs from it.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np

FAMILIES = ("tight", "gaps", "reversed", "phase1", "phase2", "phase3", "off_line")
PHASES = {"phase1": 1, "phase2": 2, "phase3": 3}
MAX_GAP = 37

# values no kernel writes: a finite float with an odd bit pattern (no residual
# or cost of the test scenes has these bits), an integer that is no index and
# no status, a 16-bit key below every key of a value >= +0 (those have the top
# bit set) that is not the NaN key 0 either
F32_SENTINEL_BITS = 0x4B5A5A5B
F64_SENTINEL_BITS = 0x4B5A5A5B5A5A5A5B
I32_SENTINEL = -2 ** 31 + 7
I64_SENTINEL = -2 ** 63 + 7
K16_SENTINEL = 0x5A5A
U8_SENTINEL = 0xA5


class Layout(NamedTuple):
    family: str
    unit: int
    offs: np.ndarray      # int64 [n]: first element of region s
    sizes: np.ndarray     # int64 [n]
    total: int            # elements of the buffer (a gap behind the last region included)

    def order(self) -> np.ndarray:
        """Region indices by ascending address (empty regions included)."""
        return np.lexsort((np.arange(self.offs.size), self.offs))


def layout(sizes: Sequence[int], family: str, unit: int = 1, seed: int = 0) -> Layout:
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if (sizes < 0).any():
        raise ValueError("negative region size")
    if family not in FAMILIES:
        raise ValueError(f"unknown family {family!r}")
    if unit < 1:
        raise ValueError("unit must be >= 1")
    if family in PHASES and unit != 1:
        raise ValueError("the phase families need unit 1")
    if family == "off_line" and 4 % unit:
        raise ValueError("off_line: offsets = 4 (mod 32) need a unit that divides 4")
    n = sizes.size
    up = lambda x, m: (x + m - 1) // m * m
    offs = np.zeros(n, np.int64)
    if family == "tight":
        end = 0
        for s in range(n):
            offs[s] = up(end, unit)
            end = offs[s] + sizes[s]
        return Layout(family, unit, offs, sizes, int(up(end, unit)))
    rng = np.random.default_rng([seed, n, unit, FAMILIES.index(family)])
    gaps = rng.integers(1, MAX_GAP + 1, size=n + 1) * unit
    walk = range(n - 1, -1, -1) if family == "reversed" else range(n)
    end = 0
    for q, s in enumerate(walk):
        o = up(end, unit) + int(gaps[q])
        if family in PHASES:
            o += (PHASES[family] - o) % 4
        elif family == "off_line":
            o += (4 - o) % 32
        offs[s] = o
        end = o + int(sizes[s])
    return Layout(family, unit, offs, sizes, int(up(end, unit) + gaps[n]))


def sentinel(dtype) -> np.generic:
    """The fill value of a buffer of ``dtype`` (numpy dtype)."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array([F32_SENTINEL_BITS], np.uint32).view(np.float32)[0]
    if dtype == np.float64:
        return np.array([F64_SENTINEL_BITS], np.uint64).view(np.float64)[0]
    if dtype == np.int32:
        return np.int32(I32_SENTINEL)
    if dtype == np.int64:
        return np.int64(I64_SENTINEL)
    if dtype in (np.uint16, np.int16):
        return np.array([K16_SENTINEL], np.uint16).view(dtype)[0]
    if dtype == np.uint8:
        return np.uint8(U8_SENTINEL)
    raise ValueError(f"no sentinel for {dtype}")


def blank(total: int, dtype) -> np.ndarray:
    """A buffer of ``total`` elements holding the sentinel everywhere."""
    return np.full(int(total), sentinel(dtype), dtype=np.dtype(dtype))


def image(lay: Layout, dtype, regions: Sequence[Optional[np.ndarray]], tail: int = 0) -> np.ndarray:
    """The buffer ``lay`` describes (+ ``tail`` elements): the sentinel
    everywhere, ``regions[s]`` (flattened; None: left as sentinel) at
    ``lay.offs[s]``."""
    out = blank(lay.total + tail, dtype)
    if len(regions) != lay.offs.size:
        raise ValueError("one region (or None) per offset")
    for s, r in enumerate(regions):
        if r is None:
            continue
        r = np.ascontiguousarray(r).reshape(-1)
        if r.dtype != out.dtype:
            raise ValueError(f"region {s} is {r.dtype}, the buffer {out.dtype}")
        if r.size != lay.sizes[s]:
            raise ValueError(f"region {s} holds {r.size} elements, its size is {lay.sizes[s]}")
        out[lay.offs[s]:lay.offs[s] + r.size] = r
    return out


def gather(buf: np.ndarray, lay: Layout) -> List[np.ndarray]:
    """The regions of ``buf`` (views), in region order."""
    return [buf[o:o + n] for o, n in zip(lay.offs, lay.sizes)]


def _bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def locate(lay: Layout, index: int) -> str:
    """Where element ``index`` of the buffer lies: 'region s (+k of n)', the
    gap in front of a region, or the tail behind the last."""
    for s in lay.order():
        o, n = int(lay.offs[s]), int(lay.sizes[s])
        if o <= index < o + n:
            return f"region {s} (+{index - o} of {n}, offset {o})"
    above = [int(s) for s in lay.order() if lay.offs[s] > index]
    if above:
        s = above[0]
        return f"gap {int(lay.offs[s]) - index} below region {s} (offset {int(lay.offs[s])})"
    return f"tail, {index - int((lay.offs + lay.sizes).max(initial=0))} past the last region"


def first_diff(got: np.ndarray, want: np.ndarray, lay: Layout, what: str = "buffer") -> Optional[str]:
    """None when ``got`` equals ``want`` bit for bit (floats as bit patterns,
    so NaN == NaN and -0 != +0); else a message naming the first differing
    index and the region or gap it lies in."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    g, w = _bits(got), _bits(want)
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (f"{what} [{lay.family}]: {bad.size} of {g.size} elements differ, first at {i} in "
            f"{locate(lay, i)}: got {got[i]!r} (bits {int(g[i]):#x}), want {want[i]!r} "
            f"(bits {int(w[i]):#x})")


def assert_image(got: np.ndarray, want: np.ndarray, lay: Layout, what: str = "buffer") -> None:
    msg = first_diff(got, want, lay, what)
    assert msg is None, msg
