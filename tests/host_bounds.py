"""Inputs, bounds grids and expected results of the host-bounds tests
(test_host_bounds_model.py on the CPU, test_host_bounds_gpu.py on the GPU); a
plain helper module: numpy, scipy and the oracle only, no GPU import.

include/mvmatch.h gives every launch a bound the host knows while the real
sizes stay on the device: ``max_n`` (pairwise, fp64, cube, bmin8, minima and
the ``_resid`` entry points), ``long_min / long_max / short_max`` (the
assignment) and ``max_rows`` (mvm_extend_costs).  Each is an UPPER bound
(``long_min`` a lower one): a caller sizes once for a capacity and feeds
batches whose counts change.  The plans always pass the batch's exact maxima,
so everything here is about bounds that are loose: above every real size and
across a limit at which the host picks another kernel, lane shape, grid or
LDS size -- with no problem or view of that class in the batch.

Every batch is built here once and is read-only; the expected results (scipy,
oracle/) are computed here, so the GPU file only compares.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Sequence, Tuple

import numpy as np
from scipy.optimize import linear_sum_assignment as scipy_lsa

# sizes at which the host-side dispatch changes class (views or long sides)
CLASS_LIMITS = (16, 32, 64, 256, 1024)

LOOSEST = (1, 2 ** 62, 2 ** 62)
CAPACITY = (1, 65536, 1024)          # the candidate-list and split-register classes' limits


def _ro(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ============================================================ assignment ====
LSAP_DENSE = [(1, 1), (3, 5), (5, 3), (40, 9), (9, 40), (64, 16), (300, 20), (24, 600), (769, 4), (1024, 3),
              (1025, 2), (1100, 5), (2500, 11), (4096, 6), (4097, 3), (5000, 20)]
LSAP_LISTS = [(4500, 64)]            # the candidate-list class with real lists
LSAP_EMPTY = [(0, 4), (4, 0)]
# the empties between the others: a kernel that walks the batch meets them mid-way
LSAP_SHAPES = LSAP_DENSE[:6] + LSAP_EMPTY[:1] + LSAP_DENSE[6:] + LSAP_LISTS + LSAP_EMPTY[1:]
LSAP_VARIANTS = ("normal", "ties")
# option sets of tests/test_lsap_gpu.py's LSAP_PATHS the grid runs under
LSAP_OPTION_SETS = ("default", "reg", "lds", "workgroup", "multi", "mreg", "sparse_lo", "sparse_tb1")
L_GRID = (5000, 8192, 8193, 65536, 65537)


@functools.lru_cache(maxsize=None)
def lsap_batch(dtype: str = "float32") -> Tuple[np.ndarray, ...]:
    """Every shape of LSAP_SHAPES twice -- random-normal costs, then the same
    rounded to half-integers (heavy exact ties) -- as ``dtype`` matrices:
    problem 2q is the normal and 2q + 1 the tied form of shape q."""
    rng = np.random.default_rng(1234)
    mats = []
    for shape in LSAP_SHAPES:
        c = rng.normal(size=shape)
        mats.append(_ro(c.astype(dtype)))
        mats.append(_ro((np.round(c * 2) / 2).astype(dtype)))
    return tuple(mats)


@functools.lru_cache(maxsize=None)
def lsap_expected(dtype: str = "float32"):
    """scipy's (row_ind, col_ind) of every problem of lsap_batch(dtype)."""
    return tuple(tuple(_ro(x.astype(np.int64)) for x in scipy_lsa(m)) for m in lsap_batch(dtype))


def shapes_of(mats: Sequence[np.ndarray]) -> List[Tuple[int, int]]:
    return [tuple(int(x) for x in m.shape) for m in mats]


def tight_bounds(shapes: Sequence[Tuple[int, int]]) -> Tuple[int, int, int]:
    """(long_min, long_max, short_max) over the non-empty problems, as
    ops.LsapPlan states them ((0, 0, 0): every problem is empty)."""
    ne = [(max(r, c), min(r, c)) for r, c in shapes if r > 0 and c > 0]
    if not ne:
        return 0, 0, 0
    return min(l for l, _ in ne), max(l for l, _ in ne), max(s for _, s in ne)


def lsap_bounds_grid(shapes: Sequence[Tuple[int, int]]) -> Dict[str, Tuple[int, int, int]]:
    """The (long_min, long_max, short_max) triples every assignment launch of
    the grid runs under; "tight" first (the run the others are compared with)."""
    lo, hi, sh = tight_bounds(shapes)
    grid = {"tight": (lo, hi, sh), "loosest": LOOSEST, "min_only": (1, hi, sh), "capacity": (lo, 65536, 1024)}
    for L in L_GRID:
        grid[f"L{L}"] = (1, L, L)
    return grid


def bounds_hold(bounds: Tuple[int, int, int], shapes: Sequence[Tuple[int, int]]) -> bool:
    lo, hi, sh = tight_bounds(shapes)
    if (lo, hi, sh) == (0, 0, 0):
        return True
    return bounds[0] <= lo and bounds[1] >= hi and bounds[2] >= sh


def _indices(pred) -> Tuple[int, ...]:
    return tuple(k for k, (r, c) in enumerate(shapes_of(lsap_batch())) if pred(r, c))


def lsap_sub_batches() -> Dict[str, Tuple[int, ...]]:
    """Problem indices of lsap_batch: under the loosest bound each sub-batch
    launches kernel classes that then find no problem of theirs."""
    return {
        "upto64": _indices(lambda r, c: 0 < min(r, c) and max(r, c) <= 64),
        "empties": _indices(lambda r, c: r == 0 or c == 0),
        "workgroup": _indices(lambda r, c: (r, c) in ((2500, 11), (1100, 5))),
        "lists": _indices(lambda r, c: (r, c) == (4500, 64)),
    }


def oracle_status(m: np.ndarray) -> int:
    """The status include/mvmatch.h gives problem ``m``, from oracle/lsap.py's
    restatement of scipy's solver: 0 solved, 1 NaN / -inf entries, 2 infeasible."""
    from oracle import lsap as OL
    try:
        OL.linear_sum_assignment(m)
    except OL.LsapError as e:
        return 1 if "invalid" in str(e) else 2
    return 0


@functools.lru_cache(maxsize=None)
def lsap_batch_y() -> Tuple[np.ndarray, ...]:
    """The second batch of the reuse test (float32): other shapes and data
    than lsap_batch, fewer problems, and between valid problems one with a NaN
    (status 1) and one whose short-side column 2 is all +inf (status 2), both
    of the candidate-list class so that its counters are defined for them."""
    rng = np.random.default_rng(99)
    shapes = [(7, 3), (4500, 8), (300, 21), (4200, 5), (2, 1025), (0, 2), (6000, 12), (33, 33)]
    mats = [rng.normal(size=s).astype(np.float32) for s in shapes]
    mats[1][4321, 5] = np.nan
    mats[3][:, 2] = np.inf
    mats[7] = np.round(mats[7] * 2) / 2
    return tuple(_ro(m) for m in mats)


LSAP_Y_STATUS = (0, 1, 0, 2, 0, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def lsap_expected_y():
    """scipy's assignment of the valid problems of lsap_batch_y (None: failed)."""
    return tuple(tuple(_ro(x.astype(np.int64)) for x in scipy_lsa(m)) if st == 0 else None
                 for m, st in zip(lsap_batch_y(), LSAP_Y_STATUS))


# ======================================================= three-view scenes ===
def scenes(counts, seed: int):
    """(pts, F, cam_offs) of one synth.make_scenes scene per count triple
    (tests/test_cubefree_gpu.py's _scenes): half-pixel centroids, a jittered rig."""
    from bpc_baseline_amd.synth import make_scenes
    sc = [make_scenes(1, 3, list(c), seed=seed + 17 * s) for s, c in enumerate(counts)]
    pts = np.concatenate([x.pts for x in sc]).reshape(-1, 2)
    F = np.concatenate([x.F for x in sc]).reshape(-1, 9)
    co = np.zeros(3 * len(counts) + 1, np.int64)
    np.cumsum(np.array(counts).reshape(-1), out=co[1:])
    return np.ascontiguousarray(pts, np.float64), np.ascontiguousarray(F, np.float64), co


def keys16(values: np.ndarray) -> np.ndarray:
    """Upper 16 bits of the order-preserving key of float32 values (NaN: 0)."""
    v = np.ascontiguousarray(values, np.float32)
    b = (v.view(np.uint32) | np.uint32(0x80000000)) >> np.uint32(16)
    return np.where(np.isnan(v), np.uint32(0), b).astype(np.uint16)


class CubeBatch:
    """A three-view batch with everything the oracle says about it: per scene
    the cube, argmin, minimum, 8-row minima, 32-column block minima, flattened
    (N*M, P) problems with scipy's assignment (None where oracle_status is
    not 0), all read-only."""

    def __init__(self, counts, seed: int, edit=None):
        from oracle import oracle as O
        self.counts = [tuple(int(x) for x in c) for c in counts]
        self.S = len(self.counts)
        pts, F, co = scenes(self.counts, seed)
        if edit is not None:
            edit(pts, F, co)
        self.pts, self.F, self.co = _ro(pts), _ro(F), _ro(co)
        self.max_view = max(max(c) for c in self.counts)
        rc, ra, rm, coffs, roffs = O.cube(pts, co, F, self.S)
        self.cubes, self.amins, self.mins, self.bm8, self.bm32 = [], [], [], [], []
        for s, (N, M, P) in enumerate(self.counts):
            c = rc[coffs[s]:coffs[s + 1]]
            self.cubes.append(_ro(c))
            self.amins.append(_ro(ra[roffs[s]:roffs[s + 1]]))
            self.mins.append(_ro(rm[roffs[s]:roffs[s + 1]]))
            if N * M * P:
                k8 = O.bmin8_keys(c.reshape(N, M, P))
                self.bm8.append(_ro(k8.reshape(-1)))
                self.bm32.append(_ro(O.bm32_keys(k8, N, M, P).reshape(-1)))
            else:
                self.bm8.append(_ro(np.zeros(0, np.uint16)))
                self.bm32.append(_ro(np.zeros(0, np.uint16)))

    def flat(self, s: int) -> np.ndarray:
        N, M, P = self.counts[s]
        return self.cubes[s].reshape(N * M, P)

    @functools.cached_property
    def status(self) -> Tuple[int, ...]:
        return tuple(oracle_status(self.flat(s)) if self.flat(s).size else 0 for s in range(self.S))

    @functools.cached_property
    def assignment(self):
        return tuple(tuple(_ro(x.astype(np.int64)) for x in scipy_lsa(self.flat(s))) if st == 0 else None
                     for s, st in enumerate(self.status))

    def residuals(self, max_n: int) -> np.ndarray:
        from oracle import oracle as O
        return O.residuals(self.pts, self.co, self.F, self.S, max_n)

    def select(self, s: int, row_ind, col_ind, threshold: float):
        """oracle/pipeline.select_sort of scene s under an assignment."""
        from oracle import pipeline as OP
        N, M, P = self.counts[s]
        return OP.select_sort(self.cubes[s], M, P, row_ind, col_ind, threshold)


# view sizes of each ragged batch -> (its scenes, the max_n values to run); the
# first max_n is the tight one
CUBE_SETS = {
    "v16": ([(16, 5, 1), (5, 16, 16), (0, 5, 16), (1, 1, 1)], (16, 17, 33, 64, 65, 257)),
    "v32": ([(32, 24, 31), (31, 32, 24), (24, 31, 32)], (32, 48, 49, 97, 193, 256, 300)),
    "v100": ([(100, 47, 64), (64, 100, 47), (47, 64, 100)], (100, 128, 161, 256, 257, 520)),
}
CUBE_VIEWS = {"v16": {0, 1, 5, 16}, "v32": {24, 31, 32}, "v100": {47, 64, 100}}
# the limits each set's max_n values cross with no view above them
CUBE_CROSSED = {"v16": {16, 32, 64, 256}, "v32": {32, 64, 256}, "v100": {256}}
CUBE_ARGMIN_PATHS = ("default", "fused", "workspace", "generic", "small")
CUBE_BMIN8_PATHS = ("default", "generic")
SMALL_KERNEL_BELOW = 64              # MVM_CUBE_SMALL: views < 64


@functools.lru_cache(maxsize=None)
def cube_batch(name: str) -> CubeBatch:
    return CubeBatch(CUBE_SETS[name][0], 40 + len(name))


def crossed(limits, real_max: int, bounds) -> set:
    """The class limits L no real size exceeds (real_max <= L) that the bounds
    straddle: some bound is <= L and some is > L."""
    return {L for L in limits if real_max <= L and any(b <= L for b in bounds) and any(b > L for b in bounds)}


def straddles(bounds, below: int, above: int) -> bool:
    """Both sides of a class limit are run: ``below`` and ``above`` are bounds."""
    return below in bounds and above in bounds


# the two 70..100-view cubes of the bmin8 assignment under CAPACITY
BMIN8_COUNTS = [(70, 100, 85), (96, 71, 100)]


@functools.lru_cache(maxsize=None)
def bmin8_batch() -> CubeBatch:
    return CubeBatch(BMIN8_COUNTS, 8)


# ------------------------------------------------------- cube-free chain ----
CHAIN_X = [(64, 100, 80), (100, 70, 64)]
CHAIN_Y = [(90, 64, 100), (64, 70, 66), (80, 80, 64), (70, 64, 90)]
CHAIN_MAX_N = (100, 128, 256)        # tight for CHAIN_X, then loose
CHAIN_CAPACITY = 256
CHAIN_Y_STATUS = (0, 1, 2, 0)
HUGE = 1e200                         # a centroid that makes every float32 cost of its column +inf


def _edit_y(pts, F, co):
    pts[co[3 * 1 + 0] + 5] = np.nan              # scene 1: one NaN centroid in view 0 -> NaN entries
    pts[co[3 * 2 + 2] + 3] = HUGE                # scene 2: column 3 all +inf -> infeasible


@functools.lru_cache(maxsize=None)
def chain_batch(which: str) -> CubeBatch:
    if which == "x":
        return CubeBatch(CHAIN_X, 61)
    return CubeBatch(CHAIN_Y, 77, edit=_edit_y)


# ================================================================ pairwise ==
PAIR_VIEWS = {0, 1, 37, 255, 300}
PAIR_COUNTS = {3: [(300, 37, 0), (1, 255, 300)], 4: [(300, 0, 37, 255), (1, 255, 300, 37)]}
PAIR_MAX_N = (300, 301, 512, 1024, 1025, 2600)       # tight first
PAIR_F64_MAX_N = (300, 301, 1025)
PAIR_OPTIONS = {"default": {}, "eager": {"pairwise_argmin": "eager"}, "rpw4": {"pairwise_rows_per_wave": 4},
                "interleaved": {"pairwise_row_interleave": 1}, "contiguous": {"pairwise_row_interleave": -1}}
FRONTS_BYTES = 8e9                   # mvm_pairwise.hip: 4 write fronts from this many padded bytes


def pairs_of(C: int) -> np.ndarray:
    return np.array([[a, b] for a in range(C) for b in range(C) if a != b], np.int32)


def fronts_max_n(S: int, P: int) -> int:
    """The smallest max_n at which the launch's own rule (padded bound
    S * P * max_n^2 * 4 B >= 8 GB) picks 4 XCD write fronts."""
    n = int(math.isqrt(int(FRONTS_BYTES // (S * P * 4))))
    while float(S * P) * n * n * 4 < FRONTS_BYTES:
        n += 1
    return n


def pair_max_ns(C: int) -> Tuple[int, ...]:
    return PAIR_MAX_N + (fronts_max_n(len(PAIR_COUNTS[C]), len(pairs_of(C))),)


class PairBatch:
    """Ragged C-view scenes with the NaN / inf / huge centroids and the
    degenerate F of test_pairwise_edge_cases, and the oracle's float32
    matrices, argmins and minima per (scene, pair)."""

    def __init__(self, C: int):
        from oracle import oracle as O
        rng = np.random.default_rng(50 + C)
        cnt = np.asarray(PAIR_COUNTS[C], np.int64)
        self.C, self.S, self.pairs = C, cnt.shape[0], pairs_of(C)
        co = np.zeros(cnt.size + 1, np.int64)
        np.cumsum(cnt.reshape(-1), out=co[1:])
        pts = np.floor(rng.uniform(0, 4800, size=(int(co[-1]), 2))) / 2
        pts[3] = [np.nan, 4.0]
        pts[9] = [np.inf, 1.0]
        pts[20] = [1e300, -1e300]
        pts[21] = [2.0 ** 41, 7.0]
        pts[int(co[-1]) - 2] = [7.5, np.nan]
        P = len(self.pairs)
        F = rng.normal(size=(self.S * P, 9))
        F[0, 0:6] = 0.0                          # degenerate row lines
        F[P + 1, [0, 1, 3, 4, 6, 7]] = 0.0       # degenerate column lines
        F[P + 2] = 0.0                           # both
        F[2] *= 1e-9                             # norms near the 1e-8 threshold
        self.pts, self.F, self.co = _ro(pts), _ro(F), _ro(co)
        self.na = cnt[:, self.pairs[:, 0]].reshape(-1)
        self.nb = cnt[:, self.pairs[:, 1]].reshape(-1)
        rd, ra, rm, doffs, roffs = O.pairwise(pts, co, F, self.pairs, self.S, C)
        n = self.na.size
        self.mats = [_ro(rd[doffs[q]:doffs[q + 1]].reshape(self.na[q], self.nb[q])) for q in range(n)]
        self.amins = [_ro(ra[roffs[q]:roffs[q + 1]]) for q in range(n)]
        self.mins = [_ro(rm[roffs[q]:roffs[q + 1]]) for q in range(n)]

    def pitched(self, row_align: int) -> List[np.ndarray]:
        """The matrices with rows of roundup(n_b, row_align), padding +inf."""
        out = []
        for m in self.mats:
            ld = (m.shape[1] + row_align - 1) // row_align * row_align
            p = np.full((m.shape[0], ld), np.inf, np.float32)
            p[:, :m.shape[1]] = m
            out.append(p.reshape(-1))
        return out

    def f64(self) -> List[np.ndarray]:
        """Per (scene, pair) the oracle's fp64 residuals: the pair as views 0
        and 1 of a three-view scene with an empty third (oracle.residuals' e12)."""
        from oracle import oracle as O
        out = []
        for q in range(self.na.size):
            s, p = divmod(q, len(self.pairs))
            a, b = (int(self.co[self.C * s + c]) for c in self.pairs[p])
            na, nb = int(self.na[q]), int(self.nb[q])
            sub = np.concatenate([self.pts[a:a + na], self.pts[b:b + nb]])
            sco = np.array([0, na, na + nb, na + nb], np.int64)
            e = O.residuals(sub, sco, np.repeat(self.F[q:q + 1], 3, axis=0), 1, max(na, nb, 1))
            out.append(_ro(e[0, 0, :na, :nb].copy()))
        return out


@functools.lru_cache(maxsize=None)
def pair_batch(C: int) -> PairBatch:
    return PairBatch(C)


# ================================================================== extend ==
EXTEND_COUNTS = (0, 1, 63, 65)
EXTEND_MAX_ROWS = (65, 66, 128, 4096)            # tight first; 64 rows per workgroup
EXTEND_COLS = [(12, 5), (64, 3), (7, 260), (33, 8)]


# ============================================================ graph replay ==
GRAPH_PAIR_MAX_N = 1025
GRAPH_CUBE_MAX_N = 257
GRAPH_PAIR_COUNTS = [[(200, 37, 1), (3, 255, 120)], [(64, 300, 0), (17, 5, 90)]]     # first, second batch
GRAPH_CUBE_COUNTS = [[(16, 5, 12), (40, 33, 52), (9, 64, 7)], [(31, 32, 24), (3, 100, 20), (64, 1, 47)]]
GRAPH_PAIRS = pairs_of(3)


class GraphBatch:
    """One batch of the replay test: a pairwise part and a cube part with the
    oracle's outputs, in the plans' tight layouts."""

    def __init__(self, which: int):
        from oracle import oracle as O
        rng = np.random.default_rng(300 + which)
        cnt = np.asarray(GRAPH_PAIR_COUNTS[which], np.int64)
        self.pS = cnt.shape[0]
        co = np.zeros(cnt.size + 1, np.int64)
        np.cumsum(cnt.reshape(-1), out=co[1:])
        self.p_pts = _ro(np.floor(rng.uniform(0, 4800, size=(int(co[-1]), 2))) / 2)
        self.p_F = _ro(rng.normal(size=(self.pS * len(GRAPH_PAIRS), 9)))
        self.p_co = _ro(co)
        self.dist, self.amin, self.minv, self.dist_offs, self.row_offs = O.pairwise(
            self.p_pts, co, self.p_F, GRAPH_PAIRS, self.pS, 3)
        self.cube = CubeBatch(GRAPH_CUBE_COUNTS[which], 500 + which)
        c = np.asarray(GRAPH_CUBE_COUNTS[which], np.int64)
        self.cube_offs = np.concatenate([[0], np.cumsum(c.prod(axis=1))]).astype(np.int64)
        self.crow_offs = np.concatenate([[0], np.cumsum(c[:, 0] * c[:, 1])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def graph_batch(which: int) -> GraphBatch:
    return GraphBatch(which)
