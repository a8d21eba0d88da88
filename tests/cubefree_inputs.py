"""Hand-built inputs for the cube-free association's edge tests
(test_cubefree_edges_model.py on the CPU, test_cubefree_edges_gpu.py on the
GPU); a plain helper module, no fixtures.

The rectified scene.  mvm_triplet_minima takes F as an input, so a test picks
it: with ``FR = [[0,0,0],[0,0,-1],[0,1,0]]`` for all three pairs every epipolar
line is (0, -+1, +-y) with unit norm (oracle/mvm_oracle.c: l2 = F p1, l1 = F^T
p2), both point-line distances of a pair are |y - y'|, a pair residual is
``0.5 * (|y - y'| + |y - y'|)`` and a cube entry

    float32(((|y_i - y_j| + |y_i - y_k|) + |y_j - y_k|) / 3)

depends on the y coordinates alone.  A test therefore writes the cube it wants:
exact ties and zeros (y on a coarse grid), a sum that straddles a 16-bit key
carry, residuals at and above 2^64, float32 costs of +inf, non-finite sums.

Every named case below is built here once, so the CPU file can pin what the
GPU file runs (closed form == oracle, the solver model's regime) and the GPU
tests cannot pass on inputs that miss the code they are about.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

FR = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])

TWO64 = 2.0 ** 64                               # kApproxResidual (csrc/mvm_cube.hip)
TWO64_UP = float(np.nextafter(TWO64, np.inf))
HUGE = (1e30, 1e200, 1.7e308)                   # > 2^64 | float32 cost +inf | d1 + d2 overflows


@dataclass
class Scene:
    """One 3-view scene: views = three f64 [n, 2] arrays, F = f64 [3, 9]
    (F12, F13, F23); rect: the F are FR (the closed form holds)."""
    views: List[np.ndarray]
    F: np.ndarray
    rect: bool = False
    note: dict = field(default_factory=dict)

    @property
    def counts(self) -> Tuple[int, int, int]:
        return tuple(len(v) for v in self.views)

    @property
    def ys(self) -> List[np.ndarray]:
        return [v[:, 1] for v in self.views]


@dataclass
class Batch:
    pts: np.ndarray            # f64 [sum n, 2]
    F: np.ndarray              # f64 [3 S, 9]
    co: np.ndarray             # i64 [3 S + 1]
    scenes: List[Scene]

    @property
    def counts(self) -> List[Tuple[int, int, int]]:
        return [s.counts for s in self.scenes]


def batch_of(scenes: Sequence[Scene]) -> Batch:
    pts = np.concatenate([v for s in scenes for v in s.views]).astype(np.float64)
    F = np.concatenate([s.F.reshape(3, 9) for s in scenes])
    co = np.zeros(3 * len(scenes) + 1, np.int64)
    np.cumsum([len(v) for s in scenes for v in s.views], out=co[1:])
    return Batch(np.ascontiguousarray(pts), np.ascontiguousarray(F), co, list(scenes))


def half_grid(n_values: int, lo: float = 100.5, step: float = 1.0) -> np.ndarray:
    """n_values half-integer-aligned y values lo, lo + step, ..."""
    return lo + step * np.arange(n_values)


def rect_scene(counts, grids, seed: int, overrides=(), x: Optional[Sequence[np.ndarray]] = None) -> Scene:
    """A rectified scene: view v's y drawn (seeded) from ``grids[v]`` (one grid
    for all views if ``grids`` is a single array), then single points
    overridden: ``overrides`` = [(view, index, y), ...].  x is irrelevant to
    the costs (FR's first column and row are zero); half-integers by default."""
    rng = np.random.default_rng(seed)
    if isinstance(grids, np.ndarray):
        grids = [grids] * 3
    views = []
    for v, n in enumerate(counts):
        y = rng.choice(np.asarray(grids[v], np.float64), size=n)
        xs = np.floor(rng.uniform(0.0, 2400.0, n)) + 0.5 if x is None else np.asarray(x[v], np.float64)
        views.append(np.stack([xs, y], axis=1))
    for v, idx, y in overrides:
        views[v][idx, 1] = y
    return Scene(views, np.tile(FR.reshape(1, 9), (3, 1)), rect=True)


def synth_scene(counts, seed: int, zero_f: Sequence[int] = ()) -> Scene:
    """One synth.make_scenes scene (half-integer centroids under a jittered
    rig); zero_f: the pairs (0: F12, 1: F13, 2: F23) whose F is zeroed, so
    every line of theirs is degenerate and the residual the 9999 sentinel."""
    from bpc_baseline_amd.synth import make_scenes
    b = make_scenes(1, 3, list(counts), seed=seed)
    F = b.F.reshape(3, 9).copy()
    for p in zero_f:
        F[p] = 0.0
    return Scene([b.pts[b.cam_offs[v]:b.cam_offs[v + 1]].copy() for v in range(3)], F)


def duplicated(scene: Scene, frac: float, seed: int) -> Scene:
    """``frac`` of each view's detections replaced by exact copies of other
    detections of the same view (tools/bench_lsap_adversarial.py's dup cases):
    copies in view 2 give identical short-side rows of the flattened (N*M, P)
    problem, copies in views 0 and 1 identical long-side columns."""
    rng = np.random.default_rng(seed)
    views = []
    for v in scene.views:
        v = v.copy()
        n = len(v)
        k = int(round(frac * n))
        if k and n > k:
            dst = rng.choice(n, size=k, replace=False)
            src = rng.choice(np.setdiff1d(np.arange(n), dst), size=k)
            v[dst] = v[src]
        views.append(v)
    return Scene(views, scene.F.copy(), rect=scene.rect, note=dict(scene.note))


# ------------------------------------------------------------ closed form ----
def closed_form_pair(ya: np.ndarray, yb: np.ndarray) -> np.ndarray:
    """e[a, b] = 0.5 * (d + d), d = |ya - yb| (both point-line distances)."""
    with np.errstate(over="ignore"):
        d = np.abs(np.asarray(ya, np.float64)[:, None] - np.asarray(yb, np.float64)[None, :])
        return 0.5 * (d + d)


def closed_form_cube(y0, y1, y2) -> np.ndarray:
    """float32 [N, M, P] cube of a rectified scene from its y coordinates."""
    e12, e13, e23 = closed_form_pair(y0, y1), closed_form_pair(y0, y2), closed_form_pair(y1, y2)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (e12[:, :, None] + e13[:, None, :]) + e23[None, :, :]
        return (s / 3.0).astype(np.float32)


def closed_form_residuals(y0, y1, y2, max_n: int) -> np.ndarray:
    """The layout of oracle.residuals for one scene: f64 [3, max_n, ld] =
    e12 [N][ld], e13T [P][ld], e23T [P][ld]; NaN outside the views."""
    ld = (max_n + 3) // 4 * 4
    out = np.full((3, max_n, ld), np.nan)
    N, M, P = len(y0), len(y1), len(y2)
    out[0, :N, :M] = closed_form_pair(y0, y1)
    out[1, :P, :N] = closed_form_pair(y0, y2).T
    out[2, :P, :M] = closed_form_pair(y1, y2).T
    return out


# --------------------------------------------------------- carry straddle ----
def key16(bits) -> np.ndarray:
    """The 16-bit key of float32 bit patterns (>= +0): upper half of bits | sign."""
    return ((np.asarray(bits).astype(np.int64) | 0x80000000) >> 16).astype(np.int64)


def straddle_sums() -> np.ndarray:
    """Every s = m * 2^-14 < 2^10 (exact in float32) whose approximate third
    float32(s) * float32(1/3) and exact third float32(s / 3) lie either side
    of a 16-bit key carry: the kernel's float32 block minimum has the wrong
    key there and its fp64 recheck must change it."""
    m = np.arange(1, 1 << 24, dtype=np.int64)
    s = m.astype(np.float64) * 2.0 ** -14
    approx = (s.astype(np.float32) * np.float32(1.0 / 3.0)).astype(np.float32).view(np.uint32)
    exact = (s / 3.0).astype(np.float32).view(np.uint32)
    return s[key16(approx) != key16(exact)]


def straddle_scene(counts, i_star: int, j_star: int, k_star: int, s: float, seed: int) -> Scene:
    """A rectified scene whose triple (i*, j*, k*) has the fp64 sum ``s`` (one
    of straddle_sums) and is the strict minimum of its 8-row group and of its
    32-column block for (i*, k*): collinear y_i* = 0 < y_j* < y_k* = s / 2
    gives the sum 2 y_k*; every other j of the block lies above y_k*, so its
    sum 2 y_j is larger.  Every partial float32 sum is exact (y_k* has 24
    significant bits), so the only error of the kernel's float32 minimum is
    the multiply by float32(1/3)."""
    N, M, P = counts
    sc = rect_scene(counts, [half_grid(60, 1000.5), half_grid(60, 600.5), half_grid(60, 800.5)], seed)
    yk = s / 2.0
    assert yk < 600.0 and float(np.float32(yk)) == yk
    sc.views[0][i_star, 1] = 0.0
    sc.views[1][j_star, 1] = 100.5
    sc.views[2][k_star, 1] = yk
    sc.note = {"straddle": (i_star, j_star, k_star, s)}
    return sc


# ------------------------------------------------------------------ cases ----
# step 1.5: a cost is 2 * 1.5 * d / 3 = d, an integer (lower 16 bits zero: every
# block minimum of such a scene fails the float32 test and is rechecked);
# step 1.0: costs 2 d / 3, mostly safe lower bits
_GRID6 = half_grid(6, step=1.5)
_GRID20 = half_grid(20)
_GRID40 = half_grid(40)
_GRID20C = half_grid(20, step=1.5)
_GRID4000 = half_grid(4000, 0.5, 0.5)


def minima_cases() -> Dict[str, Batch]:
    """The batches of the minima tests.  Shapes: N % 16 != 0 and == 0 (the row
    loop and the unrolled whole-chunk path of with_bmin8=False), M % 32 != 0,
    P = 1 and P = 63, 64, 65 (either side of a wave of short-side columns)."""
    S = straddle_sums()
    out = {}
    out["coarse"] = batch_of([
        rect_scene((33, 45, 8), _GRID6, 1),
        rect_scene((32, 64, 1), _GRID6, 2),
        rect_scene((48, 40, 63), _GRID6, 3),
        rect_scene((16, 33, 64), _GRID20C, 4),
        rect_scene((20, 70, 65), _GRID40, 5),
        rect_scene((16, 32, 5), half_grid(1), 6),                 # one value: an all-zero cube
    ])
    # the straddling triple in j block 0 and in a later one; chunk 0 and a
    # later chunk; whole chunks (N = 32) and a ragged last chunk (N = 20)
    out["straddle"] = batch_of([
        straddle_scene((32, 64, 8), 5, 9, 3, float(S[0]), 11),
        straddle_scene((32, 70, 9), 21, 41, 0, float(S[len(S) // 2]), 12),
        straddle_scene((20, 45, 64), 17, 3, 63, float(S[-1]), 13),
        straddle_scene((20, 100, 5), 2, 97, 4, float(S[7]), 14),
    ])
    # a rectified scene between two make_scenes scenes: the chunk / wave flags
    # (degenerate, near, fast) of one scene do not leak into its neighbours
    out["mixed"] = batch_of([
        synth_scene((40, 70, 50), 21),
        rect_scene((48, 40, 20), _GRID6, 22, overrides=[(0, 20, 1e200)]),
        synth_scene((64, 64, 64), 23),
    ])
    # a residual exactly 2^64 (stays on the float32 path) and the next double
    # above it (the exact per-entry path), in different j blocks; and in view 0
    # (different chunks), and in view 2
    out["two64"] = batch_of([
        rect_scene((32, 100, 9), _GRID20, 31, overrides=[(1, 35, TWO64), (1, 70, TWO64_UP)]),
        rect_scene((48, 40, 9), _GRID20, 32, overrides=[(0, 20, TWO64), (0, 40, TWO64_UP)]),
        rect_scene((20, 40, 64), _GRID20, 33, overrides=[(2, 7, TWO64), (2, 63, TWO64_UP)]),
    ])
    # one point per view at 1e30 / 1e200 / 1.7e308: view 0 in a chunk other
    # than the first, view 1 in a j block other than the first; the scene's
    # other chunks / blocks stay on the float32 path
    huge = []
    for q, h in enumerate(HUGE):
        huge.append(rect_scene((48, 70, 20), _GRID20, 40 + 3 * q, overrides=[(0, 17 + 16 * (q % 2), h)]))
        huge.append(rect_scene((40, 70, 20), _GRID20, 41 + 3 * q, overrides=[(1, 33 + q, h)]))
        huge.append(rect_scene((32, 40, 65), _GRID20, 42 + 3 * q, overrides=[(2, 62 + q, h)]))
    out["huge"] = batch_of(huge)
    # costs below 2^-100 (kApproxTiny) that are not zero: y a few units of
    # 2^-130 apart (float32 subnormals), with fp64 values float32 cannot hold
    tiny_grid = np.arange(1, 41) * (2.0 ** -130) * (1.0 + 2.0 ** -20)
    # ... and y spread over every binade from 2^-101 down to 2^-152: normal and
    # subnormal float32 images, and fp64 values below the smallest subnormal
    wide_grid = 1.37 * (1.0 + 2.0 ** -20) * 2.0 ** -np.arange(101.0, 153.0)
    out["tiny"] = batch_of([rect_scene((32, 64, 8), tiny_grid, 51), rect_scene((20, 45, 9), tiny_grid, 52),
                            rect_scene((32, 70, 64), wide_grid, 53), rect_scene((20, 33, 65), wide_grid, 54)])
    return out


@dataclass
class AssignCase:
    batch: Batch
    regime: List[Optional[str]]        # per scene: "lists" | "overflow" | None (no claim)
    options: Optional[dict] = None
    status: Optional[List[int]] = None  # expected status per scene (default all 0)


ASSIGN_SHAPES = [(64, 64, 8), (64, 64, 64), (80, 70, 5), (100, 100, 100), (16, 256, 31), (256, 16, 1)]


def assign_cases() -> Dict[str, AssignCase]:
    out = {}
    out["lists"] = AssignCase(batch_of([rect_scene(c, _GRID4000, 60 + q) for q, c in enumerate(ASSIGN_SHAPES)]),
                              ["lists"] * len(ASSIGN_SHAPES))
    grids = [_GRID6, _GRID20, _GRID6, _GRID40, _GRID6, _GRID6]
    out["overflow"] = AssignCase(batch_of([rect_scene(c, g, 70 + q)
                                           for q, (c, g) in enumerate(zip(ASSIGN_SHAPES, grids))]),
                                 ["overflow"] * len(ASSIGN_SHAPES))
    # an all-zero cube (one y value), an all-sentinel cube (all three F zero),
    # next to a solved neighbour
    out["constant"] = AssignCase(batch_of([rect_scene((64, 64, 8), half_grid(1), 80),
                                           synth_scene((64, 64, 8), 81, zero_f=(0, 1, 2)),
                                           rect_scene((64, 64, 8), _GRID4000, 82),
                                           synth_scene((80, 70, 5), 83, zero_f=(0, 1, 2))]),
                                 ["overflow", "overflow", None, "overflow"])
    out["f13_zero"] = AssignCase(batch_of([synth_scene((64, 64, 64), 90), synth_scene((64, 64, 64), 91, zero_f=(1,)),
                                           synth_scene((80, 70, 50), 92, zero_f=(1,))]), [None] * 3)
    for pct in (10, 30):
        out[f"dup{pct}"] = AssignCase(batch_of([
            duplicated(synth_scene(c, 100 + pct + q), pct / 100.0, 200 + pct + q)
            for q, c in enumerate([(64, 64, 64), (80, 70, 5), (100, 100, 100), (64, 64, 8)])]), [None] * 4)
    # +inf entries that leave the problem feasible: a view-0 and a view-1
    # point at 1e200 (M resp. N long-side columns of +inf in every short row)
    out["inf_feasible"] = AssignCase(batch_of([
        rect_scene((64, 64, 8), _GRID4000, 110, overrides=[(0, 20, 1e200)]),
        rect_scene((80, 70, 5), _GRID20, 111, overrides=[(1, 40, 1e200), (0, 3, 1.7e308)]),
        rect_scene((64, 64, 64), _GRID40, 112, overrides=[(0, 63, 1e200), (1, 0, 1e30)])]), [None] * 3)
    # a view-2 point at 1e200: one short-side row all +inf, no assignment
    # exists (status 2, scipy raises); its neighbours are solved
    out["infeasible"] = AssignCase(batch_of([
        rect_scene((64, 64, 8), _GRID4000, 120),
        rect_scene((64, 64, 8), _GRID20, 121, overrides=[(2, 5, 1e200)]),
        synth_scene((80, 70, 5), 122),
        rect_scene((64, 64, 64), _GRID4000, 123, overrides=[(2, 63, 1e200)])]), [None] * 4, status=[0, 2, 0, 2])
    # below the default class: 33 * 32 = 1,056 long-side columns.  33 blocks:
    # theta is the 16th smallest block minimum, about half the columns lie at
    # or below it and every list overflows, whatever the grid
    out["min_cols"] = AssignCase(batch_of([rect_scene((33, 32, 8), _GRID4000, 130),
                                           rect_scene((33, 32, 8), _GRID6, 131)]),
                                 ["overflow", "overflow"], options={"lsap_sparse_min_cols": 1025})
    return out


def select_batch() -> Batch:
    """Rectified scenes for the select tail: every object's y (plus a per-view
    offset, so costs are not zero) appears twice in each view, so matches come
    in groups of bit-equal costs and the stable order shows."""
    scenes = []
    for q, (N, M, P) in enumerate([(64, 64, 8), (80, 70, 64), (16, 256, 31)]):
        rng = np.random.default_rng(140 + q)
        n_obj = max(N, M, P)
        base = 200.0 + 7.0 * rng.permutation(n_obj)              # objects 7 px apart
        ys = []
        for v, n in enumerate((N, M, P)):
            half = (n + 1) // 2
            obj = rng.permutation(min(n_obj, half))[:half] if half <= n_obj else np.arange(half) % n_obj
            y = base[obj] + 0.5 * rng.integers(0, 4, half)       # per-view offset of each object
            y = np.concatenate([y, y])[:n]                       # ... held twice
            ys.append(y[rng.permutation(n)])
        sc = rect_scene((N, M, P), _GRID6, 150 + q)
        for v in range(3):
            sc.views[v][:, 1] = ys[v]
        scenes.append(sc)
    return batch_of(scenes)


def dup_detector_batch(parts, frac: float, seed: int):
    """Concatenated synth.make_detector_batch captures, ``parts`` = [(captures,
    detections per view), ...], with ``frac`` of each image's boxes replaced
    by copies of other boxes of the image (box, confidence and class).
    -> (boxes, conf, cls, img_offs, Ks, RTs) on the host."""
    from bpc_baseline_amd.synth import make_detector_batch
    rng = np.random.default_rng(seed)
    bs = [make_detector_batch(n, d, seed=seed + 101 * q) for q, (n, d) in enumerate(parts)]
    img, base = [np.array([0], np.int64)], 0
    for b in bs:
        img.append(b.img_offs[1:] + base)
        base += int(b.img_offs[-1])
    cat = lambda k: np.concatenate([getattr(b, k) for b in bs])
    boxes, conf, cls, img_offs = cat("boxes").copy(), cat("conf").copy(), cat("cls").copy(), np.concatenate(img)
    for a, e in zip(img_offs[:-1], img_offs[1:]):
        n = int(e - a)
        k = int(round(frac * n))
        dst = a + rng.choice(n, size=k, replace=False)
        src = rng.choice(np.setdiff1d(np.arange(a, e), dst), size=k)
        boxes[dst], conf[dst], cls[dst] = boxes[src], conf[src], cls[src]
    return boxes, conf, cls, img_offs, cat("Ks"), cat("RTs")
