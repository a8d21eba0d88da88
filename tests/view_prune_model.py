"""Pruning of extra views by reprojection residual (DESIGN §3.15,
mvm_prune_views_triangulate) restated in numpy, and the inputs the CPU and GPU
tests share.  A helper, not a test.

The restatement follows the definition step by step: the DLT is
``oracle.pipeline.triangulate`` (numpy's SVD), the residual is §3.12's
sequence of single IEEE operations written elementwise (no ``@``: a BLAS may
fuse), so on the first pass -- X as it stands in the buffer -- it has the
kernel's bits, and after a drop it differs from the kernel's only through the
two DLTs (§3.8: rtol 1e-10, atol 1e-9 mm).

The builders make ``synth.make_rig`` rigs of C cameras and world points
projected exactly into every view.  Every extra view then moves by a small
known offset (detection noise, 0.05-0.45 px: above a gate of 0, below a gate
of 1) and chosen extra views by a gross one, by the row's kind:

  none     nothing more
  one      one view by 30 px
  two      two views by 40 and 80 px
  all      every extra view by 25-80 px
  masking  one view by 60-100 px: it drags X so far that the good views
           exceed a gate of 5 px as well, until it is gone

``tests/test_view_prune_model.py`` proves on the CPU that these rows are what
they are meant to be and that no decision is closer than the kernel's and the
restatement's X can differ.
"""
import functools

import numpy as np

from bpc_baseline_amd.inference.utils.camera_utils import projection_matrices
from bpc_baseline_amd.synth import make_rig
from oracle import pipeline as OP

I32_MIN = np.iinfo(np.int32).min
KINDS = ("none", "one", "two", "all", "masking")
GATES = (0.0, 1.0, 5.0, 20.0, float("inf"))
MAIN_GATE = 5.0
MARGIN = 1e-6                    # px: no decision closer than this (test_view_prune_model.py)
RTOL, ATOL = 1e-10, 1e-9         # §3.8


def residual(P, X, cent):
    """§3.12's reprojection residual, elementwise: P [..., 3, 4], X [..., 3],
    cent [..., 2] -> [...]."""
    with np.errstate(all="ignore"):
        h = [((P[..., q, 0] * X[..., 0] + P[..., q, 1] * X[..., 1]) + P[..., q, 2] * X[..., 2])
             + P[..., q, 3] for q in range(3)]
        u = h[0] / h[2]
        v = h[1] / h[2]
        du = u - cent[..., 0]
        dv = v - cent[..., 1]
        return np.sqrt(du * du + dv * dv)


def jacobian_norm(P, X):
    """The 2-norm of d(u, v)/dX of the projection by P [3, 4] at X [3]."""
    h = P[:, :3] @ X + P[:, 3]
    J = (P[:2, :3] * h[2] - h[:2, None] * P[2, :3][None, :]) / (h[2] * h[2])
    return float(np.linalg.norm(J, 2))


def _worst(r):
    """The camera to drop among the candidates ``r`` {d: residual}: NaN above
    every number, then the largest, ties to the lowest camera."""
    return min(r, key=lambda d: (0, 0.0, d) if np.isnan(r[d]) else (1, -r[d], d))


def prune(views, ext_cost, X, match_offs, count, pts, cam_offs, proj, gate):
    """The definition.  -> (views, ext_cost, X, pruned, touched, trace):
    copies of the three in/out arrays after pruning, pruned int32 [cap] (0
    outside the captures' rows), touched bool [cap] = the rows whose
    ``pruned`` word the kernel writes, and per evaluated pass a dict(row,
    passno, X, K, r {d: residual}, dropped)."""
    views, ext_cost, X = views.copy(), ext_cost.copy(), X.copy()
    cap, C = views.shape
    pruned = np.zeros(cap, np.int32)
    touched = np.zeros(cap, bool)
    trace = []
    proj = proj.reshape(-1, C, 3, 4)
    for s in range(count.size):
        mo = int(match_offs[s])
        co = cam_offs[C * s:C * s + C + 1]
        for w in range(min(int(count[s]), int(match_offs[s + 1]) - mo)):
            row = mo + w
            touched[row] = True
            v = views[row]
            if not all(0 <= v[c] < co[c + 1] - co[c] for c in range(3)):
                continue
            if not all(v[d] < co[d + 1] - co[d] for d in range(3, C)):      # no detection of its view
                continue
            K = [0, 1, 2] + [d for d in range(3, C) if v[d] >= 0]
            cent = {d: pts[co[d] + v[d]] for d in K}
            x, passno = X[row].copy(), 0
            while len(K) > 3:
                r = {d: float(residual(proj[s, d], x, cent[d])) for d in K if d >= 3}
                cand = {d: q for d, q in r.items() if not q <= gate}
                d = _worst(cand) if cand else None
                trace.append(dict(row=row, scene=s, passno=passno, X=x.copy(), K=tuple(K), r=r, dropped=d))
                if d is None:
                    break
                K.remove(d)
                views[row, d] = -1
                ext_cost[row, d - 3] = np.inf
                pruned[row] |= 1 << d
                x = OP.triangulate(proj[s, K][None], np.stack([cent[c] for c in K])[None])[0]
                passno += 1
            if pruned[row]:
                X[row] = x
    return views, ext_cost, X, pruned, touched, trace


class Case:
    """One input of the op: host arrays in the op's argument order (``args``),
    the true world point of every row (NaN outside the captures' rows) and the
    kind of every row ("" outside, "skip" for a row with a seed or an
    extra-view index out of range)."""
    FIELDS = ("views", "ext_cost", "X", "match_offs", "count", "pts", "cam_offs", "proj")

    def args(self):
        return tuple(getattr(self, k) for k in self.FIELDS)


def _offset(rng, lo, hi):
    """A pixel offset of length in [lo, hi], in a random direction."""
    a, m = rng.uniform(0, 2 * np.pi), rng.uniform(lo, hi)
    return np.array([m * np.cos(a), m * np.sin(a)])


def build(C, counts, caps, seed, *, kinds=KINDS, empty_view=(), bad_seed_rows=(), bad_extra_rows=(), nan_view=(),
          inf_view=(), tie=False, unkept=0.15):
    """``counts[s]`` matches in a segment of ``caps[s]`` rows per capture; row w
    of a capture is of kind ``kinds[w % len(kinds)]`` (kinds that need two
    extra views fall back to "one" at C = 4).  ``empty_view``: captures whose
    camera 3 has no detection; ``bad_seed_rows``: (capture, w) whose camera-1
    index is the view's size, ``bad_extra_rows``: whose camera-(C-1) index
    is; ``nan_view`` / ``inf_view``: captures whose
    camera C-1 has a P with rows 0 and 2 / row 2 zeroed (residual NaN / inf);
    ``tie``: camera 4 is camera 3 again, detections and shifts included;
    ``unkept``: the share of other extra-view slots left at -1.  Rows outside
    the captures' hold sentinels (views INT32_MIN, ext_cost / X NaN).  X
    arrives as the restatement's DLT over each row's kept views."""
    rng = np.random.default_rng(seed)
    counts, caps = np.asarray(counts, np.int32), np.asarray(caps, np.int64)
    S, n_ext = counts.size, C - 3
    c = Case()
    c.C, c.S, c.count = C, S, counts
    c.match_offs = np.zeros(S + 1, np.int64)
    np.cumsum(caps, out=c.match_offs[1:])
    cap = int(c.match_offs[-1])
    nv = np.repeat(counts.astype(np.int64)[:, None] + 2, C, axis=1)     # two clutter detections a view
    for s in empty_view:
        nv[s, 3] = 0
    c.cam_offs = np.zeros(S * C + 1, np.int64)
    np.cumsum(nv.reshape(-1), out=c.cam_offs[1:])
    c.pts = rng.uniform(0.0, 2400.0, (int(c.cam_offs[-1]) + 1, 2))       # one row beyond the last view
    c.proj = np.zeros((S, C, 3, 4))
    c.views = np.full((cap, C), I32_MIN, np.int32)
    c.ext_cost = np.full((cap, n_ext), np.nan, np.float32)
    c.X = np.full((cap, 3), np.nan)
    c.truth = np.full((cap, 3), np.nan)
    c.kind = np.full(cap, "", dtype=object)
    c.gross = np.zeros((cap, C), bool)                                    # the grossly shifted views
    for s in range(S):
        n, mo = int(counts[s]), int(c.match_offs[s])
        assert n <= caps[s]
        Ks, RTs = make_rig(rng, C)
        P = projection_matrices(np.stack(Ks)[None], np.stack(RTs)[None])[0]
        if tie:
            P[4] = P[3]
        c.proj[s] = P
        Xw = np.stack([rng.uniform(-120, 120, n), rng.uniform(-120, 120, n), rng.uniform(-60, 60, n)], 1)
        h = np.einsum("cij,nj->cni", P, np.concatenate([Xw, np.ones((n, 1))], 1))
        uv = h[..., :2] / h[..., 2:3]                                     # exact projections [C, n, 2]
        co = c.cam_offs[C * s:C * s + C + 1]
        rows = slice(mo, mo + n)
        c.truth[rows] = Xw
        for w in range(n):
            kind = kinds[w % len(kinds)]
            if n_ext < 2 and kind in ("two", "masking"):
                kind = "one"
            ext = list(range(3, C))
            shift = {d: _offset(rng, 0.05, 0.45) for d in ext}
            pick = [int(d) for d in rng.permutation(ext)]
            if tie and kind in ("one", "masking") and pick[0] == 4:
                pick[0] = 3                       # the tied pair, not its upper half alone
            gross = {"none": [], "one": pick[:1], "two": pick[:2], "all": ext, "masking": pick[:1]}[kind]
            size = {"one": [(30, 30)], "two": [(40, 40), (80, 80)], "all": [(25, 80)] * n_ext,
                    "masking": [(60, 100)]}.get(kind, [])
            for d, (lo, hi) in zip(gross, size):
                shift[d] = _offset(rng, lo, hi)
                c.gross[mo + w, d] = True
            for d in ext:
                uv[d, w] += shift[d]
            c.kind[mo + w] = kind
        if tie:
            uv[4] = uv[3]
            c.gross[rows, 4] = c.gross[rows, 3]
        keep = rng.random((n, C)) >= unkept
        keep[:, :3] = True
        keep |= c.gross[rows]                      # a gross view is a kept one
        if tie:
            keep[:, 4] = keep[:, 3]
        for cam in range(C):
            if nv[s, cam] == 0:
                keep[:, cam] = False
                c.gross[rows, cam] = False
                c.views[rows, cam] = -1
                continue
            perm = rng.permutation(int(nv[s, cam]))[:n]
            c.pts[co[cam] + perm] = uv[cam]
            c.views[rows, cam] = np.where(keep[:, cam], perm, -1)
        c.ext_cost[rows] = np.where(keep[:, 3:], rng.uniform(0, 30, (n, n_ext)), np.inf)
    for s in nan_view:
        c.proj[s, C - 1, 0] = 0.0
        c.proj[s, C - 1, 2] = 0.0
    for s in inf_view:
        c.proj[s, C - 1, 2] = 0.0
    for s, w in bad_seed_rows:
        row = int(c.match_offs[s]) + w
        c.views[row, 1] = nv[s, 1]
        c.kind[row] = "skip"
    for s, w in bad_extra_rows:
        row = int(c.match_offs[s]) + w
        c.views[row, C - 1] = nv[s, C - 1]
        c.kind[row] = "skip"
    # X as the extension leaves it: the DLT over the kept views (a skipped row: what it came with)
    for s in range(S):
        co = c.cam_offs[C * s:C * s + C + 1]
        for row in range(int(c.match_offs[s]), int(c.match_offs[s]) + int(counts[s])):
            v = c.views[row]
            if c.kind[row] == "skip":
                c.X[row] = c.truth[row]
                continue
            K = [d for d in range(C) if v[d] >= 0]
            c.X[row] = OP.triangulate(c.proj[s, K][None], np.stack([c.pts[co[d] + v[d]] for d in K])[None])[0]
    return c


# per-capture counts at the wave's edges, and count == capacity (captures 1, 3 and 6)
COUNTS = (0, 1, 63, 64, 65, 257, 7)
CAPS = (5, 1, 64, 64, 70, 300, 7)


@functools.lru_cache(maxsize=None)
def case(name, C):
    """The named inputs of tests/test_view_prune_gpu.py (seeds chosen so that
    tests/test_view_prune_model.py's margins hold)."""
    if name == "counts":        # the wave's edges; an empty extra view; a seed / an extra index out of range
        return build(C, COUNTS, CAPS, 100 + C, empty_view=(4,), bad_seed_rows=((2, 5), (5, 256)),
                     bad_extra_rows=((3, 63),))
    if name.startswith("captures"):     # 1, 4, 5 and 1,025 captures of 0-3 matches
        S = int(name[len("captures"):])
        rng = np.random.default_rng(S)
        return build(C, rng.integers(1 if S < 8 else 0, 4, S), [3] * S, 200 + S + C)
    if name == "nan":           # a P without its third row in camera C-1: NaN (capture 0), inf (capture 1)
        return build(C, (12, 12, 5), (12, 14, 5), 300 + C, nan_view=(0,), inf_view=(1,), unkept=0.0)
    if name == "tie":           # camera 4 = camera 3
        return build(C, (15, 4), (16, 4), 400 + C, tie=True, unkept=0.0)
    raise KeyError(name)


# (name, C) of every input the GPU test runs; "tie" needs two extra cameras
CASES = tuple([("counts", C) for C in (4, 5, 8)] + [(f"captures{S}", C) for S in (1, 4, 5, 1025) for C in (4, 8)]
              + [("nan", C) for C in (4, 5)] + [("tie", C) for C in (5, 8)])


@functools.lru_cache(maxsize=None)
def expected(name, C, gate):
    """``prune`` of ``case(name, C)`` under ``gate``, computed once."""
    return prune(*case(name, C).args(), gate)


def shift_extra_boxes(f, seed, share=0.4, lo=6.0, hi=12.0):
    """A copy of a tests/test_extend_gpu.py fixture's boxes with ``share`` of
    the extra views' detections moved by a whole-pixel offset of length in
    [lo, hi] (the centroid of an integer box moves by exactly that)."""
    rng = np.random.default_rng(seed)
    boxes = f.boxes.copy()
    for s in range(f.S):
        for cam in range(3, f.C):
            a, b = int(f.img_offs[f.C * s + cam]), int(f.img_offs[f.C * s + cam + 1])
            for k in range(a, b):
                if rng.random() < share:
                    while True:
                        d = rng.integers(-12, 13, 2)
                        if lo <= np.hypot(*d) <= hi:
                            break
                    boxes[k] += np.array([d[0], d[1], d[0], d[1]], np.float32)
    return boxes
