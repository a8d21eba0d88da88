"""Refinement of triangulated points by reprojection error, with covariance
(mvm_refine_points): the normative statement in plain fp64, and
the inputs the CPU and GPU tests share.  A helper, not a test.

``refine_row`` is the definition.  It is written in Python floats (IEEE
doubles): every product, sum, division and square root below is one rounded
operation, in the order it stands -- CPython fuses nothing -- so the kernel,
which is built with contraction off, must return its bits.  ``_div`` is IEEE
division where Python raises (a zero divisor).  A NaN's sign and payload are
not part of the statement: NaN compares equal to NaN (``same``).

The builders make ``synth.make_rig`` rigs of C cameras and world points
projected exactly into every view; a row keeps a random subset of 2..C views,
its centroids get 0-2 px of noise and are rounded to half-integers ("noisy"),
or stay exact ("exact").  X arrives as the DLT over the kept views
(``oracle.pipeline.triangulate``).
"""
import functools
import math

import numpy as np

from bpc_baseline_amd.inference.utils.camera_utils import projection_matrices
from bpc_baseline_amd.synth import make_rig
from oracle import pipeline as OP

I32_MIN = np.iinfo(np.int32).min
LAMBDA0 = 1e-3          # the first damping
LAMBDA_MIN = 1e-15      # its floor
FACTOR = 10.0           # down on an accepted step, up on a rejected one
STEP_TOL = 1e-20        # converged: d.d <= STEP_TOL (X.X)
CONVERGED, CAPPED, FAILED, SKIPPED = 0, 1, 2, 3
NAN = float("nan")


def _note(trace, key, value):
    """Record ``value`` under ``key`` where a trace is kept (refine_trace) -> None."""
    if trace is not None:
        trace[key] = value


def _div(a, b):
    """IEEE a / b."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _project(p, X):
    """(u, v, h2) of X under the row-major 3x4 ``p`` (12 floats)."""
    h0 = ((p[0] * X[0] + p[1] * X[1]) + p[2] * X[2]) + p[3]
    h1 = ((p[4] * X[0] + p[5] * X[1]) + p[6] * X[2]) + p[7]
    h2 = ((p[8] * X[0] + p[9] * X[1]) + p[10] * X[2]) + p[11]
    return _div(h0, h2), _div(h1, h2), h2


def cost(P, cent, X):
    """The summed squared reprojection error of X over the kept views, in
    their (ascending camera) order: P a list of 12-float rows, cent of (cx, cy)."""
    c = 0.0
    for p, (cx, cy) in zip(P, cent):
        u, v, _ = _project(p, X)
        ru = u - cx
        rv = v - cy
        c = c + (ru * ru + rv * rv)
    return c


def normal_equations(P, cent, X):
    """-> (A = [A00, A01, A02, A11, A12, A22], g = [g0, g1, g2]) at X."""
    A = [0.0] * 6
    g = [0.0] * 3
    for p, (cx, cy) in zip(P, cent):
        u, v, h2 = _project(p, X)
        ru = u - cx
        rv = v - cy
        a = [_div(p[j] - u * p[8 + j], h2) for j in range(3)]
        b = [_div(p[4 + j] - v * p[8 + j], h2) for j in range(3)]
        q = 0
        for j in range(3):
            for k in range(j, 3):
                A[q] = A[q] + (a[j] * a[k] + b[j] * b[k])
                q += 1
        for j in range(3):
            g[j] = g[j] + (a[j] * ru + b[j] * rv)
    return A, g


def ldlt(M, trace=None):
    """M = L D L^T of the symmetric [M00, M01, M02, M11, M12, M22] in this
    order -> (d0, d1, d2, l10, l20, l21), or None at the first pivot that is
    not > 0 (a NaN is not); ``trace["pivot"]`` then names it (0, 1, 2)."""
    M00, M01, M02, M11, M12, M22 = M
    d0 = M00
    if not d0 > 0.0:
        return _note(trace, "pivot", 0)
    l10 = M01 / d0
    l20 = M02 / d0
    d1 = M11 - l10 * M01
    if not d1 > 0.0:
        return _note(trace, "pivot", 1)
    t = M12 - l20 * M01
    l21 = t / d1
    d2 = (M22 - l20 * M02) - l21 * t
    if not d2 > 0.0:
        return _note(trace, "pivot", 2)
    return d0, d1, d2, l10, l20, l21


def solve(A, g, lam, trace=None):
    """delta of (A + lam diag A) delta = -g, or None where a pivot fails."""
    M = list(A)
    M[0] = A[0] + lam * A[0]
    M[3] = A[3] + lam * A[3]
    M[5] = A[5] + lam * A[5]
    f = ldlt(M, trace)
    if f is None:
        return None
    d0, d1, d2, l10, l20, l21 = f
    y0 = -g[0]
    y1 = -g[1] - l10 * y0
    y2 = (-g[2] - l20 * y0) - l21 * y1
    z0 = y0 / d0
    z1 = y1 / d1
    z2 = y2 / d2
    x2 = z2
    x1 = z1 - l21 * x2
    x0 = (z0 - l10 * x1) - l20 * x2
    return [x0, x1, x2]


def inverse(A):
    """The upper triangle, row-major, of A^-1 from the same factorisation
    (A^-1 = L^-T D^-1 L^-1), or six NaN where a pivot fails."""
    f = ldlt(A)
    if f is None:
        return [NAN] * 6
    d0, d1, d2, l10, l20, l21 = f
    i0 = 1.0 / d0
    i1 = 1.0 / d1
    i2 = 1.0 / d2
    m20 = l10 * l21 - l20            # L^-1's entry (2, 0)
    q2 = l21 * i2
    p1 = l10 * i1
    r2 = m20 * i2
    c00 = (i0 + l10 * p1) + m20 * r2
    c01 = -p1 - m20 * q2
    c02 = r2
    c11 = i1 + l21 * q2
    c12 = -q2
    c22 = i2
    return [c00, c01, c02, c11, c12, c22]


def _finite(*vals):
    return all(math.isfinite(x) for x in vals)


TRACE_KEYS = ("evals", "accepted", "rejections", "longest_run", "ties", "nan_trials", "inf_trials", "floor_steps",
              "xx_zero")


def refine_row(P, cent, X, max_evals, trace=None):
    """The definition for one row that is not skipped: P / cent of its kept
    views in ascending camera order, X its start.
    -> (X_out [3], rms [2], status, evals, cov [6]).
    ``trace``: a dict that receives what the descent did (``refine_trace``);
    it takes no part in any value returned."""
    X_in = [float(x) for x in X]
    X = list(X_in)
    n = float(len(P))
    cost0 = c = cost(P, cent, X)
    lam, evals, status = LAMBDA0, 0, None
    t = trace
    run = 0                                  # the rejections since the last accepted step (traced only)
    if t is not None:
        t.update(dict.fromkeys(TRACE_KEYS, 0), pivot=None, failed_at=None, failed_after_accept=False,
                 capped_in_run=False)
    if not _finite(c):
        status = FAILED
        _note(t, "failed_at", "start")
    while status is None:
        A, g = normal_equations(P, cent, X)
        if not _finite(*A, *g):
            status = FAILED
            _note(t, "failed_at", "sums")
            break
        while True:
            d = solve(A, g, lam, t)
            if d is None or not _finite(*d):
                status = FAILED
                _note(t, "failed_at", "pivot" if d is None else "step")
                break
            if t is not None and (X[0] * X[0] + X[1] * X[1]) + X[2] * X[2] == 0.0:
                t["xx_zero"] += 1
            if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= STEP_TOL * ((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2]):
                status = CONVERGED
                break
            if evals == max_evals:
                status = CAPPED
                _note(t, "capped_in_run", run > 0)
                break
            evals += 1
            Y = [X[0] + d[0], X[1] + d[1], X[2] + d[2]]
            c1 = cost(P, cent, Y)
            if t is not None:
                t["floor_steps"] += lam == LAMBDA_MIN
            if c1 < c:
                X, c = Y, c1
                lam = max(lam / FACTOR, LAMBDA_MIN)
                if t is not None:
                    t["accepted"] += 1
                    run = 0
                break
            if t is not None:
                run += 1
                t["rejections"] += 1
                t["longest_run"] = max(t["longest_run"], run)
                t["ties"] += c1 == c
                t["nan_trials"] += c1 != c1
                t["inf_trials"] += c1 == math.inf
            lam = lam * FACTOR
    if status == FAILED:
        _note(t, "failed_after_accept", t is not None and t["accepted"] > 0)
        X, c = X_in, cost0
    _note(t, "evals", evals)
    rms = [math.sqrt(cost0 / n), math.sqrt(c / n)]
    cov = inverse(normal_equations(P, cent, X)[0])
    return X, rms, status, evals, cov


def refine_trace(P, cent, X, max_evals):
    """``refine_row`` and what its descent did -> (its result, trace):
    ``evals``, ``accepted``, ``rejections`` and the ``longest_run`` of them,
    rejections whose trial cost equals the current one (``ties``), is NaN
    (``nan_trials``) or +inf (``inf_trials``), evaluations whose damping is
    the floor (``floor_steps``), convergence tests with X.X = 0 (``xx_zero``),
    ``failed_at`` ("start", "sums", "pivot", "step" or None) with the
    ``pivot`` that failed (0, 1, 2), ``failed_after_accept`` and
    ``capped_in_run`` (the cap met after a rejection)."""
    trace = {}
    return refine_row(P, cent, X, max_evals, trace), trace


def refine(views, X, match_offs, count, pts, cam_offs, proj, max_evals=10, fill=None, traces=None):
    """The op over a batch.  ``fill``: what the outputs hold before the call,
    (X_out, rms, info, cov) arrays, copied (default: NaN / INT32_MIN).
    ``traces``: a dict that receives {row: trace} of the rows not skipped.
    -> (X_out f64 [cap, 3], rms f64 [cap, 2], info int32 [cap, 2], cov f64 [cap, 6])."""
    cap, C = views.shape
    if fill is None:
        fill = (np.full((cap, 3), np.nan), np.full((cap, 2), np.nan), np.full((cap, 2), I32_MIN, np.int32),
                np.full((cap, 6), np.nan))
    X_out, rms, info, cov = (a.copy() for a in fill)
    proj = proj.reshape(-1, C, 12)
    for s in range(count.size):
        mo = int(match_offs[s])
        co = cam_offs[C * s:C * s + C + 1]
        for w in range(min(int(count[s]), int(match_offs[s + 1]) - mo)):
            row = mo + w
            v = views[row]
            K = [d for d in range(C) if v[d] >= 0]
            if len(K) < 2 or any(v[d] >= co[d + 1] - co[d] for d in K):
                X_out[row], rms[row], info[row], cov[row] = X[row], np.nan, (SKIPPED, 0), np.nan
                continue
            P = [proj[s, d].tolist() for d in K]
            cent = [pts[co[d] + v[d]].tolist() for d in K]
            trace = None if traces is None else traces.setdefault(row, {})
            x, r, status, evals, cv = refine_row(P, cent, X[row], max_evals, trace)
            X_out[row], rms[row], info[row], cov[row] = x, r, (status, evals), cv
    return X_out, rms, info, cov


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same(got, want):
    """Bit for bit, a NaN standing for any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    n = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), n) and np.array_equal(bits(got)[~n], bits(want)[~n]))


# ------------------------------------------------------------- inputs ----
class Case:
    """One input of the op: host arrays in the op's argument order (``args``),
    the true world point (NaN outside the captures' rows) and the kind of
    every row ("" outside)."""
    FIELDS = ("views", "X", "match_offs", "count", "pts", "cam_offs", "proj")

    def args(self):
        return tuple(getattr(self, k) for k in self.FIELDS)

    def rows(self):
        """The rows of the captures' matches."""
        return np.concatenate([np.arange(o, o + n) for o, n in zip(self.match_offs[:-1], self.count)]
                              + [np.zeros(0, np.int64)]).astype(np.int64)


def build(C, counts, caps, seed, *, exact_every=5, full_views=False, zero_row3=(), zero_cols=(),
          bad_rows=(), single_rows=(), noise=2.0):
    """``counts[s]`` matches in a segment of ``caps[s]`` rows per capture.
    Row w keeps a random subset of 2..C views (``full_views``: all); every
    ``exact_every``-th row is "exact", the others "noisy" with ``noise`` px.
    ``zero_row3``: captures whose camera 0 has a P with a zero third row
    ("zero3": the cost is not finite); ``zero_cols``: captures whose every P
    has its first three columns zero ("azero": A = 0); both keep all views.
    ``bad_rows``: (capture, w) whose highest kept camera's index is its view's
    size, ``single_rows``: that keep one view only (both "skip").  Rows
    outside the captures' hold sentinels (views INT32_MIN, X NaN)."""
    rng = np.random.default_rng(seed)
    counts, caps = np.asarray(counts, np.int32), np.asarray(caps, np.int64)
    S = counts.size
    c = Case()
    c.C, c.S, c.count = C, S, counts
    c.match_offs = np.zeros(S + 1, np.int64)
    np.cumsum(caps, out=c.match_offs[1:])
    cap = int(c.match_offs[-1])
    nv = np.repeat(counts.astype(np.int64)[:, None] + 2, C, axis=1)      # two clutter detections a view
    c.cam_offs = np.zeros(S * C + 1, np.int64)
    np.cumsum(nv.reshape(-1), out=c.cam_offs[1:])
    c.pts = rng.uniform(0.0, 2400.0, (int(c.cam_offs[-1]) + 1, 2))        # one row beyond the last view
    c.proj = np.zeros((S, C, 3, 4))
    c.views = np.full((cap, C), I32_MIN, np.int32)
    c.X = np.full((cap, 3), np.nan)
    c.truth = np.full((cap, 3), np.nan)
    c.kind = np.full(cap, "", dtype=object)
    for s in range(S):
        n, mo = int(counts[s]), int(c.match_offs[s])
        assert n <= caps[s]
        Ks, RTs = make_rig(rng, C)
        P = projection_matrices(np.stack(Ks)[None], np.stack(RTs)[None])[0]
        c.proj[s] = P
        Xw = np.stack([rng.uniform(-120, 120, n), rng.uniform(-120, 120, n), rng.uniform(-60, 60, n)], 1)
        h = np.einsum("cij,nj->cni", P, np.concatenate([Xw, np.ones((n, 1))], 1))
        uv = h[..., :2] / h[..., 2:3]                                     # exact projections [C, n, 2]
        co = c.cam_offs[C * s:C * s + C + 1]
        rows = slice(mo, mo + n)
        c.truth[rows] = Xw
        special = s in zero_row3 or s in zero_cols
        keep = np.zeros((n, C), bool)
        for w in range(n):
            exact = exact_every and w % exact_every == exact_every - 1
            c.kind[mo + w] = "zero3" if s in zero_row3 else "azero" if s in zero_cols else \
                "exact" if exact else "noisy"
            k = C if full_views or special else int(rng.integers(2, C + 1))
            keep[w, rng.permutation(C)[:k]] = True
            if not exact:
                a, m = rng.uniform(0, 2 * np.pi, C), rng.uniform(0, noise, C)
                uv[:, w] = np.round(2.0 * (uv[:, w] + np.stack([m * np.cos(a), m * np.sin(a)], 1))) / 2.0
        for s2, w in single_rows:
            if s2 == s:
                keep[w] = False
                keep[w, int(rng.integers(0, C))] = True
                c.kind[mo + w] = "skip"
        for cam in range(C):
            perm = rng.permutation(int(nv[s, cam]))[:n]
            c.pts[co[cam] + perm] = uv[cam]
            c.views[rows, cam] = np.where(keep[:, cam], perm, -1)
        for s2, w in bad_rows:
            if s2 == s:
                d = int(np.nonzero(keep[w])[0][-1])
                c.views[mo + w, d] = nv[s, d]
                c.kind[mo + w] = "skip"
        # X as the chain leaves it: the DLT over the kept views
        for w in range(n):
            v = c.views[mo + w]
            K = [d for d in range(C) if v[d] >= 0]
            if c.kind[mo + w] == "skip":
                c.X[mo + w] = Xw[w]
                continue
            c.X[mo + w] = OP.triangulate(P[K][None], np.stack([c.pts[co[d] + v[d]] for d in K])[None])[0]
    for s in zero_row3:
        c.proj[s, 0, 2] = 0.0
    for s in zero_cols:
        c.proj[s, :, :, :3] = 0.0
    return c


# per-capture counts at the wave's edges, an empty capture between full ones,
# and count == capacity (captures 0, 2, 3, 4 and 7)
COUNTS = (3, 0, 1, 63, 64, 65, 257, 7)
CAPS = (3, 5, 1, 64, 64, 70, 300, 7)
CAMS = (3, 4, 5, 8)
MAX_EVALS = (1, 2, 10, 64)


@functools.lru_cache(maxsize=None)
def case(name, C):
    """The named inputs of tests/test_refine_model.py and tests/test_refine_gpu.py."""
    if name == "counts":        # the wave's edges
        return build(C, COUNTS, CAPS, 1700 + C)
    if name.startswith("captures"):     # 1, 4, 5 and 1,025 captures of 0-3 matches
        S = int(name[len("captures"):])
        rng = np.random.default_rng(S)
        return build(C, rng.integers(1 if S < 8 else 0, 4, S), [3] * S, 1800 + S + C)
    if name == "regimes":       # zero third row (capture 0), A = 0 (capture 1), skipped rows (capture 2)
        return build(C, (4, 4, 12), (4, 6, 12), 1900 + C, zero_row3=(0,), zero_cols=(1,),
                     bad_rows=((2, 1), (2, 6), (2, 10)), single_rows=((2, 0), (2, 3), (2, 8)))
    if name == "truth":         # 600 rigs, one noisy point each over all its views (the mean distance to the truth)
        return build(C, (1,) * 600, (1,) * 600, 2000 + C, exact_every=0, full_views=True)
    import refine_edges                 # where the descent rejects, stalls and fails (imports this module)
    if name in refine_edges.NAMES:
        return refine_edges.build(name, C)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, C, max_evals=10):
    """``refine`` of ``case(name, C)``, computed once."""
    return refine(*case(name, C).args(), max_evals)
