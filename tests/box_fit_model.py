"""The translation of a pose fitted to the detected boxes, given the model
(mvm_fit_boxes): the normative statement in plain fp64.  A
helper, not a test.

``fit_row`` is the definition.  It is written in Python floats (IEEE doubles):
every product, sum, division and square root below is one rounded operation, in
the order it stands -- CPython fuses nothing -- so the kernel, which is built
with contraction off, must return its bits.  The step and the loop are
tests/refine_model.py's (``solve``, ``inverse``, the constants), with t for X.
A NaN's sign and payload are not part of the statement (``same``).
"""
import math

import numpy as np

from refine_model import (CAPPED, CONVERGED, FACTOR, FAILED, LAMBDA0, LAMBDA_MIN, SKIPPED, STEP_TOL, _div, _finite,
                          _note, bits, inverse, same, solve)

__all__ = ["evaluate", "fit_row", "fit_trace", "fit_boxes", "same", "bits", "CONVERGED", "CAPPED", "FAILED",
           "SKIPPED"]

I32_MIN = np.iinfo(np.int32).min
NAN = float("nan")
INF = math.inf
TRACE_KEYS = ("evals", "accepted", "rejections", "invalid_trials")


def extremes(p, R, verts, t):
    """One view at t: p the row-major 3 x 4 (12 floats), R row-major 3 x 3 (9),
    verts a list of (x, y, z).
    -> ([(umin, h2), (vmin, h2), (umax, h2), (vmax, h2)], invalid): each
    extreme with the depth of its vertex, strict '<' / '>' in ascending vertex
    order (an exact tie keeps the lowest vertex; a NaN is never taken), from
    (+-inf, NaN); invalid where some vertex's h2 is not > 0."""
    M = [[(p[4 * q] * R[j] + p[4 * q + 1] * R[3 + j]) + p[4 * q + 2] * R[6 + j] for j in range(3)] for q in range(3)]
    c = [((p[4 * q] * t[0] + p[4 * q + 1] * t[1]) + p[4 * q + 2] * t[2]) + p[4 * q + 3] for q in range(3)]
    umin, vmin, umax, vmax = [INF, NAN], [INF, NAN], [-INF, NAN], [-INF, NAN]
    invalid = False
    for x, y, z in verts:
        h0 = ((M[0][0] * x + M[0][1] * y) + M[0][2] * z) + c[0]
        h1 = ((M[1][0] * x + M[1][1] * y) + M[1][2] * z) + c[1]
        h2 = ((M[2][0] * x + M[2][1] * y) + M[2][2] * z) + c[2]
        if not h2 > 0.0:
            invalid = True
        u = _div(h0, h2)
        v = _div(h1, h2)
        if u < umin[0]:
            umin = [u, h2]
        if v < vmin[0]:
            vmin = [v, h2]
        if u > umax[0]:
            umax = [u, h2]
        if v > vmax[0]:
            vmax = [v, h2]
    return [umin, vmin, umax, vmax], invalid


def evaluate(P, R, boxes, verts, t):
    """cost, A, g and the residuals at t over the kept views, ascending: P a
    list of 12-float rows, boxes of (x1, y1, x2, y2) floats.
    -> (cost, A = [A00, A01, A02, A11, A12, A22], g [3], resid [[4] per view]).
    An invalid view makes the cost +inf; A, g and resid are what they are."""
    cost = 0.0
    A = [0.0] * 6
    g = [0.0] * 3
    resid = []
    invalid = False
    for p, box in zip(P, boxes):
        ext, bad = extremes(p, R, verts, t)
        invalid = invalid or bad
        r = [ext[e][0] - box[e] for e in range(4)]
        resid.append(r)
        for e in range(4):
            cost = cost + r[e] * r[e]
            pe, h2 = ext[e]
            q = 4 * (e & 1)                      # a u edge reads P's row 0, a v edge row 1
            a = [_div(p[q + j] - pe * p[8 + j], h2) for j in range(3)]
            k = 0
            for j in range(3):
                for m in range(j, 3):
                    A[k] = A[k] + a[j] * a[m]
                    k += 1
            for j in range(3):
                g[j] = g[j] + a[j] * r[e]
    if invalid:
        cost = INF
    return cost, A, g, resid


def fit_row(P, R, boxes, verts, t0, max_evals, trace=None):
    """The definition for one row that is not skipped.
    -> (t_out [3], rms [2], status, evals, cov [6], resid [[4] per kept view]).
    ``trace``: a dict that receives what the descent did; it takes no part in
    any value returned."""
    t_in = [float(x) for x in t0]
    t = list(t_in)
    n4 = 4.0 * float(len(P))
    cost0, A, g, _ = evaluate(P, R, boxes, verts, t)
    c = cost0
    lam, evals, status = LAMBDA0, 0, None
    if trace is not None:
        trace.update(dict.fromkeys(TRACE_KEYS, 0), failed_at=None)
    if not _finite(c):
        status = FAILED
        _note(trace, "failed_at", "start")
    while status is None:
        if not _finite(*A, *g):
            status = FAILED
            _note(trace, "failed_at", "sums")
            break
        while True:
            d = solve(A, g, lam)
            if d is None or not _finite(*d):
                status = FAILED
                _note(trace, "failed_at", "pivot" if d is None else "step")
                break
            if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= STEP_TOL * ((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]):
                status = CONVERGED
                break
            if evals == max_evals:
                status = CAPPED
                break
            evals += 1
            y = [t[0] + d[0], t[1] + d[1], t[2] + d[2]]
            c1, A1, g1, _ = evaluate(P, R, boxes, verts, y)
            if c1 < c:
                t, c, A, g = y, c1, A1, g1
                lam = max(lam / FACTOR, LAMBDA_MIN)
                if trace is not None:
                    trace["accepted"] += 1
                break
            if trace is not None:
                trace["rejections"] += 1
                trace["invalid_trials"] += c1 == INF
            lam = lam * FACTOR
    if status == FAILED:
        t, c = t_in, cost0
    _note(trace, "evals", evals)
    rms = [math.sqrt(cost0 / n4), math.sqrt(c / n4)]
    _, A, _, resid = evaluate(P, R, boxes, verts, t)
    return t, rms, status, evals, inverse(A), resid


def fit_trace(P, R, boxes, verts, t0, max_evals):
    """``fit_row`` and what its descent did -> (its result, trace)."""
    trace = {}
    return fit_row(P, R, boxes, verts, t0, max_evals, trace), trace


def fit_boxes(pose, scene, views, boxes, proj, verts, max_evals=10, scene_base=0, fill=None, traces=None):
    """The op over rows: pose f64 [n, 4, 4], scene int32 [n], views int32
    [n, C], boxes int32 [n, C, 4], proj f64 [S, C, 3, 4], verts f64 [V, 3].
    ``fill``: what the outputs hold before the call, a dict of arrays, copied
    (default NaN / INT32_MIN); ``traces`` receives {row: trace}.
    -> dict(pose, rms [n, 2], info int32 [n, 2], cov [n, 6], resid [n, C, 4])."""
    n, C = views.shape
    S = proj.shape[0]
    if fill is None:
        fill = dict(pose=np.full((n, 4, 4), np.nan), rms=np.full((n, 2), np.nan),
                    info=np.full((n, 2), I32_MIN, np.int32), cov=np.full((n, 6), np.nan),
                    resid=np.full((n, C, 4), np.nan))
    out = {k: np.array(v, copy=True) for k, v in fill.items()}
    proj = np.asarray(proj, np.float64).reshape(S, C, 12)
    vl = np.asarray(verts, np.float64).reshape(-1, 3).tolist()
    for w in range(n):
        out["pose"][w] = pose[w]
        s = int(scene[w]) - scene_base
        K = [d for d in range(C) if views[w][d] >= 0]
        out["resid"][w] = np.nan
        if not 0 <= s < S or not K:
            out["rms"][w], out["info"][w], out["cov"][w] = np.nan, (SKIPPED, 0), np.nan
            continue
        P = [proj[s, d].tolist() for d in K]
        bx = [[float(b) for b in boxes[w][d]] for d in K]
        R = pose[w][:3, :3].reshape(9).tolist()
        trace = None if traces is None else traces.setdefault(w, {})
        t, rms, status, evals, cov, resid = fit_row(P, R, bx, vl, pose[w][:3, 3].tolist(), max_evals, trace)
        out["pose"][w][:3, 3] = t
        out["rms"][w], out["info"][w], out["cov"][w] = rms, (status, evals), cov
        for d, r in zip(K, resid):
            out["resid"][w][d] = r
    return out
