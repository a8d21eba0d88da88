"""Poses against ground truth restated in numpy -- the normative
statement of what mvm_score_poses and mvm_match_scores compute; the kernels
return these bits.

Everything is float64, and every product, sum, difference and square root below
is one rounded operation in the order written (numpy fuses nothing).

Pair errors.  Row r of the range with s = scene[r] - scene_base, column
g < Gmax = max(1, the largest ground-truth count); each rule applies only where
the one before did not:

  1. s is no capture of gt_offs: err = t_err = +inf, rot_cos = NaN, sym = -2.
  2. g >= g_s (padding): the same with sym = -1.
  3. one of the 12 read entries of the estimate or of the ground-truth pose is
     not below 2^200 in magnitude (a NaN is not): the same with sym = -3.
  4. otherwise, with (Rp, tp) the estimate, (Rg, tg) the ground truth, (Sk, sk)
     symmetry k:
       M[i][j] = (Rg[i][0] Sk[0][j] + Rg[i][1] Sk[1][j]) + Rg[i][2] Sk[2][j]
       A[i][j] = Rp[i][j] - M[i][j]
       u[i]    = ((Rg[i][0] sk[0] + Rg[i][1] sk[1]) + Rg[i][2] sk[2]) + tg[i]
       b[i]    = tp[i] - u[i]
       d[i]    = ((A[i][0] v[0] + A[i][1] v[1]) + A[i][2] v[2]) + b[i]   per vertex v
       q       = (d[0] d[0] + d[1] d[1]) + d[2] d[2]
       m_k     = max_v q
     sym = the lowest k with the smallest m_k, err = sqrt(m_sym),
     t_err = sqrt((e0 e0 + e1 e1) + e2 e2) with e = tp - tg,
     rot_cos = (sum_ij Rp[i][j] M_sym[i][j] - 1) 0.5, row-major, left to right.

Under rule 3 and with vertices and symmetries below 2^200 too, every d is
finite and every q is in [+0, +inf] (a square may overflow; it is never a NaN),
so the maximum is exact and order-free.  This is the affine form of BOP's mssd,
min_k max_v |(Rp v + tp) - (Rg (Sk v + sk) + tg)|; ``mssd_direct`` states that
form.

Greedy matching.  Per threshold tau and capture s the capture's rows are walked
in table order; row r takes the not-yet-taken g < min(g_s, Gmax) with the
smallest err[r, g] among those with err[r, g] < tau (strict; the lowest g wins a
tie), or -1.  ``match_scores`` states it vectorised over (threshold, capture),
``match_scores_loop`` as a plain loop.
"""
import numpy as np

PADDING, NO_CAPTURE, NOT_FINITE = -1, -2, -3
POSE_MAX = 2.0 ** 200
MAX_SYMS, MAX_THRESHOLDS, MAX_MATCH_GT = 64, 16, 1024
KEYS = ("err", "sym", "t_err", "rot_cos")


def same(a, b):
    """Bit-equal up to the payload of a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all())


def g_max_of(gt_offs):
    d = np.diff(np.asarray(gt_offs, np.int64))
    return max(1, int(d.max())) if d.size else 1


def _affine(Rp, tp, Rg, tg, S):
    """(A [m, 3, 3], b [m, 3], dot [m]) of m pairs under one symmetry S [4, 4]."""
    m = len(Rp)
    A, b = np.empty((m, 3, 3)), np.empty((m, 3))
    dot = None
    for i in range(3):
        for j in range(3):
            M = (Rg[:, i, 0] * S[0, j] + Rg[:, i, 1] * S[1, j]) + Rg[:, i, 2] * S[2, j]
            A[:, i, j] = Rp[:, i, j] - M
            pm = Rp[:, i, j] * M
            dot = pm if dot is None else dot + pm
        u = ((Rg[:, i, 0] * S[0, 3] + Rg[:, i, 1] * S[1, 3]) + Rg[:, i, 2] * S[2, 3]) + tg[:, i]
        b[:, i] = tp[:, i] - u
    return A, b, dot


def _max_sq(A, b, verts, chunk=4096):
    """m_k [m]: the largest squared length of A v + b over the vertices."""
    m = np.zeros(len(A))
    for v0 in range(0, len(verts), chunk):
        v = verts[v0:v0 + chunk]
        d = [((A[:, i, 0, None] * v[None, :, 0] + A[:, i, 1, None] * v[None, :, 1])
              + A[:, i, 2, None] * v[None, :, 2]) + b[:, i, None] for i in range(3)]
        q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        m = np.maximum(m, q.max(axis=1))
    return m


def score_poses(pose, scene, gt_pose, gt_offs, verts, syms=None, rows=None, scene_base=0):
    """-> dict of err f64, sym int32, t_err f64, rot_cos f64, each [rows, Gmax]."""
    pose = np.asarray(pose, np.float64).reshape(-1, 4, 4)
    scene = np.asarray(scene, np.int32)
    gt_pose = np.asarray(gt_pose, np.float64).reshape(-1, 4, 4)
    gt_offs = np.asarray(gt_offs, np.int64)
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    syms = np.eye(4)[None] if syms is None else np.asarray(syms, np.float64).reshape(-1, 4, 4)
    assert len(verts) >= 1 and 1 <= len(syms) <= MAX_SYMS
    assert (np.abs(verts) < POSE_MAX).all() and (np.abs(syms[:, :3]) < POSE_MAX).all()
    b0, e0 = (0, len(scene)) if rows is None else rows
    S, G = len(gt_offs) - 1, g_max_of(gt_offs)
    n = e0 - b0
    err = np.full((n, G), np.inf)
    t_err = np.full((n, G), np.inf)
    rot_cos = np.full((n, G), np.nan)
    sym = np.empty((n, G), np.int32)
    s = scene[b0:e0].astype(np.int64) - int(scene_base)
    known = (s >= 0) & (s < S)
    sym[:] = np.where(known, PADDING, NO_CAPTURE)[:, None]
    sk = np.where(known, s, 0)
    count = np.where(known, gt_offs[sk + 1] - gt_offs[sk], 0)
    rr, gg = np.nonzero(np.arange(G)[None, :] < count[:, None])
    if len(rr) == 0:
        return dict(err=err, sym=sym, t_err=t_err, rot_cos=rot_cos)
    P, Q = pose[b0 + rr], gt_pose[gt_offs[sk[rr]] + gg]
    with np.errstate(invalid="ignore"):
        sane = ((np.abs(P[:, :3]) < POSE_MAX).all(axis=(1, 2)) & (np.abs(Q[:, :3]) < POSE_MAX).all(axis=(1, 2)))
    sym[rr[~sane], gg[~sane]] = NOT_FINITE
    rr, gg, P, Q = rr[sane], gg[sane], P[sane], Q[sane]
    if len(rr) == 0:
        return dict(err=err, sym=sym, t_err=t_err, rot_cos=rot_cos)
    Rp, tp, Rg, tg = P[:, :3, :3], P[:, :3, 3], Q[:, :3, :3], Q[:, :3, 3]
    best = best_dot = best_k = None
    with np.errstate(over="ignore"):
        for k, Sk in enumerate(syms):
            A, b, dot = _affine(Rp, tp, Rg, tg, Sk)
            mk = _max_sq(A, b, verts)
            if k == 0:
                best, best_dot, best_k = mk, dot, np.zeros(len(rr), np.int32)
            else:
                lower = mk < best                   # strict: the lowest k keeps a tie
                best = np.where(lower, mk, best)
                best_dot = np.where(lower, dot, best_dot)
                best_k = np.where(lower, np.int32(k), best_k)
    e = tp - tg
    err[rr, gg] = np.sqrt(best)
    sym[rr, gg] = best_k
    t_err[rr, gg] = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    rot_cos[rr, gg] = (best_dot - 1.0) * 0.5
    return dict(err=err, sym=sym, t_err=t_err, rot_cos=rot_cos)


def mssd_direct(pose_p, pose_g, verts, syms=None):
    """BOP's mssd of one pair as it is written: both point sets transformed,
    the largest distance over the vertices, the smallest over the symmetries."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    syms = np.eye(4)[None] if syms is None else np.asarray(syms, np.float64).reshape(-1, 4, 4)
    est = verts @ pose_p[:3, :3].T + pose_p[:3, 3]
    out = np.inf
    for S in syms:
        gt = (verts @ S[:3, :3].T + S[:3, 3]) @ pose_g[:3, :3].T + pose_g[:3, 3]
        out = min(out, float(np.sqrt(((est - gt) ** 2).sum(axis=1)).max()))
    return out


def _ranges(row_offs, gt_offs, n, G):
    """Per capture (begin, end, ground-truth count), clamped as the kernel
    clamps them: offsets into 0 .. n, an end up to its begin, a count into 0 .. G."""
    row_offs, gt_offs = np.asarray(row_offs, np.int64), np.asarray(gt_offs, np.int64)
    assert len(row_offs) == len(gt_offs) and (np.diff(row_offs) >= 0).all()
    b = np.clip(row_offs[:-1], 0, n)
    e = np.maximum(np.clip(row_offs[1:], 0, n), b)
    return b, e, np.clip(np.diff(gt_offs), 0, G)


def match_scores_loop(err, row_offs, gt_offs, thresholds):
    """The greedy rule as a plain loop -> (gt_index int32 [T, n], tp int32 [T, S])."""
    err = np.asarray(err, np.float64)
    n, G = err.shape
    thresholds = np.asarray(thresholds, np.float64).reshape(-1)
    assert 1 <= len(thresholds) <= MAX_THRESHOLDS and 1 <= G <= MAX_MATCH_GT
    b, e, gs = _ranges(row_offs, gt_offs, n, G)
    gt_index = np.full((len(thresholds), n), -1, np.int32)
    tp = np.zeros((len(thresholds), len(b)), np.int32)
    for t, tau in enumerate(thresholds):
        for s in range(len(b)):
            taken = set()
            for r in range(int(b[s]), int(e[s])):
                pick = -1
                for g in range(int(gs[s])):
                    if g in taken or not err[r, g] < tau:
                        continue
                    if pick < 0 or err[r, g] < err[r, pick]:
                        pick = g
                if pick >= 0:
                    taken.add(pick)
                    gt_index[t, r] = pick
                    tp[t, s] += 1
    return gt_index, tp


def match_scores(err, row_offs, gt_offs, thresholds):
    """The same, every (threshold, capture) at once: step j takes the j-th row
    of every capture that has one."""
    err = np.asarray(err, np.float64)
    n, G = err.shape
    thresholds = np.asarray(thresholds, np.float64).reshape(-1)
    assert 1 <= len(thresholds) <= MAX_THRESHOLDS and 1 <= G <= MAX_MATCH_GT
    b, e, gs = _ranges(row_offs, gt_offs, n, G)
    T, S = len(thresholds), len(b)
    gt_index = np.full((T, n), -1, np.int32)
    tp = np.zeros((T, S), np.int32)
    free = np.broadcast_to(np.arange(G)[None, None, :] < gs[None, :, None], (T, S, G)).copy()
    for j in range(int((e - b).max()) if S else 0):
        live = np.nonzero(b + j < e)[0]
        rows = b[live] + j
        v = np.broadcast_to(err[rows][None], (T, len(live), G))
        with np.errstate(invalid="ignore"):
            ok = free[:, live] & (v < thresholds[:, None, None])
        key = np.where(ok, v, np.inf)
        pick = key.argmin(axis=2)                   # the first of equal minima: the lowest g
        hit = np.take_along_axis(ok, pick[..., None], axis=2)[..., 0]
        tt, ll = np.nonzero(hit)
        gt_index[tt, rows[ll]] = pick[tt, ll]
        free[tt, live[ll], pick[tt, ll]] = False
        tp[:, live] += hit
    return gt_index, tp


def recall_precision(tp, row_offs, gt_offs):
    """-> (recall f64 [T], precision f64 [T]) over the whole table: matched rows
    over ground-truth objects and over rows (NaN where there are none)."""
    tp = np.asarray(tp).sum(axis=1).astype(np.float64)
    n_gt = float(np.diff(np.asarray(gt_offs, np.int64)).sum())
    n_rows = float(np.diff(np.asarray(row_offs, np.int64)).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return tp / n_gt, tp / n_rows


# ---------------------------------------------------------------- inputs ----
def random_rotations(rng, n):
    """Uniform on SO(3): normalised Gaussian quaternions."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def random_poses(rng, n, t_max=1e3):
    P = np.zeros((n, 4, 4))
    P[:, :3, :3] = random_rotations(rng, n)
    P[:, :3, 3] = rng.uniform(-t_max, t_max, (n, 3))
    P[:, 3, 3] = 1.0
    return P


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    M = np.eye(4)
    M[:2, :2] = [[c, -s], [s, c]]
    return M


def z_symmetries(K):
    """K turns about z; the half turn is exact where K is even."""
    out = np.stack([rot_z(2 * np.pi * k / K) for k in range(K)])
    if K % 2 == 0:
        out[K // 2] = np.diag([-1.0, -1.0, 1.0, 1.0])
    out[0] = np.eye(4)
    return out
