"""From the rotation head's raw outputs to a pose per match (DESIGN §3.19,
mvm_fuse_rotations): the normative statement, and the inputs the CPU and GPU
tests share.  A helper, not a test.

``fuse_rotations`` is the definition.  It is written in numpy over all slots at
once: every product, sum, division and square root below is one rounded
operation on arrays of one type (float32 in ``decode``, float64 after it), in
the order it stands -- numpy fuses nothing -- so the kernel, which is built with
contraction off, must return its bits.  A NaN's sign and payload are not part
of the statement: NaN compares equal to NaN (``same``).

A slot is (table row r, selected camera c).  Its raw vector is decoded in
float32 as the reference decodes it (``decode``), taken to the world in float64
(``to_world``), and the usable slots of a row are fused (``fuse="cam"``: one
camera's; ``fuse="mean"``: the chordal mean, the largest eigenvector of Horn's
4 x 4 matrix by cyclic Jacobi rotations, ``mean_rotation``).
``mean_rotation_svd`` states the mean a second way for the CPU tests.
"""
import numpy as np

MODES = {"euler": (0, 3), "quat": (1, 4), "6d": (2, 6)}      # name -> (code, D)
FUSE = {"cam": 0, "mean": 1}
NO_VIEW, NO_CAPTURE, DEGENERATE = 1, 2, 4                     # slot status (0: usable)
NO_ROTATION, AMBIGUOUS = 1, 2                                 # row status bits
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))      # one Jacobi sweep
SWEEPS = 8
AMBIGUOUS_GAP = 1e-9                                          # lambda1 - lambda2 <= GAP * n_used
EULER_MARGIN = 2.0 ** -40                                     # euler_filter
# a world rotation with a non-finite entry, or one of this magnitude or more, is DEGENERATE: below it the sum of
# eight, Horn's combinations of three, the power step's four squares and the spread's nine all stay finite
WORLD_MAX = 2.0 ** 500

F1, F2, EPS32 = np.float32(1), np.float32(2), np.float32(1e-8)
PI32, TWO_PI32 = np.float32(np.pi), np.float32(2 * np.pi)


def same(a, b):
    """Bit equality of two arrays of one dtype and shape, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def _norm3(v0, v1, v2):
    return np.sqrt((v0 * v0 + v1 * v1) + v2 * v2)


def quat_matrix(x, y, z, w, one, two):
    """The nine entries of the reference's quat_to_rotmat, left to right, in
    the type of the arguments -> [..., 3, 3]."""
    m = [one - two * y * y - two * z * z, two * x * y - two * z * w, two * x * z + two * y * w,
         two * x * y + two * z * w, one - two * x * x - two * z * z, two * y * z - two * x * w,
         two * x * z - two * y * w, two * y * z + two * x * w, one - two * x * x - two * y * y]
    return np.stack(m, axis=-1).reshape(np.shape(x) + (3, 3))


def wrap_euler(a):
    """((a + pi) mod 2 pi) - pi in float32, the modulo floored (numpy's)."""
    a = np.asarray(a, np.float32)
    return np.mod(a + PI32, TWO_PI32) - PI32


def decode(raw, mode):
    """raw float32 [n, D] -> float32 [n, 3, 3], every operation in float32
    except the sine and cosine, which are the float64 ones rounded once."""
    raw = np.ascontiguousarray(raw, np.float32)
    assert raw.ndim == 2 and raw.shape[1] == MODES[mode][1]
    with np.errstate(all="ignore"):
        if mode == "quat":
            x, y, z, w = (raw[:, i] for i in range(4))
            n = np.sqrt(((x * x + y * y) + z * z) + w * w) + EPS32
            x, y, z, w = x / n, y / n, z / n, w / n
            n = np.sqrt(((x * x + y * y) + z * z) + w * w)
            x, y, z, w = x / n, y / n, z / n, w / n
            return quat_matrix(x, y, z, w, F1, F2)
        if mode == "6d":
            a1 = [raw[:, i] for i in range(3)]
            a2 = [raw[:, 3 + i] for i in range(3)]
            n = np.maximum(_norm3(*a1), EPS32)
            b1 = [v / n for v in a1]
            d = (b1[0] * a2[0] + b1[1] * a2[1]) + b1[2] * a2[2]
            tmp = [a2[i] - d * b1[i] for i in range(3)]
            n = np.maximum(_norm3(*tmp), EPS32)
            b2 = [v / n for v in tmp]
            b3 = [b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]]
            return np.stack([np.stack([b1[i], b2[i], b3[i]], axis=-1) for i in range(3)], axis=-2)
        a = wrap_euler(raw).astype(np.float64)
        s, c = np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)
        sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
        cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
        m = [cy * cz, -cy * sz, sy,
             sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy,
             -cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy]
        return np.stack(m, axis=-1).reshape(-1, 3, 3)


def to_world(R, M):
    """R f64 [n, 3, 3] (world -> camera), M float32 [n, 3, 3] -> W = R^T M in
    float64: W[i][j] = (R[0][i] M[0][j] + R[1][i] M[1][j]) + R[2][i] M[2][j]."""
    R = np.asarray(R, np.float64)
    M = np.asarray(M, np.float32).astype(np.float64)
    W = np.empty(M.shape, np.float64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                W[:, i, j] = (R[:, 0, i] * M[:, 0, j] + R[:, 1, i] * M[:, 1, j]) + R[:, 2, i] * M[:, 2, j]
    return W


def horn_matrix(A):
    """A f64 [n, 3, 3] -> the symmetric N [n, 4, 4] with q^T N q = sum_ij
    A[i][j] R(q)[i][j] for a unit quaternion q = (x, y, z, w)."""
    N = np.empty(A.shape[:1] + (4, 4), np.float64)
    a = lambda i, j: A[:, i, j]
    N[:, 0, 0] = (a(0, 0) - a(1, 1)) - a(2, 2)
    N[:, 1, 1] = (a(1, 1) - a(0, 0)) - a(2, 2)
    N[:, 2, 2] = (a(2, 2) - a(0, 0)) - a(1, 1)
    N[:, 3, 3] = (a(0, 0) + a(1, 1)) + a(2, 2)
    N[:, 0, 1] = a(0, 1) + a(1, 0)
    N[:, 0, 2] = a(0, 2) + a(2, 0)
    N[:, 0, 3] = a(2, 1) - a(1, 2)
    N[:, 1, 2] = a(1, 2) + a(2, 1)
    N[:, 1, 3] = a(0, 2) - a(2, 0)
    N[:, 2, 3] = a(1, 0) - a(0, 1)
    for p, q in PAIRS:
        N[:, q, p] = N[:, p, q]
    return N


def jacobi4(N):
    """Cyclic Jacobi on the upper triangle of N f64 [n, 4, 4]: SWEEPS sweeps of
    PAIRS; a pair whose off-diagonal entry is exactly 0 is skipped.
    -> (d [n, 4] the diagonal left, V [n, 4, 4] the accumulated rotations:
    column j belongs to d[j])."""
    n = N.shape[0]
    a = [[N[:, p, q].copy() for q in range(4)] for p in range(4)]        # a[p][q] used for p <= q
    v = [[np.full(n, 1.0 if p == q else 0.0) for q in range(4)] for p in range(4)]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                apq = a[p][q]
                skip = apq == 0.0
                theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                new = {(p, p): a[p][p] - h, (q, q): a[q][q] + h, (p, q): np.zeros(n)}
                for k in range(4):
                    if k in (p, q):
                        continue
                    kp, kq = (min(k, p), max(k, p)), (min(k, q), max(k, q))
                    akp, akq = a[kp[0]][kp[1]], a[kq[0]][kq[1]]
                    new[kp] = c * akp - s * akq
                    new[kq] = s * akp + c * akq
                for (i, j), val in new.items():
                    a[i][j] = np.where(skip, a[i][j], val)
                for k in range(4):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = np.where(skip, vkp, c * vkp - s * vkq)
                    v[k][q] = np.where(skip, vkq, s * vkp + c * vkq)
    d = np.stack([a[i][i] for i in range(4)], axis=-1)
    V = np.stack([np.stack(v[k], axis=-1) for k in range(4)], axis=-2)
    return d, V


def mean_rotation(W, used):
    """The chordal mean of the rotations W f64 [n, K, 3, 3] over the slots with
    ``used`` [n, K], summed in slot order -> (R f64 [n, 3, 3], lam f64 [n, 2]:
    the two largest eigenvalues of Horn's matrix): the eigenvector jacobi4
    gives for the largest eigenvalue, polished by one shifted power step,
    normalised, its sign fixed, through quat_matrix.  A row without a used slot
    gets the mean of nothing, which its caller overwrites."""
    W = np.asarray(W, np.float64)
    n, K = W.shape[:2]
    A = np.zeros((n, 3, 3))
    for k in range(K):
        A = np.where(used[:, k, None, None], A + W[:, k], A)
    d, V = jacobi4(horn_matrix(A))
    best = np.zeros(n, np.int64)
    lam1 = d[:, 0].copy()
    for j in range(1, 4):                                   # the lowest index wins a tie
        up = d[:, j] > lam1
        best, lam1 = np.where(up, j, best), np.where(up, d[:, j], lam1)
    lam2 = np.full(n, -np.inf)
    for j in range(4):
        up = (best != j) & (d[:, j] > lam2)
        lam2 = np.where(up, d[:, j], lam2)
    q = [np.take_along_axis(V[:, k, :], best[:, None], axis=1)[:, 0] for k in range(4)]
    with np.errstate(all="ignore"):
        # one shifted power step polishes the vector: tr N = 0, so -lam1 / 3 is
        # the mean of the other three eigenvalues; kept only where it has a length
        N = horn_matrix(A)
        third = lam1 / 3.0
        p = [(((N[:, i, 0] * q[0] + N[:, i, 1] * q[1]) + N[:, i, 2] * q[2]) + N[:, i, 3] * q[3]) + third * q[i]
             for i in range(4)]
        np_ = np.sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3])
        q = [np.where(np_ > 0.0, p[i], q[i]) for i in range(4)]
        nq = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        q = [v / nq for v in q]
        big, neg = np.abs(q[0]), q[0] < 0.0
        for k in range(1, 4):                               # the component of largest magnitude is positive
            up = np.abs(q[k]) > big
            big, neg = np.where(up, np.abs(q[k]), big), np.where(up, q[k] < 0.0, neg)
        q = [np.where(neg, -v, v) for v in q]
        R = quat_matrix(q[0], q[1], q[2], q[3], 1.0, 2.0)
    return R, np.stack([lam1, lam2], axis=-1)


def mean_rotation_svd(Ws):
    """The same mean of a list of 3 x 3 rotations, stated independently: the
    rotation nearest their sum (SVD with the determinant fix)."""
    U, _, Vt = np.linalg.svd(np.sum(np.asarray(Ws, np.float64), axis=0))
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def fuse_rotations(raw, scene, views, X, RTs, mode, rows=None, cams=None, fuse="cam", cam=2, scene_base=0):
    """The definition.  raw float32 [rows, cams, D]; scene int32 [n], views
    int32 [n, C] and X f64 [n, 3] a table's fields; RTs f64 [S, C, 4, 4].
    -> dict of rot_views f64 [rows, cams, 3, 3], R f64 [rows, 3, 3], pose f64
    [rows, 4, 4], spread f64 [rows, cams], slot_status int32 [rows, cams],
    row_status int32 [rows], lam f64 [rows, 2] (NaN unless fuse="mean")."""
    RTs = np.asarray(RTs, np.float64)
    S, C = RTs.shape[:2]
    n = len(scene)
    b, e = (0, n) if rows is None else rows
    cams = list(range(C)) if cams is None else list(cams)
    m, K, D = e - b, len(cams), MODES[mode][1]
    raw = np.asarray(raw, np.float32).reshape(m, K, D)
    if fuse == "cam" and cam not in cams:
        raise ValueError(f"cam={cam} is not among the selected cameras {cams}")
    sc = np.asarray(scene[b:e], np.int64) - scene_base
    in_range = (sc >= 0) & (sc < S)
    status = np.zeros((m, K), np.int32)
    W = np.full((m, K, 3, 3), np.nan)
    for k, c in enumerate(cams):
        st = np.where(~in_range, NO_CAPTURE, np.where(np.asarray(views)[b:e, c] < 0, NO_VIEW, 0)).astype(np.int32)
        M = decode(raw[:, k], mode)
        st = np.where((st == 0) & ~np.isfinite(M).all(axis=(1, 2)), DEGENERATE, st).astype(np.int32)
        Wk = to_world(RTs[np.where(in_range, sc, 0), c, :3, :3], M) if S else np.full((m, 3, 3), np.nan)
        # a NaN, an infinity or an absurd magnitude from the extrinsic rotation (a NaN fails the comparison)
        with np.errstate(invalid="ignore"):
            sane = (np.abs(Wk) < WORLD_MAX).all(axis=(1, 2))
        st = np.where((st == 0) & ~sane, DEGENERATE, st).astype(np.int32)
        W[:, k] = np.where((st == 0)[:, None, None], Wk, np.nan)
        status[:, k] = st
    used = status == 0
    lam = np.full((m, 2), np.nan)
    if fuse == "cam":
        k = cams.index(cam)
        R, ok = W[:, k].copy(), used[:, k]
        row_status = np.where(ok, 0, NO_ROTATION).astype(np.int32)
    else:
        R, lam = mean_rotation(np.where(used[:, :, None, None], W, 0.0), used)
        n_used = used.sum(axis=1)
        ok = n_used > 0
        row_status = np.where(ok, np.where(lam[:, 0] - lam[:, 1] <= AMBIGUOUS_GAP * n_used, AMBIGUOUS, 0),
                              NO_ROTATION).astype(np.int32)
        lam = np.where(ok[:, None], lam, np.nan)
    R = np.where(ok[:, None, None], R, np.nan)
    spread = np.zeros((m, K))
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                dlt = W[:, :, i, j] - R[:, None, i, j]
                spread = spread + dlt * dlt
    spread = np.where(used & ok[:, None], spread, np.nan)
    pose = np.zeros((m, 4, 4))
    pose[:, :3, :3] = R
    pose[:, :3, 3] = np.asarray(X, np.float64)[b:e]
    pose[:, 3, 3] = 1.0
    return dict(rot_views=W, R=R, pose=pose, spread=spread, slot_status=status, row_status=row_status, lam=lam)


def invariants(out):
    """What a result promises whatever its inputs hold, asserted on a dict of
    ``fuse_rotations``' outputs (the model's or the device's; ``rot_views``
    and ``spread`` may be absent): R is finite unless the row has
    NO_ROTATION and NaN where it has; a slot's rot_views are finite if and only
    if its status is 0; its spread is finite if and only if it is usable and
    the row has a rotation."""
    has = (np.asarray(out["row_status"]) & NO_ROTATION) == 0
    usable = np.asarray(out["slot_status"]) == 0
    assert np.isin(out["row_status"], (0, NO_ROTATION, AMBIGUOUS)).all()
    assert np.isin(out["slot_status"], (0, NO_VIEW, NO_CAPTURE, DEGENERATE)).all()
    assert (np.isfinite(out["R"]).all(axis=(1, 2)) == has).all(), "R finite <=> the row has a rotation"
    assert np.isnan(out["R"][~has]).all() and (has <= usable.any(axis=1)).all()
    assert same(np.ascontiguousarray(out["pose"][:, :3, :3]), out["R"])
    if "rot_views" in out:
        assert (np.isfinite(out["rot_views"]).all(axis=(2, 3)) == usable).all(), "rot_views finite <=> slot status 0"
        assert np.isnan(out["rot_views"][~usable]).all()
    if "spread" in out:
        assert (np.isfinite(out["spread"]) == (usable & has[:, None])).all(), "spread finite <=> usable and fused"


# ---- inputs ---------------------------------------------------------------------------------

def euler_filter(raw):
    """raw float32 [n, 3] -> bool [n]: the vectors whose three wrapped angles
    all have a float64 sine and cosine further than EULER_MARGIN, relative,
    from every float32 rounding boundary.  Any float64 sine good to a few
    thousand ulp then rounds to the same float32."""
    a = wrap_euler(raw).astype(np.float64)
    keep = np.ones(a.shape, bool)
    for v in (np.sin(a), np.cos(a)):
        f = v.astype(np.float32)
        lo = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2
        hi = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
        keep &= np.minimum(np.abs(v - lo), np.abs(v - hi)) > EULER_MARGIN * np.abs(v)
    return keep.all(axis=1)


def random_raw(rng, n, mode):
    """n raw vectors of ``mode``: standard normal (quat, 6d) or angles within
    +-3 turns that pass ``euler_filter`` (which may drop 1 % at the most)."""
    D = MODES[mode][1]
    if mode != "euler":
        return rng.standard_normal((n, D)).astype(np.float32)
    draw = rng.uniform(-6 * np.pi, 6 * np.pi, (n + n // 50 + 8, 3)).astype(np.float32)
    keep = euler_filter(draw)
    assert (~keep).sum() <= len(draw) // 100, "the filter dropped more than 1 % of the angles"
    return np.ascontiguousarray(draw[keep][:n])


def random_rotations(rng, n):
    """n rotations f64 [n, 3, 3], uniform, orthonormal to a few ulp."""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return quat_matrix(q[:, 0], q[:, 1], q[:, 2], q[:, 3], 1.0, 2.0)


def axis_angle(axis, angle):
    """Rodrigues' formula in float64 -> [3, 3]."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)
