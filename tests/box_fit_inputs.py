"""The inputs the CPU and GPU tests of the box fit share (DESIGN §3.22;
tests/box_fit_model.py is the statement).  A helper, not a test.

``build`` makes ``synth.make_rig`` rigs of C cameras, a vertex cloud whose
origin is off the middle of its extent, a random rotation and a true
translation per row, and per view the truncated (toward zero, as the
detector's ``int(box)``) extents of the exact projection, optionally with
pixel noise first.  A row's start is the DLT of all its box centres (what the
table's X is); it then keeps a random 1..C of its views for the fit.
"""
import functools

import numpy as np

import box_fit_model as M
from bpc_baseline_amd.inference.utils.camera_utils import projection_matrices
from bpc_baseline_amd.synth import make_rig
from oracle import pipeline as OP
from score_model import random_rotations

I32_MIN = np.iinfo(np.int32).min
LO, HI = np.array([-20.0, -40.0, -10.0]), np.array([80.0, 40.0, 30.0])      # mm: the origin is off-centre


def cloud(rng, V):
    """V vertices uniform in the off-centre box -> f64 [V, 3]."""
    return rng.uniform(LO, HI, (V, 3))


def cloud_with_outliers(rng, V, at):
    """``cloud`` drawn small, with the vertices ``at`` = (i_xlo, i_ylo, i_xhi,
    i_yhi) far out along -x, -y, +x, +y of the object."""
    v = rng.uniform(-10.0, 10.0, (V, 3))
    v[at[0]] = v[at[1]] = v[at[2]] = v[at[3]] = 0.0
    for i, d in zip(at, ((-300.0, 0, 0), (0, -300.0, 0), (300.0, 0, 0), (0, 300.0, 0))):
        v[i] += d
    return v


def project_boxes(P, R, t, verts, rng=None, noise=0.0):
    """The truncated extents of the projection under (R, t) in every view of
    P [C, 3, 4] -> int32 [C, 4]."""
    X = verts @ R.T + t
    h = np.einsum("cij,nj->cni", P[:, :, :3], X) + P[:, None, :, 3]
    u, v = h[..., 0] / h[..., 2], h[..., 1] / h[..., 2]
    b = np.stack([u.min(1), v.min(1), u.max(1), v.max(1)], 1)
    if rng is not None and noise:
        b = b + rng.uniform(-noise, noise, b.shape)
    return np.trunc(b).astype(np.int32)


class Case:
    """One input of the op: host arrays in the op's argument order (``args``),
    the true translation and the kind of every row."""
    FIELDS = ("pose", "scene", "views", "boxes", "proj", "verts")

    def args(self):
        return tuple(getattr(self, k) for k in self.FIELDS)


def build(C, n, V, seed, *, noise=0.0, keep=None, verts=None, per_rig=4, kinds=()):
    """n rows over ceil(n / per_rig) rigs.  ``keep``: the number of views every
    row keeps (default random 1..C).  ``kinds``: (row, kind) pairs, kind one of
      "behind"   the start is a kept camera's centre: a vertex is behind it;
      "near"     one view kept, the truth at 0.3 of the way from its camera to
                 the start: the box is 3.3 times the start's, and the first
                 steps land behind the camera and are rejected;
      "noview"   every view is -1;
      "noscene"  the scene id is no capture (below and above alternately).
    Rows are "fit" otherwise."""
    rng = np.random.default_rng(seed)
    S = max(1, -(-n // per_rig))
    c = Case()
    c.C, c.S, c.V = C, S, V
    c.verts = cloud(rng, V) if verts is None else np.asarray(verts, np.float64)
    rigs = [make_rig(rng, C) for _ in range(S)]
    c.proj = np.stack([projection_matrices(np.stack(k)[None], np.stack(r)[None])[0] for k, r in rigs])
    centres = np.stack([[-rt[:3, :3].T @ rt[:3, 3] for rt in r] for _, r in rigs])          # [S, C, 3]
    c.scene = rng.permutation(np.arange(n) % S).astype(np.int32)
    c.pose = np.tile(np.eye(4), (n, 1, 1))
    c.views = np.full((n, C), -1, np.int32)
    c.boxes = np.zeros((n, C, 4), np.int32)
    c.truth = np.zeros((n, 3))
    c.kind = np.full(n, "fit", dtype=object)
    for w, k in kinds:
        c.kind[w] = k
    Rs = random_rotations(rng, n)
    for w in range(n):
        s, kind = int(c.scene[w]), c.kind[w]
        P = c.proj[s]
        t = np.array([rng.uniform(-250, 250), rng.uniform(-250, 250), rng.uniform(-80, 80)])
        k = C if kind == "behind" else 1 if kind == "near" else keep or int(rng.integers(1, C + 1))
        kept = np.sort(rng.permutation(C)[:k])
        start = t
        if kind == "near":
            t = centres[s, kept[0]] + 0.3 * (start - centres[s, kept[0]])
        c.truth[w] = t
        c.pose[w, :3, :3] = Rs[w]
        c.boxes[w] = project_boxes(P, Rs[w], t, c.verts, rng, noise)
        cent = 0.5 * (c.boxes[w][:, :2] + c.boxes[w][:, 2:]).astype(np.float64)
        c.pose[w, :3, 3] = OP.triangulate(P[None], cent[None])[0]
        if kind == "behind":
            c.pose[w, :3, 3] = centres[s, kept[0]]
        if kind == "near":
            c.pose[w, :3, 3] = start                 # the same ray, 3.3 times as deep
        c.views[w, kept] = rng.integers(0, 50, k)
        if kind == "noview":
            c.views[w] = rng.integers(-5, 0, C)
        if kind == "noscene":
            c.scene[w] = -1 - w if w % 2 else S + w
    return c


def zero_columns(c, scenes):
    """The captures ``scenes`` get P with zero first three columns (A = 0: no
    pivot); their rows become "azero".  In place -> c."""
    for s in scenes:
        c.proj[s, :, :, :3] = 0.0
        c.kind[(c.scene == s) & (c.kind == "fit")] = "azero"
    return c


def restarts(c, max_evals=10):
    """The converged rows of ``c`` started again at their own result: a start
    that already satisfies the stop rule -> a Case of those rows ("restart")."""
    out = M.fit_boxes(*c.args(), max_evals)
    rows = np.nonzero(out["info"][:, 0] == M.CONVERGED)[0]
    r = Case()
    r.C, r.S, r.V, r.verts, r.proj = c.C, c.S, c.V, c.verts, c.proj
    r.pose, r.scene, r.views, r.boxes = out["pose"][rows], c.scene[rows], c.views[rows], c.boxes[rows]
    r.truth, r.kind = c.truth[rows], np.full(len(rows), "restart", dtype=object)
    return r


def last_case(V):
    """All four kinds of extreme on the last vertex, over a row's views: R = I,
    the last vertex far out along +x +y, camera 0 upright (it is umax and vmax
    there), camera 1 rolled half a turn (umin and vmin), camera 2 upright and
    not kept.  Three rows, the truth a few mm off the start."""
    rng = np.random.default_rng(2700 + V)
    c = Case()
    c.C, c.S, c.V = 3, 1, V
    c.verts = rng.uniform(-10.0, 10.0, (V, 3))
    c.verts[V - 1] = (300.0, 300.0, 0.0)
    K = np.array([[4000.0, 0, 1200], [0, 4000.0, 1200], [0, 0, 1]])
    Rz = np.diag([-1.0, -1.0, 1.0])
    RT = [np.concatenate([r, [[0.0], [0.0], [1500.0]]], 1) for r in (np.eye(3), Rz, np.eye(3))]
    c.proj = np.stack([K @ rt for rt in RT])[None]
    n = 3
    c.pose = np.tile(np.eye(4), (n, 1, 1))
    c.scene = np.zeros(n, np.int32)
    c.views = np.tile(np.array([3, 0, -1], np.int32), (n, 1))
    c.truth = rng.uniform(-40, 40, (n, 3))
    c.boxes = np.stack([project_boxes(c.proj[0], np.eye(3), t, c.verts) for t in c.truth])
    c.pose[:, :3, 3] = c.truth + rng.uniform(-5, 5, (n, 3))
    c.kind = np.full(n, "fit", dtype=object)
    return c


def tie_case(swap):
    """The hand-built exact tie: P = [I | 0], R = I, t0 = (0, 0, 1); vertices
    (1, 0, 1) and (2, 0, 3) share u = 0.5 at depths 2 and 4, the others lie
    inside.  ``swap`` exchanges the two in ``verts``: the maximum's depth, and
    with it its Jacobian row, is the other one's."""
    c = Case()
    c.C, c.S = 3, 1
    v = np.array([[1.0, 0.0, 1.0], [2.0, 0.0, 3.0], [-1.0, -1.0, 1.0], [-0.5, 1.0, 1.0], [0.25, 0.25, 2.0]])
    if swap:
        v[[0, 1]] = v[[1, 0]]
    c.verts, c.V = v, len(v)
    c.proj = np.tile(np.eye(3, 4), (1, 3, 1, 1))
    c.pose = np.eye(4)[None].copy()
    c.pose[0, 2, 3] = 1.0
    c.scene = np.zeros(1, np.int32)
    c.views = np.array([[0, -1, 4]], np.int32)
    c.boxes = np.tile(np.array([-1, -1, 1, 1], np.int32), (1, 3, 1))
    c.truth, c.kind = np.full((1, 3), np.nan), np.array(["tie"], dtype=object)
    return c


CAMS = (3, 4, 8)
MAX_EVALS = (1, 2, 10, 64)
VERTS = (1, 2, 63, 64, 65, 129, 1024)
ROWS = (1, 3, 4, 5, 257)


@functools.lru_cache(maxsize=None)
def case(name, C=3):
    """The named inputs of the tests."""
    if name.startswith("verts"):        # V at the lanes' edges: 6 rows
        return build(C, 6, int(name[5:]), 2200 + C, noise=0.5)
    if name.startswith("rows"):         # row counts at the workgroup's edge
        return build(C, int(name[4:]), 5, 2300 + C, noise=0.5)
    if name == "regimes":
        kinds = [(w, k) for w, k in zip(range(20), ("behind", "near", "noview", "noscene", "fit") * 4)]
        c = build(C, 36, 9, 2400 + C, noise=0.5, kinds=kinds)
        plain = [s for s in range(c.S) if not set(c.kind[c.scene == s]) - {"fit", "noview"}]
        return zero_columns(c, plain[:2])
    if name == "restart":
        return restarts(build(C, 12, 9, 2500 + C))
    if name == "truth":                 # a few hundred rows: the mean distance to the true translation
        return build(C, 240, 24, 2600 + C, noise=0.0, per_rig=8)
    if name.startswith("last"):         # all four kinds of extreme on the last vertex
        return last_case(int(name[4:]))
    if name == "stride2":               # the extremes in the second stride of lanes 5..8
        return build(C, 3, 129, 2800 + C, keep=C,
                     verts=cloud_with_outliers(np.random.default_rng(7), 129, (69, 70, 71, 72)))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, C=3, max_evals=10):
    """``fit_boxes`` of ``case(name, C)`` with its traces, computed once -> (outputs, traces)."""
    traces = {}
    return M.fit_boxes(*case(name, C).args(), max_evals, traces=traces), traces


class Captures:
    """Detector outputs of S captures of C cameras whose objects are known."""


@functools.lru_cache(maxsize=None)
def captures(C, S=3, n_obj=5, V=12, seed=2900):
    """S captures of C cameras, each of ``n_obj`` copies of one model (``verts``)
    at known poses (``R`` [S, n_obj, 3, 3], ``t`` [S, n_obj, 3]) that every
    camera sees: per view the boxes are the truncated extents of the exact
    projections, shuffled.  ``ident[s][c]``: the object of each detection."""
    rng = np.random.default_rng(seed + C)
    f = Captures()
    f.S, f.C, f.verts = S, C, cloud(rng, V)
    f.Ks, f.RTs = np.zeros((S, C, 3, 3), np.float32), np.zeros((S, C, 4, 4))
    f.R = random_rotations(rng, S * n_obj).reshape(S, n_obj, 3, 3)
    f.t = np.stack([rng.uniform(-250, 250, (S, n_obj)), rng.uniform(-250, 250, (S, n_obj)),
                    rng.uniform(-80, 80, (S, n_obj))], axis=2)
    f.ident, boxes = [], []
    for s in range(S):
        Ks, RTs = make_rig(rng, C)
        f.Ks[s], f.RTs[s] = np.stack(Ks), np.stack(RTs)
        P = projection_matrices(f.Ks[s][None], f.RTs[s][None])[0]
        b = np.stack([project_boxes(P, f.R[s, o], f.t[s, o], f.verts) for o in range(n_obj)], 1)     # [C, n_obj, 4]
        order = [rng.permutation(n_obj) for _ in range(C)]
        f.ident.append(order)
        boxes += [b[c][order[c]] for c in range(C)]
    f.boxes = np.concatenate(boxes).astype(np.float32)
    f.conf = np.full(len(f.boxes), 0.9, np.float32)
    f.cls = np.zeros(len(f.boxes), np.float32)
    f.img_offs = np.arange(S * C + 1, dtype=np.int64) * n_obj
    return f


def first_three(f):
    """Cameras 0-2 of every capture as a batch of their own -> Captures."""
    g = Captures()
    n = int(f.img_offs[1])
    rows = np.concatenate([np.arange(f.C * s * n, (f.C * s + 3) * n) for s in range(f.S)])
    g.S, g.C, g.verts, g.R, g.t = f.S, 3, f.verts, f.R, f.t
    g.Ks, g.RTs, g.ident = f.Ks[:, :3].copy(), f.RTs[:, :3].copy(), [i[:3] for i in f.ident]
    g.boxes, g.conf, g.cls = f.boxes[rows], f.conf[rows], f.cls[rows]
    g.img_offs = np.arange(f.S * 3 + 1, dtype=np.int64) * n
    return g
