"""Hand-built inputs where the rotation fusion is hard: the cube
group with its exact ties, a sum of exactly zero, views next to half a turn
apart either side of the ambiguity threshold, a double largest eigenvalue,
uniform rotations over all of SO(3), the decoders' extremes and rigs that are
not finite.  A helper, not a test: tests/test_pose_edges_model.py proves on the
CPU which regime every input is in, tests/test_pose_edges_gpu.py demands the
model's bits of the device.

Every function returns a ``Table`` with the fields tests/test_pose_gpu.py's
``Case`` carries, so its ``run_op``, ``expected`` and ``check`` take it.  An
exact rotation reaches a slot in one of two ways:

- ``mode="6d"`` over an identity rig: two signed unit axis vectors decode
  exactly, so the 24 rotations of the cube are float32-exact (``cube_raw``);
- ``through_rig``: raw ``(0, 0, 0, 1)`` in ``mode="quat"`` decodes to the exact
  identity, and with ``RTs[s, c, :3, :3] = W^T`` and one capture per row the
  world product returns the float64 ``W`` to the last bit.
"""
from functools import lru_cache
from itertools import combinations, permutations, product

import numpy as np

import pose_model as M
from bpc_baseline_amd.synth import make_rig

DELTAS = (1e-1, 1e-3, 1e-5, 1e-7, 1e-8, 3e-9, 1e-9, 1e-10, 1e-12, 0.0)     # family c: the angle short of a half turn
PER_DELTA = 6
EULER_SCALES = (1e3, 1e6, 1e12, 1e30, 3e38)
BAD_CAM = 2                                                               # family h, and fuse="cam"'s default
RIG_KINDS = ("nan", "+inf", "-inf", "1e308", "translation")
RIG_BOUND_KINDS = ("at_max", "below_max")                                 # either side of pose_model.WORLD_MAX


class Table:
    """The fields of test_pose_gpu.Case: ``raw`` float32 [n, C, D], ``views``
    int32 [n, C], ``scene`` int32 [n], ``X`` f64 [n, 3], ``RTs`` f64
    [S, C, 4, 4]; ``tags`` holds what a family knows of its rows."""

    def __init__(self, mode, raw, views, RTs, scene, **tags):
        self.mode, self.scene_base = mode, 0
        self.raw = np.ascontiguousarray(raw, np.float32)
        self.views = np.ascontiguousarray(views, np.int32)
        self.RTs = np.ascontiguousarray(RTs, np.float64)
        self.scene = np.ascontiguousarray(scene, np.int32)
        self.n, self.C = self.views.shape
        self.S = len(self.RTs)
        assert self.raw.shape == (self.n, self.C, M.MODES[mode][1]) and self.RTs.shape == (self.S, self.C, 4, 4)
        assert self.scene.shape == (self.n,) and self.scene.min() >= 0 and self.scene.max() < self.S
        self.X = np.random.default_rng(self.n).uniform(-300, 300, (self.n, 3))
        self.tags = tags

    def device(self, dev):
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t(self.scene), t(self.views), t(self.X), t(self.RTs)

    def model(self, fuse="mean", cam=BAD_CAM, cams=None):
        cams = list(range(self.C)) if cams is None else list(cams)
        return M.fuse_rotations(self.raw[:, cams], self.scene, self.views, self.X, self.RTs, self.mode, cams=cams,
                                fuse=fuse, cam=cam)


def identity_rig(S, C):
    return np.tile(np.eye(4), (S, C, 1, 1))


def through_rig(W, used, degenerate=None):
    """W f64 [n, C, 3, 3], used bool [n, C] -> a "quat" table with one capture
    per row whose usable slots hold exactly W; ``degenerate`` slots have a view
    and the zero quaternion, every other slot has no view."""
    n, C = used.shape
    degenerate = np.zeros((n, C), bool) if degenerate is None else degenerate
    assert not (used & degenerate).any()
    raw = np.zeros((n, C, 4), np.float32)
    raw[..., 3] = 1
    raw[degenerate] = 0
    RTs = identity_rig(n, C)
    RTs[:, :, :3, :3] = np.where(used[:, :, None, None], np.swapaxes(W, 2, 3), np.eye(3))
    return Table("quat", raw, np.where(used | degenerate, 0, -1), RTs, np.arange(n))


# ---- a, b: the cube group over an identity rig ------------------------------------------------

@lru_cache(maxsize=None)
def cube_group():
    """The 24 rotations of the cube, f64 [24, 3, 3], the identity first."""
    out = []
    for perm in permutations(range(3)):
        for signs in product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            R[np.arange(3), perm] = signs
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    out.sort(key=lambda R: -np.trace(R))
    assert len(out) == 24 and (out[0] == np.eye(3)).all()
    return np.stack(out)


def cube_raw(idx):
    """The 6-D vectors (first and second column) of the cube rotations idx."""
    G = cube_group()[np.asarray(idx)]
    return np.concatenate([G[..., :, 0], G[..., :, 1]], axis=-1).astype(np.float32)


def _cube_table(rows):
    n = len(rows)
    idx, views = np.zeros((n, 4), np.int64), np.full((n, 4), -1, np.int32)
    for r, row in enumerate(rows):
        idx[r, :len(row)], views[r, :len(row)] = row, 0
    t = Table("6d", cube_raw(idx), views, identity_rig(1, 4), np.zeros(n), size=np.array([len(r) for r in rows]))
    t.tags["idx"] = idx
    return t


@lru_cache(maxsize=None)
def cube_rows():
    """a: every single rotation of the cube, every pair, every triple and
    1,000 seeded quadruples with repetition, four cameras."""
    rng = np.random.default_rng(24)
    rows = [c for k in (1, 2, 3) for c in combinations(range(24), k)]
    rows += [tuple(q) for q in rng.integers(0, 24, (1000, 4))]
    return _cube_table(rows)


@lru_cache(maxsize=None)
def zero_sum():
    """b: the four half-turn-related views I, diag(1,-1,-1), diag(-1,1,-1),
    diag(-1,-1,1), which sum to exactly zero, and a row whose only usable slot
    is the all-zero 6-D vector (the zero matrix, slot status 0)."""
    G = cube_group()
    diag = [int(np.nonzero([(g == np.diag(d)).all() for g in G])[0][0])
            for d in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
    t = _cube_table([tuple(diag), (0,)])
    t.raw[1, 0] = 0
    return t


# ---- c, d, e, f: float64 rotations through the rig --------------------------------------------

def _pair(rng, delta):
    B = M.random_rotations(rng, 1)[0]
    return B, B @ M.axis_angle(rng.standard_normal(3), np.pi - delta)


@lru_cache(maxsize=None)
def half_turn():
    """c: rows of B and B . axis_angle(a, pi - delta), PER_DELTA seeded (B, a)
    for each delta of DELTAS, in slots 0 and 2 of three cameras."""
    rng = np.random.default_rng(31)
    n = len(DELTAS) * PER_DELTA
    W, used = np.tile(np.eye(3), (n, 3, 1, 1)), np.tile([True, False, True], (n, 1))
    delta = np.repeat(DELTAS, PER_DELTA)
    for r in range(n):
        W[r, 0], W[r, 2] = _pair(rng, delta[r])
    t = through_rig(W, used)
    t.tags["delta"] = delta
    return t


D_DELTAS = (1e-9, 1e-9 / 3)     # family d: the gap is about 4 delta per pair of views, here 4e-9 in both rows


@lru_cache(maxsize=None)
def used_not_selected():
    """d: two rows of eight selected cameras.  Row 0: one pair of family c at
    delta = 1e-9 (gap about 4e-9, above 1e-9 . 2, below 1e-9 . 8) among three
    slots without a view and three degenerate ones: not ambiguous.  Row 1:
    three copies of such a pair at delta = 1e-9 / 3 (the sum and the gap are
    three times a pair's: about 4e-9 again, at or below 1e-9 . 6) with one slot
    of either kind: ambiguous."""
    rng = np.random.default_rng(32)
    W = np.tile(np.eye(3), (2, 8, 1, 1))
    used, degenerate = np.zeros((2, 8), bool), np.zeros((2, 8), bool)
    W[0, 1], W[0, 6] = _pair(rng, D_DELTAS[0])
    used[0, [1, 6]], degenerate[0, [0, 3, 7]] = True, True
    a, b = _pair(rng, D_DELTAS[1])
    W[1, [0, 3, 5]], W[1, [2, 4, 7]] = a, b
    used[1, [0, 2, 3, 4, 5, 7]], degenerate[1, 6] = True, True
    return through_rig(W, used, degenerate)


@lru_cache(maxsize=None)
def symmetric():
    """e: three views 0, 120 and 240 degrees about one axis (the sum is 3 a
    a^T, its largest eigenvalue double), and in the next row the same with the
    third view off by 1e-6 rad; eight seeded axes, the last four behind a
    common rotation B."""
    rng = np.random.default_rng(33)
    W, exact = [], []
    for i in range(8):
        a = rng.standard_normal(3)
        B = M.random_rotations(rng, 1)[0] if i >= 4 else np.eye(3)
        for off in (0.0, 1e-6):
            W.append([B @ M.axis_angle(a, 0.0), B @ M.axis_angle(a, 2 * np.pi / 3),
                      B @ M.axis_angle(a, 4 * np.pi / 3 + off)])
            exact.append(off == 0.0)
    t = through_rig(np.array(W), np.ones((len(W), 3), bool))
    t.tags["exact"] = np.array(exact)
    return t


@lru_cache(maxsize=None)
def wide():
    """f: uniform random rotations in 2, 3, 4 and 8 usable slots of eight
    cameras, 200 rows each; the other slots have no view."""
    rng = np.random.default_rng(34)
    k = np.repeat((2, 3, 4, 8), 200)
    n = len(k)
    used = np.zeros((n, 8), bool)
    for r in range(n):
        used[r, rng.permutation(8)[:k[r]]] = True
    return through_rig(M.random_rotations(rng, n * 8).reshape(n, 8, 3, 3), used)


# ---- g: the decoders' extremes -----------------------------------------------------------------

QUAT_EXTREMES = (((1e20, 0, 0, 1), False), ((3e38, 3e38, 3e38, 3e38), False), ((2e19, 1, 1, 1), False),
                 ((1e-20, 1e20, 0, 0), False), ((1e19, 1e19, 0, 0), True))
# (vector, finite): the finite ones are no rotations, their determinant is 0, or 0.017 in the last
SIXD_EXTREMES = (((1e20, 0, 0, 0, 1, 0), True), ((1, 0, 0, 1e38, 1e38, 0), True),
                 ((3e38, 3e38, 3e38, 1, 0, 0), True), ((0, 0, 0, 0, 0, 0), True), ((1, 0, 0, 0, 0, 0), True),
                 ((1e-30, 0, 0, 0, 1e30, 0), True), ((1, 1, 0, 3e38, 3e38, 3e38), False),
                 ((1, 2, 3, 2, 4, 6), True))


def euler_edge_angles():
    pi32, inf32 = M.PI32, np.float32(np.inf)
    fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)
    edge = []
    for p in (pi32, -pi32):
        edge += [np.nextafter(p, -inf32), p, np.nextafter(p, inf32)]
    edge += [M.TWO_PI32, np.float32(-0.0), tiny, -tiny, fmax, -fmax]
    return np.array(edge, np.float32)


def euler_extremes():
    """The edge angles one at a time in each position, all of them in turn in
    all three, then 200 seeded vectors at each of EULER_SCALES, all through
    ``euler_filter`` -> (raw [n, 3], how many of the first are edge rows)."""
    edge = euler_edge_angles()
    rows = [np.roll([e, 0, 0], i) for e in edge for i in range(3)]
    rows += [[edge[i], edge[(i + 1) % len(edge)], edge[(i + 2) % len(edge)]] for i in range(len(edge))]
    rows = np.array(rows, np.float32)
    assert M.euler_filter(rows).all(), "an edge angle lies on a float32 rounding boundary"
    rng = np.random.default_rng(35)
    out = [rows]
    for scale in EULER_SCALES:
        draw = rng.uniform(-scale, scale, (208, 3)).astype(np.float32)
        keep = M.euler_filter(draw)
        assert (~keep).sum() <= len(draw) // 100, "the filter dropped more than 1 % of the angles"
        out.append(draw[keep][:200])
    return np.concatenate(out), len(rows)


@lru_cache(maxsize=None)
def decode_extremes(mode):
    """g: each vector in all three slots of its own row (so fuse="cam" sees it
    too), one capture, a random three-camera rig."""
    if mode == "euler":
        vec, n_edge = euler_extremes()
        tags = dict(n_edge=n_edge)
    else:
        listed = QUAT_EXTREMES if mode == "quat" else SIXD_EXTREMES
        vec = np.array([v for v, _ in listed], np.float32)
        tags = dict(finite=np.array([f for _, f in listed]))
    n = len(vec)
    rig = np.stack(make_rig(np.random.default_rng(36), 3)[1])[None].astype(np.float64)
    return Table(mode, np.repeat(vec[:, None], 3, axis=1), np.zeros((n, 3)), rig, np.zeros(n), **tags)


# ---- h: rigs that are not finite ----------------------------------------------------------------

@lru_cache(maxsize=None)
def bad_rig(kind):
    """h: three rows of four cameras over one capture, random quaternions.
    ``kind`` puts a NaN, an infinity or 1e308 into camera BAD_CAM's rotation
    block, or ("translation") a NaN into the translation column and the bottom
    row of its matrix, which nothing reads; "clean" is the rig itself.
    "at_max" and "below_max" give that camera the identity quaternion and the
    block diag(v, 1, 1), so that its world rotation holds exactly v = -2^500
    (degenerate) or the float64 below 2^500 (usable: finite, and no rotation)."""
    rng = np.random.default_rng(37)
    raw = M.random_raw(rng, 12, "quat").reshape(3, 4, 4)
    RTs = np.stack(make_rig(rng, 4)[1])[None].astype(np.float64).copy()
    if kind in RIG_BOUND_KINDS:
        raw[:, BAD_CAM] = (0, 0, 0, 1)
        RTs[0, BAD_CAM, :3, :3] = np.eye(3)
        RTs[0, BAD_CAM, 0, 0] = -M.WORLD_MAX if kind == "at_max" else np.nextafter(M.WORLD_MAX, 0.0)
    elif kind == "translation":
        RTs[0, BAD_CAM, :3, 3], RTs[0, BAD_CAM, 3, :] = np.nan, np.nan
    elif kind != "clean":
        RTs[0, BAD_CAM, 1, 2] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "1e308": 1e308}[kind]
    return Table("quat", raw, np.zeros((3, 4)), RTs, np.zeros(3))


def mean_tables():
    """name -> table, the families that run with fuse="mean"."""
    out = dict(cube=cube_rows(), zero_sum=zero_sum(), half_turn=half_turn(), used_not_selected=used_not_selected(),
               symmetric=symmetric(), wide=wide())
    out.update({f"rig_{k}": bad_rig(k) for k in RIG_KINDS + RIG_BOUND_KINDS})
    return out


def all_tables():
    out = mean_tables()
    out.update({f"decode_{m}": decode_extremes(m) for m in M.MODES})
    return out
