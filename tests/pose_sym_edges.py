"""Hand-built inputs for the mean under symmetries.  A helper,
not a test: tests/test_pose_sym_model.py proves on the CPU what every family
is, tests/test_pose_sym_gpu.py demands the model's bits of the device.  Every
function returns (``pose_edges.Table``, syms f64 [K, 4, 4]) and the table's
``tags`` hold what the family knows of its rows."""
from functools import lru_cache

import numpy as np

import pose_edges as E
import pose_model as P
import pose_sym_model as M

BAD_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "1e308": 1e308, "zero": 0.0}
# (n, C, K, rounds) of the GPU test's main parametrisation, and (n, C, seed) of every test_pose_gpu.Case that
# tests/test_pose_sym_gpu.py builds in mode "euler" (scene_base = 7 is a quaternion case)
GPU_SIZES = ((1, 3, 1, 2), (255, 5, 2, 1), (256, 8, 4, 2), (257, 8, 24, 4), (513, 5, 64, 2), (257, 3, 1024, 2),
             (256, 3, 64, 1), (255, 5, 24, 4))
EULER_CASES = tuple(sorted({(n, C, 0) for n, C, _, _ in GPU_SIZES} | {(257, 4, 0)}))
ROUND2_DEG = (25.0, -17.0, -23.0, -24.0)          # the reference view, then three either side of -45 degrees from it


def cube_index(R):
    """The index of the cube rotation R in ``pose_edges.cube_group``."""
    return int(np.nonzero((E.cube_group() == R).all(axis=(1, 2)))[0][0])


@lru_cache(maxsize=None)
def cube_views():
    """400 rows of four views R G_k over the identity rig in "6d" (float32
    exact): R and every k seeded from the cube group, which is the symmetry
    group too.  tags: ``first`` the index of R G_k0, ``sym`` the S every slot
    must take to reach it."""
    rng = np.random.default_rng(41)
    G = E.cube_group()
    a, k = rng.integers(0, 24, 400), rng.integers(0, 24, (400, 4))
    idx = np.array([[cube_index(G[a[r]] @ G[k[r, c]]) for c in range(4)] for r in range(400)])
    sym = np.array([[cube_index(G[k[r, c]].T @ G[k[r, 0]]) for c in range(4)] for r in range(400)], np.int32)
    t = E._cube_table([tuple(row) for row in idx])
    t.tags.update(first=idx[:, 0], sym=sym)
    return t, M.with_blocks(G)


def z_views(rng, n, C, fold, noise_deg, used=None):
    """n rows of C views R0 Rz(2 pi k / fold + noise) through the rig, R0
    uniform, k seeded, |noise| <= noise_deg -> (table, syms, R0, k)."""
    R0 = P.random_rotations(rng, n)
    k = rng.integers(0, fold, (n, C))
    ang = 2 * np.pi * k / fold + np.radians(rng.uniform(-noise_deg, noise_deg, (n, C)))
    W = np.array([[R0[r] @ M.rot_z(ang[r, c]) for c in range(C)] for r in range(n)])
    used = np.ones((n, C), bool) if used is None else used
    t = E.through_rig(W, used)
    t.tags.update(R0=R0, k=k, W=W)
    return t, M.z_fold(fold)


@lru_cache(maxsize=None)
def duplicated():
    """Exact quarter turns about z under {I, Rz90, Rz90 again, Rz180, Rz270,
    Rz270 again}: a view that needs a duplicated element takes the lower index
    with a margin of exactly 0."""
    t, four = z_views(np.random.default_rng(42), 64, 4, 4, 0.0)
    return t, four[[0, 1, 1, 2, 3, 3]]


@lru_cache(maxsize=None)
def round_two():
    """A four-fold axis with the reference view 25 degrees off and the others
    either side of 45 degrees from it: round 1 sends two of them to the
    neighbouring element, round 2 moves the third after them, round 3 changes
    nothing.  32 rows behind seeded R0 and quarter turns."""
    rng = np.random.default_rng(43)
    n = 32
    R0 = P.random_rotations(rng, n)
    k = rng.integers(0, 4, (n, 4))
    k[:, 0] = 0
    W = np.array([[R0[r] @ M.rot_z(np.radians(ROUND2_DEG[c]) + np.pi / 2 * k[r, c]) for c in range(4)]
                  for r in range(n)])
    t = E.through_rig(W, np.ones((n, 4), bool))
    t.tags.update(R0=R0)
    return t, M.z_fold(4)


@lru_cache(maxsize=None)
def lost_reference():
    """Rows of five cameras whose first selected slots are not usable: row 0
    NO_VIEW, NO_VIEW, then views; row 1 DEGENERATE, NO_VIEW, then views; row 2
    every slot DEGENERATE; row 3 a capture the rig does not hold.  Exact
    quarter turns, four-fold symmetry."""
    rng = np.random.default_rng(44)
    used = np.array([[0, 0, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], bool)
    degenerate = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]], bool)
    t, syms = z_views(rng, 4, 5, 4, 0.0, used)
    t2 = E.through_rig(t.tags["W"], used, degenerate)
    t2.tags.update(t.tags)
    t2.scene[3] = t2.S                                    # past the rig's captures
    return t2, syms


@lru_cache(maxsize=None)
def bad_symmetries(kind, everywhere):
    """Noisy four-fold rows under a group with ``kind`` written over the whole
    block of element 1 (or of every element)."""
    t, syms = z_views(np.random.default_rng(45), 48, 4, 4, 8.0)
    syms = syms.copy()
    syms[slice(None) if everywhere else 1, :3, :3] = BAD_VALUES[kind]
    return t, syms


@lru_cache(maxsize=None)
def one_bad_entry(kind):
    """The same rows with a single entry of element 2 replaced."""
    t, syms = z_views(np.random.default_rng(46), 48, 4, 4, 8.0)
    syms = syms.copy()
    syms[2, 1, 0] = BAD_VALUES[kind]
    return t, syms


def families():
    """name -> (table, syms): what the GPU test sends to the device."""
    out = dict(cube=cube_views(), duplicated=duplicated(), round_two=round_two(), lost_reference=lost_reference())
    for kind in BAD_VALUES:
        out[f"bad_{kind}_one"] = bad_symmetries(kind, False)
        out[f"bad_{kind}_all"] = bad_symmetries(kind, True)
        out[f"entry_{kind}"] = one_bad_entry(kind)
    return out


def model(t, syms, rounds=2, cams=None):
    cams = list(range(t.C)) if cams is None else list(cams)
    return M.fuse_rotations_sym(t.raw[:, cams], t.scene, t.views, t.X, t.RTs, t.mode, syms, cams=cams, rounds=rounds)
