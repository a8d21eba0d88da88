"""tests/pose_model.py against the reference's recorded results
(tests/golden/rot_decode.npz, written by tools/gen_golden_rotations.py), its
closed forms and its independent statement of the mean.  CPU."""
import os
from fractions import Fraction

import numpy as np
import pytest

import pose_model as M
from bpc_baseline_amd.synth import make_rig

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "rot_decode.npz"))
EPS = float(np.spacing(1.0))
# the model's distance to the reference: measured on the golden inputs (1.2e-7,
# 2.6e-6 and 0, the issue's own inputs gave 1.2e-7, 2.1e-6 and 2.2e-16), one power of two up
BOUND_EULER, BOUND_6D, BOUND_WORLD = 2.0 ** -22, 2.0 ** -17, 2.0 ** -51


def _finite(mode):
    return np.isfinite(GOLDEN[f"{mode}_rot"]).all(axis=(1, 2))


def test_quat_is_the_reference_bit_for_bit():
    got, ok = M.decode(GOLDEN["quat_raw"], "quat"), _finite("quat")
    assert ok.sum() >= 300 and M.same(got[ok], GOLDEN["quat_rot"][ok])
    assert not np.isfinite(got[~ok]).all(axis=(1, 2)).any()           # the zero quaternion: not finite in both


@pytest.mark.parametrize("mode, bound", (("euler", BOUND_EULER), ("6d", BOUND_6D)))
def test_distance_to_the_reference(mode, bound):
    got, ok = M.decode(GOLDEN[f"{mode}_raw"], mode), _finite(mode)
    assert ok.all() and np.isfinite(got).all()
    worst = np.abs(got.astype(np.float64) - GOLDEN[f"{mode}_rot"]).max()
    print(mode, "largest distance to the reference:", worst)
    assert worst <= bound


@pytest.mark.parametrize("mode", ("euler", "quat", "6d"))
def test_world_product_and_pose_layout(mode):
    ok = _finite(mode)
    R = GOLDEN["rts"][GOLDEN[f"{mode}_cam"]][:, :3, :3]
    W = M.to_world(R, GOLDEN[f"{mode}_rot"])
    worst = np.abs(W[ok] - GOLDEN[f"{mode}_world"][ok]).max()
    print(mode, "world product, largest distance:", worst)
    assert worst <= BOUND_WORLD
    if mode == "quat":                                                # the whole chain, fuse="cam"
        n, cam = len(ok), GOLDEN["quat_cam"]
        views = np.where(np.arange(3)[None, :] == cam[:, None], 0, -1).astype(np.int32)
        for c in range(3):
            rows = np.nonzero(cam == c)[0]
            out = M.fuse_rotations(GOLDEN["quat_raw"][rows][:, None], np.zeros(len(rows), np.int32), views[rows],
                                   GOLDEN["t"][rows], GOLDEN["rts"][None], "quat", cams=[c], fuse="cam", cam=c)
            good = ok[rows]
            assert np.abs(out["pose"][good] - GOLDEN["pose"][rows][good]).max() <= BOUND_WORLD
            assert (out["row_status"][~good] == M.NO_ROTATION).all() and (out["row_status"][good] == 0).all()
            assert (out["pose"][:, 3] == [0, 0, 0, 1]).all() and (out["pose"][:, :3, 3] == GOLDEN["t"][rows]).all()


def test_closed_forms():
    eye = np.eye(3, dtype=np.float32)
    assert M.same(M.decode(np.zeros((1, 3), np.float32), "euler")[0], eye)
    assert M.same(M.decode(np.array([[0, 0, 0, 1]], np.float32), "quat")[0], eye)
    assert M.same(M.decode(np.array([[0, 0, 0, -3]], np.float32), "quat")[0], eye)
    assert M.same(M.decode(np.array([[1, 0, 0, 0, 1, 0]], np.float32), "6d")[0], eye)
    assert M.same(M.decode(np.array([[5, 0, 0, 7, 2, 0]], np.float32), "6d")[0], eye)
    h = np.sqrt(0.5)
    qz = M.decode(np.array([[0, 0, h, h]], np.float32), "quat")[0]                 # a quarter turn about z
    assert np.abs(qz - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() <= 2.0 ** -22
    ez = M.decode(np.array([[0, 0, np.pi / 2]], np.float32), "euler")[0]
    assert np.abs(ez - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() <= 2.0 ** -22
    ex = M.decode(np.array([[np.pi / 2 + 4 * np.pi, 0, 0]], np.float32), "euler")[0]  # two turns out
    assert np.abs(ex - [[1, 0, 0], [0, 0, -1], [0, 1, 0]]).max() <= 2.0 ** -19
    sz = M.decode(np.array([[0, 1, 0, -1, 0, 0]], np.float32), "6d")[0]
    assert M.same(sz, np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32))
    # R_c = I: the world rotation is the decoded one, widened
    m = M.decode(M.random_raw(np.random.default_rng(0), 50, "quat"), "quat")
    assert M.same(M.to_world(np.tile(np.eye(3), (50, 1, 1)), m), m.astype(np.float64))
    # the wrap, either side of pi and several turns out: the same angle up to whole turns (float32
    # sums: an ulp of 2 pi), never outside [-pi, pi]
    pi32 = np.float32(np.pi)
    lo, hi = np.nextafter(pi32, np.float32(0)), np.nextafter(pi32, np.float32(4))
    a = np.array([lo, hi, -lo, -hi, pi32, -pi32, 0, 1, -2, 7 * np.pi + 0.5, -9 * np.pi - 0.25], np.float32)
    w = M.wrap_euler(a)
    assert w.dtype == np.float32 and (np.abs(w) <= pi32).all() and w[6] == 0
    assert np.abs(np.sin((w.astype(np.float64) - a) / 2)).max() <= 2e-6


def rational_rotations(rng, n):
    """Rotations whose entries are correctly rounded: integer quaternions, the
    entries exact fractions rounded once."""
    out = np.empty((n, 3, 3))
    for r in range(n):
        x, y, z, w = (int(v) for v in rng.integers(-60, 61, 4))
        s = x * x + y * y + z * z + w * w
        if s == 0:
            w, s = 1, 1
        m = [s - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
             2 * x * y + 2 * z * w, s - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
             2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, s - 2 * x * x - 2 * y * y]
        out[r] = np.array([float(Fraction(v, s)) for v in m]).reshape(3, 3)
    return out


@pytest.mark.parametrize("k", (1, 2, 3, 5, 8))
def test_the_mean_of_copies_of_one_rotation_is_that_rotation(k):
    """To 4 ulp of 1 per entry (the entries lie in [-1, 1]); the rotation
    itself is orthonormal to half an ulp."""
    R = rational_rotations(np.random.default_rng(2), 2000)
    Rm, lam = M.mean_rotation(np.repeat(R[:, None], k, axis=1), np.ones((len(R), k), bool))
    assert np.abs(Rm - R).max() <= 4 * EPS
    assert np.abs(lam - [3 * k, -k]).max() <= 1e-13 * k


def test_the_mean_of_plus_and_minus_theta_is_the_identity():
    rng = np.random.default_rng(3)
    for _ in range(200):
        axis, theta = rng.standard_normal(3), rng.uniform(0, 1.5)
        W = np.stack([M.axis_angle(axis, theta), M.axis_angle(axis, -theta)])[None]
        Rm, _ = M.mean_rotation(W, np.ones((1, 2), bool))
        assert np.abs(Rm[0] - np.eye(3)).max() <= 1e-15


def _near(rng, k, degrees):
    base = M.random_rotations(rng, 1)[0]
    return np.stack([base @ M.axis_angle(rng.standard_normal(3), rng.uniform(0, np.radians(degrees) / 2))
                     for _ in range(k)])


def test_the_order_of_two_views_does_not_matter():
    rng = np.random.default_rng(4)
    for _ in range(200):
        W = _near(rng, 2, 60)
        a, _ = M.mean_rotation(W[None], np.ones((1, 2), bool))
        b, _ = M.mean_rotation(W[None, ::-1], np.ones((1, 2), bool))
        assert np.abs(a - b).max() <= 1e-15


def test_jacobi_mean_is_the_svd_mean():
    rng = np.random.default_rng(5)
    for _ in range(500):
        k = int(rng.integers(2, 9))
        W = _near(rng, k, 60)
        Rm, lam = M.mean_rotation(W[None], np.ones((1, k), bool))
        assert np.abs(Rm[0] - M.mean_rotation_svd(W)).max() <= 1e-13
        assert abs(np.linalg.det(Rm[0]) - 1) <= 1e-14 and np.abs(Rm[0].T @ Rm[0] - np.eye(3)).max() <= 1e-14
        assert lam[0, 0] - lam[0, 1] > 1e-9 * k


def test_unused_slots_take_no_part():
    rng = np.random.default_rng(6)
    W = _near(rng, 5, 40)
    used = np.array([[True, False, True, True, False]])
    a, la = M.mean_rotation(W[None], used)
    b, lb = M.mean_rotation(W[None, [0, 2, 3]], np.ones((1, 3), bool))
    assert M.same(a, b) and M.same(la, lb)


def _one_row(raw, views, mode="quat", scene=0, S=1, C=3, **kw):
    rig = np.tile(np.eye(4), (S, C, 1, 1))
    return M.fuse_rotations(np.asarray(raw, np.float32)[None], np.array([scene], np.int32),
                            np.array([views], np.int32), np.array([[1.0, 2.0, 3.0]]), rig, mode, **kw)


def test_every_status():
    q = [[0, 0, 0, 1], [0, 0, 1, 1], [0.1, 0, 1, 1]]
    out = _one_row(q, [0, 0, 0], fuse="mean")
    assert (out["slot_status"] == 0).all() and out["row_status"][0] == 0
    assert (out["spread"] >= 0).all() and (out["spread"] <= 8).all() and np.isfinite(out["R"]).all()
    out = _one_row(q, [0, -1, 5], fuse="mean")
    assert list(out["slot_status"][0]) == [0, M.NO_VIEW, 0] and np.isnan(out["rot_views"][0, 1]).all()
    assert np.isnan(out["spread"][0, 1]) and np.isfinite(out["spread"][0, [0, 2]]).all()
    for scene in (-1, 1):                                             # either side of the captures
        out = _one_row(q, [0, -1, 0], scene=scene, fuse="mean")
        assert (out["slot_status"] == M.NO_CAPTURE).all() and out["row_status"][0] == M.NO_ROTATION
        assert np.isnan(out["R"]).all() and np.isnan(out["spread"]).all() and np.isnan(out["rot_views"]).all()
        assert (out["pose"][0, :, 3] == [1, 2, 3, 1]).all() and (out["pose"][0, 3, :3] == 0).all()
    assert _one_row(q, [0, 0, 0], scene=7, scene_base=7)["row_status"][0] == 0
    out = _one_row([[0, 0, 0, 0], [np.nan, 0, 0, 1], [0, 0, 0, 1]], [0, 0, 0], fuse="mean")
    assert list(out["slot_status"][0]) == [M.DEGENERATE, M.DEGENERATE, 0] and out["row_status"][0] == 0
    assert M.same(out["R"][0], np.eye(3)) and out["spread"][0, 2] == 0
    # fuse="cam": the camera's own slot decides
    out = _one_row(q, [0, 0, -1], fuse="cam", cam=2)
    assert out["row_status"][0] == M.NO_ROTATION and np.isnan(out["R"]).all() and np.isnan(out["spread"]).all()
    out = _one_row(q, [-1, -1, 0], fuse="cam", cam=2)
    assert out["row_status"][0] == 0 and M.same(out["R"][0], out["rot_views"][0, 2]) and out["spread"][0, 2] == 0
    with pytest.raises(ValueError):
        _one_row(q[:2], [0, 0, 0], cams=[0, 1], fuse="cam", cam=2)
    out = _one_row(q, [-1, -1, -1], fuse="mean")
    assert out["row_status"][0] == M.NO_ROTATION
    # two views half a turn apart: no mean
    out = _one_row([[0, 0, 0, 1], [1, 0, 0, 0], [0, 0, 0, 1]], [0, 0, -1], fuse="mean")
    assert out["row_status"][0] == M.AMBIGUOUS and np.isfinite(out["R"]).all()
    assert abs(out["lam"][0, 0] - out["lam"][0, 1]) <= 2e-9


def test_spread_is_the_squared_frobenius_distance():
    rng = np.random.default_rng(8)
    raw = M.random_raw(rng, 4 * 5, "6d").reshape(5, 4, 6)
    rig = np.stack(make_rig(rng, 4)[1])[None]
    out = M.fuse_rotations(raw, np.zeros(5, np.int32), np.zeros((5, 4), np.int32), np.zeros((5, 3)), rig, "6d",
                           fuse="mean")
    want = ((out["rot_views"] - out["R"][:, None]) ** 2).sum(axis=(2, 3))
    assert np.abs(out["spread"] - want).max() <= 1e-14 and (out["spread"] <= 8).all()


def test_the_euler_filter():
    rng = np.random.default_rng(9)
    draw = rng.uniform(-6 * np.pi, 6 * np.pi, (20000, 3)).astype(np.float32)
    keep = M.euler_filter(draw)
    assert (~keep).mean() <= 0.01
    # the sine of a tiny float32 angle lies next to the angle itself, half an ulp from any boundary
    assert M.euler_filter(np.array([[1e-5, 0, 0]], np.float32)).all()
    assert len(M.random_raw(rng, 1000, "euler")) == 1000
