"""The rotation fusion on the GPU where the mean is hard: the
inputs of tests/pose_edges.py -- the cube group's exact ties, a sum of exactly
zero, views next to half a turn apart either side of the ambiguity threshold,
a double largest eigenvalue, uniform rotations over all of SO(3), the decoders'
extremes, rigs that are not finite -- against tests/pose_model.py bit for bit,
with the checks of tests/test_pose_gpu.py: every output pre-filled with
sentinels between guard rows and compared whole, NaN equal to NaN, the inputs
unchanged.  tests/test_pose_edges_model.py pins on the CPU that these inputs
are where they claim to be; here the statuses are read off the model's result,
which the device has just returned to the bit, so it took those paths."""
import numpy as np
import pytest

import pose_edges as E
import pose_model as M
from test_pose_gpu import check

pytestmark = pytest.mark.gpu


def _mean(t, dev):
    return check(t, dev, (0, t.n), range(t.C), "mean")


def test_the_cube_group(cuda):
    """The zero-skip of the Jacobi rotations, the lowest-index tie of the
    largest eigenvalue, the magnitude tie of the sign rule, half-turn
    quaternions with w = 0."""
    t = E.cube_rows()
    want = _mean(t, cuda)
    amb = want["row_status"] == M.AMBIGUOUS
    for k in (2, 3, 4):
        rows = t.tags["size"] == k
        assert amb[rows].any() and not amb[rows].all()
    assert (want["lam"][amb, 0] == want["lam"][amb, 1]).any()
    want = check(t, cuda, (0, t.n), range(4), "cam", cam=2)
    assert set(want["row_status"]) == {0, M.NO_ROTATION}


def test_a_sum_of_exactly_zero(cuda):
    want = _mean(E.zero_sum(), cuda)
    assert (want["row_status"] == M.AMBIGUOUS).all() and (want["lam"] == 0).all()
    assert M.same(want["R"][0], np.diag([1.0, -1.0, -1.0])) and M.same(want["R"][1], want["R"][0])


def test_near_a_half_turn(cuda):
    t = E.half_turn()
    want = _mean(t, cuda)
    for d in E.DELTAS:
        assert (want["row_status"][t.tags["delta"] == d] == (0 if d >= 1e-9 else M.AMBIGUOUS)).all(), d


def test_the_threshold_counts_used_slots(cuda):
    want = _mean(E.used_not_selected(), cuda)
    assert list(want["row_status"]) == [0, M.AMBIGUOUS] and list((want["slot_status"] == 0).sum(axis=1)) == [2, 6]


def test_a_double_largest_eigenvalue(cuda):
    t = E.symmetric()
    want = _mean(t, cuda)
    assert (want["row_status"] == np.where(t.tags["exact"], M.AMBIGUOUS, 0)).all()


def test_wide_spreads(cuda):
    want = _mean(E.wide(), cuda)
    assert (want["row_status"] == 0).all() and set((want["slot_status"] == 0).sum(axis=1)) == {2, 3, 4, 8}


@pytest.mark.parametrize("fuse", ("mean", "cam"))
@pytest.mark.parametrize("mode", ("euler", "quat", "6d"))
def test_decode_extremes(cuda, mode, fuse):
    t = E.decode_extremes(mode)
    want = check(t, cuda, (0, t.n), range(3), fuse)
    if mode == "euler":
        assert (want["slot_status"] == 0).all() and (want["row_status"] == 0).all()
    else:
        finite = t.tags["finite"]
        assert ((want["slot_status"] == 0) == finite[:, None]).all() and finite.any() and not finite.all()
        assert ((want["row_status"] & M.NO_ROTATION) == 0).tolist() == finite.tolist()


@pytest.mark.parametrize("kind", E.RIG_KINDS + E.RIG_BOUND_KINDS)
def test_rigs_that_are_not_finite(cuda, kind):
    """A NaN, an infinity, 1e308 or -2^500 in one camera's rotation block costs
    that camera's slots and nothing else; a NaN where nothing reads, or the
    float64 below 2^500, costs nothing."""
    t = E.bad_rig(kind)
    usable = kind in ("translation", "below_max")
    want = _mean(t, cuda)
    bad = want["slot_status"][:, E.BAD_CAM]
    assert (bad == (0 if usable else M.DEGENERATE)).all() and (want["row_status"] != M.NO_ROTATION).all()
    assert np.isfinite(want["R"]).all()
    want = check(t, cuda, (0, t.n), range(4), "cam", cam=E.BAD_CAM)
    assert (want["row_status"] == (0 if usable else M.NO_ROTATION)).all()
    want = check(t, cuda, (0, t.n), (3, 0, 1), "mean")                  # the bad camera deselected
    assert (want["slot_status"] == 0).all()
    check(t, cuda, (0, t.n), range(4), "cam", cam=0)
