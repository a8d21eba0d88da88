"""The inputs of tests/pose_edges.py are where they claim to be:
what tests/pose_model.py makes of each family -- the statuses, the eigenvalue
gaps either side of the ambiguity threshold, the decoders' finite / not-finite
split -- its orthonormality, its distance to the SVD statement of the mean over
all of SO(3), and the promises a result keeps whatever its inputs hold.  CPU.

SVD_PRODUCT: |R - R_svd|_max . (lam1 - lam2) / n_used over every non-ambiguous
row of the cube group, the near-half-turn pairs, the symmetric triples and the
uniform sets (3,882 rows) peaked at 8.83e-15, in the uniform sets; the cube
group gave 4.22e-15, the pairs 5.0e-16, the triples 2.2e-16 (measured against
``mean_rotation_svd``, numpy's SVD).  The bound is 2^-45 = 2.84e-14, the
smallest power of two at least twice the maximum, as the bounds of
tests/test_pose_model.py were set."""
import numpy as np
import pytest

import pose_edges as E
import pose_model as M
import test_pose_gpu as gpu

SVD_PRODUCT = 2.0 ** -45                                  # 2.8e-14
GAP = M.AMBIGUOUS_GAP


def _gap(out):
    return out["lam"][:, 0] - out["lam"][:, 1]


@pytest.fixture(scope="module")
def means():
    return {name: t.model("mean") for name, t in E.mean_tables().items()}


def test_the_cube_group_reaches_every_status(means):
    t, out = E.cube_rows(), means["cube"]
    size, amb = t.tags["size"], out["row_status"] == M.AMBIGUOUS
    assert len(E.cube_group()) == 24 and (np.bincount(size)[1:] == (24, 276, 2024, 1000)).all()
    counts = [int(amb[size == k].sum()) for k in (1, 2, 3, 4)]
    print("ambiguous singles, pairs, triples, quadruples:", counts)
    assert counts[0] == 0 and min(counts[1:]) > 0
    assert set(out["row_status"]) == {0, M.AMBIGUOUS} and set(out["slot_status"].reshape(-1)) == {0, M.NO_VIEW}
    # the 6-D rule decodes the group exactly, so the views are the group's
    assert M.same(out["rot_views"][size == 4], E.cube_group()[t.tags["idx"][size == 4]])
    # a single rotation is its own mean; half-turn quaternions (w = 0) among them
    assert np.abs(out["R"][size == 1] - E.cube_group()).max() <= 4 * np.spacing(1.0)
    # exact ties did occur: rows whose two largest eigenvalues are equal to the bit
    assert (_gap(out)[amb] == 0).any()


def test_a_sum_of_exactly_zero(means):
    out = means["zero_sum"]
    assert list(out["slot_status"][1]) == [0, M.NO_VIEW, M.NO_VIEW, M.NO_VIEW] and (out["slot_status"][0] == 0).all()
    assert (out["rot_views"][0].sum(axis=0) == 0).all() and (out["rot_views"][1, 0] == 0).all()
    assert (out["row_status"] == M.AMBIGUOUS).all() and (out["lam"] == 0).all()
    for r in range(2):                        # every pair skipped, the power step zero: the first unit vector kept
        assert M.same(out["R"][r], np.diag([1.0, -1.0, -1.0]))


def test_near_a_half_turn_either_side_of_the_threshold(means):
    t, out = E.half_turn(), means["half_turn"]
    delta, gap = t.tags["delta"], _gap(out)
    assert ((out["slot_status"] == 0).sum(axis=1) == 2).all()                       # n_used = 2
    for d in E.DELTAS:
        rows = delta == d
        print(f"delta {d:g}: gap {gap[rows].min():.4g} .. {gap[rows].max():.4g}")
        if d >= 1e-9:
            assert (gap[rows] > GAP * 2).all() and (out["row_status"][rows] == 0).all()
            assert np.abs(gap[rows] / (4 * d) - 1).max() <= 1e-2                    # the gap is about 4 delta
        else:
            assert (gap[rows] <= GAP * 2).all() and (out["row_status"][rows] == M.AMBIGUOUS).all()
    assert 2e-9 < gap[delta == 1e-9].min() and gap[delta == 1e-9].max() < 8e-9      # family d builds on this


def test_the_threshold_counts_used_slots_not_selected_ones(means):
    out = means["used_not_selected"]
    gap, n_used, n_sel = _gap(out), (out["slot_status"] == 0).sum(axis=1), out["slot_status"].shape[1]
    print("gaps", gap, "used", n_used)
    assert list(n_used) == [2, 6] and n_sel == 8
    assert {M.NO_VIEW, M.DEGENERATE} <= set(out["slot_status"][0]) and {M.NO_VIEW, M.DEGENERATE} <= set(
        out["slot_status"][1])
    assert GAP * 2 < gap[0] <= GAP * n_sel and out["row_status"][0] == 0            # the selected count would flag it
    assert GAP * 2 < gap[1] <= GAP * 6 and out["row_status"][1] == M.AMBIGUOUS      # the first row's count would not
    # the selected count is never below the used one, so it cannot clear a row: the second row pins the
    # count from below instead (a rule that stopped at the first row's 2 would clear it)
    assert not gap[1] <= GAP * 2


def test_a_double_largest_eigenvalue(means):
    t, out = E.symmetric(), means["symmetric"]
    exact = t.tags["exact"]
    assert (out["row_status"][exact] == M.AMBIGUOUS).all() and (out["row_status"][~exact] == 0).all()
    assert np.abs(out["lam"][exact] - 3).max() <= 1e-14
    assert np.abs(_gap(out)[~exact] / 4e-6 - 1).max() <= 1e-3 and (_gap(out)[~exact] > GAP * 3).all()


def test_wide_spreads_cover_their_slot_counts(means):
    out = means["wide"]
    n_used = (out["slot_status"] == 0).sum(axis=1)
    assert (np.bincount(n_used, minlength=9)[[2, 3, 4, 8]] == 200).all() and (out["row_status"] == 0).all()
    # the views of a row are far apart: the largest pairwise angle is beyond 90 degrees in most rows
    W = np.where((out["slot_status"] == 0)[:, :, None, None], out["rot_views"], 0.0)
    tr = np.einsum("rkij,rlij->rkl", W, W)
    tr = np.where((out["slot_status"] == 0)[:, :, None] & (out["slot_status"] == 0)[:, None, :], tr, 3.0)
    assert (tr.min(axis=(1, 2)) < 1.0).mean() > 0.75                                # tr = 1 + 2 cos(angle)


def test_orthonormal_wherever_a_rotation_is_written(means):
    worst = 0.0
    for name, out in means.items():
        R = out["R"][out["row_status"] != M.NO_ROTATION]
        assert len(R) == len(out["R"]) and np.isfinite(R).all(), name
        worst = max(worst, np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max(), np.abs(np.linalg.det(R) - 1).max())
    print("R^T R - I and det R - 1, largest:", worst)
    assert worst <= 1e-14


def test_the_mean_is_the_svd_mean_over_all_of_so3(means):
    worst, rows = 0.0, 0
    for name in ("cube", "half_turn", "symmetric", "wide"):
        out = means[name]
        used, gap = out["slot_status"] == 0, _gap(out)
        peak = 0.0
        for r in np.nonzero(out["row_status"] == 0)[0]:
            ref = M.mean_rotation_svd(out["rot_views"][r][used[r]])
            peak = max(peak, np.abs(out["R"][r] - ref).max() * gap[r] / used[r].sum())
            rows += 1
        print(f"{name}: |R - R_svd| . gap / n_used peaks at {peak:.3g}")
        worst = max(worst, peak)
    print(f"{rows} rows, largest product {worst:.3g}, bound {SVD_PRODUCT:.3g}")
    assert rows > 3500 and worst <= SVD_PRODUCT


@pytest.mark.parametrize("fuse", ("mean", "cam"))
def test_what_a_result_promises(fuse):
    """On every table of tests/pose_edges.py and of the GPU tests' ``Case``."""
    for name, t in E.all_tables().items():
        M.invariants(t.model(fuse))
    for n, C, mode in ((257, 3, "euler"), (513, 4, "quat"), (257, 8, "6d"), (5, 4, "6d"), (1, 3, "quat")):
        c = gpu.case(n, C, mode)
        M.invariants(gpu.expected(c, (0, n), range(C), fuse))


@pytest.mark.parametrize("kind", E.RIG_KINDS[:4])
def test_a_rig_that_is_not_finite_costs_one_slot(kind, means):
    t, clean, out = E.bad_rig(kind), E.bad_rig("clean"), means[f"rig_{kind}"]
    bad, others = E.BAD_CAM, [c for c in range(4) if c != E.BAD_CAM]
    assert not (np.abs(t.RTs[0, bad, :3, :3]) < M.WORLD_MAX).all() and M.same(t.raw, clean.raw)
    assert (out["slot_status"][:, bad] == M.DEGENERATE).all() and (out["slot_status"][:, others] == 0).all()
    assert np.isnan(out["rot_views"][:, bad]).all() and np.isnan(out["spread"][:, bad]).all()
    assert (out["row_status"] == 0).all() and np.isfinite(out["R"]).all()
    M.invariants(out)
    # the mean is the mean with that camera deselected, bit for bit, and the other slots are the clean rig's
    without = t.model("mean", cams=others)
    for k in ("R", "pose", "row_status", "lam"):
        assert M.same(out[k], without[k]), k
    ref = clean.model("mean")
    assert M.same(out["rot_views"][:, others], ref["rot_views"][:, others])
    assert M.same(out["spread"][:, others], without["spread"]) and M.same(without["R"], clean.model("mean", cams=others)["R"])
    cam = t.model("cam", cam=bad)
    assert (cam["row_status"] == M.NO_ROTATION).all() and np.isnan(cam["R"]).all() and np.isnan(cam["spread"]).all()
    M.invariants(cam)
    good = t.model("cam", cam=0)
    assert M.same(good["R"], clean.model("cam", cam=0)["R"]) and (good["row_status"] == 0).all()


def test_either_side_of_the_largest_world_entry(means):
    """An entry of -2^500 makes the slot degenerate; the float64 below 2^500
    leaves it usable, and everything written stays finite."""
    at, below = means["rig_at_max"], means["rig_below_max"]
    assert (at["slot_status"][:, E.BAD_CAM] == M.DEGENERATE).all() and (below["slot_status"] == 0).all()
    assert (below["rot_views"][:, E.BAD_CAM, 0, 0] == np.nextafter(M.WORLD_MAX, 0.0)).all()
    assert (E.bad_rig("at_max").RTs[0, E.BAD_CAM, 0, 0] == -M.WORLD_MAX)
    for out in (at, below, E.bad_rig("below_max").model("cam"), E.bad_rig("at_max").model("cam")):
        M.invariants(out)
    assert np.isfinite(below["spread"]).all() and below["spread"][:, E.BAD_CAM].min() > 2.0 ** 990


def test_the_translation_and_bottom_row_are_never_read():
    t, clean = E.bad_rig("translation"), E.bad_rig("clean")
    assert np.isnan(t.RTs).sum() == 7 and np.isfinite(t.RTs[:, :, :3, :3]).all()
    for fuse in ("mean", "cam"):
        got, want = t.model(fuse), clean.model(fuse)
        for k in want:
            assert M.same(got[k], want[k]), (fuse, k)
        assert (got["slot_status"] == 0).all() and (got["row_status"] == 0).all()


@pytest.mark.parametrize("mode", ("quat", "6d"))
def test_the_decoders_finite_split(mode):
    t = E.decode_extremes(mode)
    m = M.decode(t.raw[:, 0], mode)
    finite = np.isfinite(m).all(axis=(1, 2))
    for r in range(t.n):
        assert finite[r] == t.tags["finite"][r], (mode, tuple(t.raw[r, 0]))
    out = t.model("mean")
    assert ((out["slot_status"] == 0) == finite[:, None]).all() and ((out["slot_status"] == M.DEGENERATE) == ~finite[:, None]).all()
    det = np.linalg.det(m[finite].astype(np.float64))
    if mode == "quat":
        assert abs(det[0] - 1) <= 1e-6
    else:   # finite, status 0, no rotation: the determinant is 0, or 0.017 for the collinear pair
        assert (det[:6] == 0).all() and abs(det[6] - 0.017) <= 1e-3
        assert (out["row_status"][finite] != M.NO_ROTATION).all() and np.isfinite(out["R"][finite]).all()
        assert M.same(m[3], np.zeros((3, 3), np.float32))


def test_the_euler_extremes():
    t = E.decode_extremes("euler")
    n_edge = t.tags["n_edge"]
    edge = E.euler_edge_angles()
    assert n_edge == 4 * len(edge) and t.n == n_edge + 200 * len(E.EULER_SCALES)
    assert M.euler_filter(t.raw[:, 0]).all() and np.isfinite(t.raw).all()
    w = M.wrap_euler(edge)
    assert (np.abs(w) <= M.PI32).all()
    fmax = np.finfo(np.float32).max
    assert w[list(edge).index(fmax)] == np.float32(-1.4096296)
    assert w[list(edge).index(M.PI32)] == -M.PI32 and abs(w[list(edge).index(M.TWO_PI32)]) <= 1e-6
    for i, scale in enumerate(E.EULER_SCALES):                                     # many turns out, as claimed
        rows = t.raw[n_edge + 200 * i:n_edge + 200 * (i + 1), 0]
        assert np.abs(rows).max() <= scale and np.median(np.abs(rows)) > scale / 4
    out = t.model("mean")
    assert (out["slot_status"] == 0).all() and (out["row_status"] == 0).all()
    m = M.decode(t.raw[:, 0], "euler").astype(np.float64)
    assert np.abs(np.swapaxes(m, 1, 2) @ m - np.eye(3)).max() <= 2.0 ** -21
