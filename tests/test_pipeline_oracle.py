"""Pin the CPU restatement of _detect's packing and of triangulate_multi_view
(oracle/pipeline.py) against the reference's own outputs (a8, a9 fixtures),
and its threshold + stable sort (select_sort) against the restated
match_objects (oracle/lsap.py) on the a7 captures and the a3 cubes."""
import numpy as np
import pytest

from oracle import lsap, pipeline


def test_detect_pack_matches_reference(golden):
    z = golden("a8_detect.npz")
    for c in range(int(z["n"])):
        bbox, center, offs = pipeline.detect_pack(z[f"d{c}_boxes"], z[f"d{c}_conf"], z[f"d{c}_cls"],
                                                  z[f"d{c}_in_offs"], float(z[f"d{c}_thresh"]))
        np.testing.assert_array_equal(offs, z[f"d{c}_out_offs"])
        np.testing.assert_array_equal(bbox, z[f"d{c}_bbox"])
        assert center.dtype == np.float64
        np.testing.assert_array_equal(center, z[f"d{c}_center"])


def test_detect_fixture_covers_edges(golden):
    """The fixture exercises what the kernel must get right: confidences equal
    to the float32 threshold and one ulp below, negative fractional coordinates
    (int() truncates toward zero), empty images, foreign classes."""
    z = golden("a8_detect.npz")
    seen_eq = seen_below = seen_neg = seen_empty = seen_cls = False
    for c in range(int(z["n"])):
        t32 = np.float32(float(z[f"d{c}_thresh"]))
        conf, boxes, cls = z[f"d{c}_conf"], z[f"d{c}_boxes"], z[f"d{c}_cls"]
        seen_eq |= bool(np.any(conf == t32))
        seen_below |= bool(np.any(conf == np.nextafter(t32, np.float32(-1))))
        seen_neg |= bool(np.any((boxes < 0) & (boxes > -1)))
        seen_empty |= bool(np.any(np.diff(z[f"d{c}_in_offs"]) == 0))
        seen_cls |= bool(np.any(cls != 0))
    assert seen_eq and seen_below and seen_neg and seen_empty and seen_cls


def _assert_select_sort_equals_match_objects(cube, thr, tag):
    N, M, P = cube.shape
    rows, cols = lsap.linear_sum_assignment(cube.reshape(N * M, P))
    match, cost = pipeline.select_sort(cube.reshape(-1), M, P, rows, cols, thr)
    ref = sorted(lsap.match_objects(cube, thr), key=lambda m: cube[m])
    assert match.dtype == np.int32 and cost.dtype == np.float32
    np.testing.assert_array_equal(match, np.asarray(ref, np.int32).reshape(-1, 3), err_msg=str(tag))
    np.testing.assert_array_equal(cost.view(np.int32),
                                  np.asarray([cube[m] for m in ref], np.float32).view(np.int32),
                                  err_msg=str(tag))
    return len(ref)


@pytest.mark.parametrize("thr", [30, np.inf])
def test_select_sort_equals_sorted_match_objects(golden, thr):
    """select_sort (the checker of the GPU select tail) is the reference's
    sorted(match_objects(cube, thr), key=cost) on every a7 capture's cube
    (oracle cube of the stored centres) and on the a3 cubes."""
    from bpc_baseline_amd.inference.utils.camera_utils import camera_pairs, fundamental_matrices
    from oracle import oracle as O
    z = golden("a7_match.npz")
    kept = 0
    for c in range(int(z["n"])):
        views = [np.asarray(z[f"m{c}_pts{cam}"], np.float64).reshape(-1, 2) for cam in range(3)]
        co = np.zeros(4, np.int64)
        np.cumsum([len(v) for v in views], out=co[1:])
        F = fundamental_matrices(list(z[f"m{c}_K"]), list(z[f"m{c}_RT"]), camera_pairs(3))
        cube = O.cube(np.concatenate(views), co, F, 1)[0].reshape(np.diff(co))
        n = _assert_select_sort_equals_match_objects(cube, thr, ("a7", c))
        if thr == 30:        # and that is what the reference's _match kept
            assert n == z[f"m{c}_t"].shape[0], c
        kept += n
    g = golden("a3_cost_cubes.npz")
    for name in g["names"]:
        kept += _assert_select_sort_equals_match_objects(g[f"{name}_cube"], thr, ("a3", name))
    assert kept > 0


def _edge_cube():
    """One cost equal to float32(0.7), which is below 0.7 in float64 (float32
    rounds 0.7 down), and one a float32 ulp above it."""
    lo = np.float32(0.7)
    hi = np.nextafter(lo, np.float32(1))
    assert float(lo) < 0.7 < float(hi)
    # rows (i, j) = (0, 0), (0, 1); the assignment is the diagonal
    return np.array([[[lo, 50.0], [50.0, hi]]], np.float32), lo, hi


def test_threshold_compares_in_float64():
    """The documented contract (include/mvmatch.h): cost < threshold in
    float64.  A float32 compare (NumPy >= 2 on a float32 scalar and a Python
    float) rounds 0.7 down to the first cost and drops it."""
    cube, lo, hi = _edge_cube()
    assert lsap.match_objects(cube, 0.7) == [(0, 0, 0)]
    rows, cols = lsap.linear_sum_assignment(cube.reshape(2, 2))
    match, cost = pipeline.select_sort(cube.reshape(-1), 2, 2, rows, cols, 0.7)
    np.testing.assert_array_equal(match, [[0, 0, 0]])
    np.testing.assert_array_equal(cost.view(np.int32), np.array([lo]).view(np.int32))
    # a float64 threshold between the two keeps the same; at float(lo), strict <
    assert lsap.match_objects(cube, float(hi)) == [(0, 0, 0)]
    assert lsap.match_objects(cube, float(lo)) == []
    assert pipeline.select_sort(cube.reshape(-1), 2, 2, rows, cols, float(lo))[0].shape == (0, 3)


def test_dropin_match_objects_threshold_in_float64(monkeypatch):
    """The drop-in's own host-side compare follows the same contract (its
    assignment, a GPU call, replaced by the restated solver here)."""
    from bpc_baseline_amd.inference import epipolar_matching as em
    monkeypatch.setattr(em, "linear_sum_assignment", lsap.linear_sum_assignment)
    cube, lo, hi = _edge_cube()
    assert [tuple(int(x) for x in m) for m in em.match_objects(cube, 0.7)] == [(0, 0, 0)]
    assert [tuple(int(x) for x in m) for m in em.match_objects(cube, float(hi))] == [(0, 0, 0)]
    assert em.match_objects(cube, float(lo)) == []
    assert len(em.match_objects(cube, 51)) == 2


def test_triangulate_matches_reference(golden):
    z = golden("a9_triangulate.npz")
    for V in (2, 3, 4, 8):
        X = pipeline.triangulate(z[f"v{V}_proj"], z[f"v{V}_pts"])
        np.testing.assert_allclose(X, z[f"v{V}_X"], rtol=1e-12, atol=1e-9)


def test_triangulate_matches_match_fixture(golden):
    """PosePrediction.t of the reference's _match runs (a7)."""
    z = golden("a7_match.npz")
    for c in range(int(z["n"])):
        cent = z[f"m{c}_centroids"]
        if cent.shape[0] == 0:
            continue
        P = np.stack([z[f"m{c}_K"][v] @ z[f"m{c}_RT"][v][:3] for v in range(3)])
        proj = np.broadcast_to(P, (cent.shape[0], 3, 3, 4))
        X = pipeline.triangulate(proj, cent)
        np.testing.assert_allclose(X, z[f"m{c}_t"], rtol=1e-12, atol=1e-9)
