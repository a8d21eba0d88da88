"""tests/score_model.py against closed forms, its own second
statements and BOP's direct form -- no GPU."""
import numpy as np
import pytest

import score_model as M

# the model against mssd_direct on the random families below: the largest
# relative difference measured is 4.24e-16 (K = 2); the bound is the smallest
# power of two at least twice that, 2^-50 = 8.9e-16
DIRECT_BOUND = 2.0 ** -50


def one_pair(P, Q, verts, syms=None):
    out = M.score_poses(P[None], [0], Q[None], [0, 1], verts, syms)
    return {k: out[k][0, 0] for k in M.KEYS}


def test_equal_poses_give_zero():
    rng = np.random.default_rng(0)
    P = M.random_poses(rng, 1)[0]
    got = one_pair(P, P, rng.uniform(-50, 50, (9, 3)), M.z_symmetries(4))
    assert got["err"] == 0.0 and got["sym"] == 0 and got["t_err"] == 0.0
    assert abs(got["rot_cos"] - 1.0) <= 2.0 ** -50


def test_a_pure_translation_gives_its_length_for_any_vertices():
    rng = np.random.default_rng(1)
    P = M.random_poses(rng, 1)[0]
    for V in (1, 7, 300):
        Q = P.copy()
        Q[:3, 3] += rng.uniform(-100, 100, 3)
        e = P[:3, 3] - Q[:3, 3]
        want = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        got = one_pair(P, Q, rng.uniform(-1e3, 1e3, (V, 3)))
        assert got["err"] == want and got["t_err"] == want and got["sym"] == 0


def test_a_half_turn_about_z_is_a_symmetry():
    rng = np.random.default_rng(2)
    Q = M.random_poses(rng, 1)[0]
    half = np.diag([-1.0, -1.0, 1.0, 1.0])
    P = Q.copy()
    P[:3, :3] = Q[:3, :3] * np.array([-1.0, -1.0, 1.0])[None, :]          # Q's rotation times the half turn, exactly
    verts = rng.uniform(-50, 50, (12, 3))
    assert one_pair(P, Q, verts)["err"] > 10.0
    got = one_pair(P, Q, verts, np.stack([np.eye(4), half]))
    assert got["err"] == 0.0 and got["sym"] == 1 and got["t_err"] == 0.0
    assert abs(got["rot_cos"] - 1.0) <= 2.0 ** -50


def test_equal_symmetries_give_the_lower_index():
    rng = np.random.default_rng(3)
    P, Q = M.random_poses(rng, 2)
    verts = rng.uniform(-50, 50, (12, 3))
    S = M.z_symmetries(4)
    got = one_pair(P, Q, verts, S[[1, 2, 2, 1, 3]])
    alone = [one_pair(P, Q, verts, S[[k]])["err"] for k in (1, 2, 3)]
    best = int(np.argmin(alone))
    assert got["err"] == alone[best] and got["sym"] == (0, 1, 4)[best]
    got = one_pair(P, Q, verts, S[[2, 2]])
    assert got["sym"] == 0


def test_a_single_origin_vertex_gives_the_translation_error_bit_for_bit():
    rng = np.random.default_rng(4)
    P, G = M.random_poses(rng, 40), M.random_poses(rng, 40)
    out = M.score_poses(P, np.arange(40) // 10, G, [0, 10, 20, 30, 40], np.zeros((1, 3)))
    assert out["err"].shape == (40, 10) and np.isfinite(out["err"]).all()
    assert M.same(out["err"], out["t_err"])


def test_each_status_rule_and_their_order():
    rng = np.random.default_rng(5)
    P, G = M.random_poses(rng, 6), M.random_poses(rng, 5)
    P[1, 0, 0] = np.nan
    P[2, 3] = np.nan                                  # the bottom row is never read
    G[3, 1, 3] = 2.0 ** 200
    G[4, 2, 2] = -np.nextafter(2.0 ** 200, 0)        # the float64 below 2^200 passes
    scene = np.array([7, 7, 8, 9, 6, 10], np.int32)
    out = M.score_poses(P, scene, G, [0, 2, 2, 5], [[0.0, 0, 0]], scene_base=7)     # captures of 2, 0, 3 objects
    assert out["sym"].shape == (6, 3)
    assert out["sym"][0].tolist() == [0, 0, M.PADDING]
    assert out["sym"][1].tolist() == [M.NOT_FINITE, M.NOT_FINITE, M.PADDING]      # padding before the pose's NaN
    assert out["sym"][2].tolist() == [M.PADDING] * 3                               # an empty capture
    assert out["sym"][3].tolist() == [0, M.NOT_FINITE, 0]
    assert out["sym"][4].tolist() == out["sym"][5].tolist() == [M.NO_CAPTURE] * 3   # no capture before all else
    bad = out["sym"] < 0
    assert np.isposinf(out["err"][bad]).all() and np.isposinf(out["t_err"][bad]).all()
    assert np.isnan(out["rot_cos"][bad]).all()
    assert np.isfinite(out["err"][~bad]).all() and np.isfinite(out["rot_cos"][~bad]).all()
    P[4, 0, 0] = np.inf                               # a pose that is not finite in a row of no capture: still -2
    assert (M.score_poses(P, scene, G, [0, 2, 2, 5], [[0.0, 0, 0]], scene_base=7)["sym"][4] == M.NO_CAPTURE).all()
    part = M.score_poses(P, scene, G, [0, 2, 2, 5], [[0.0, 0, 0]], rows=(2, 4), scene_base=7)
    assert all(M.same(part[k], out[k][2:4]) for k in M.KEYS)


def random_match_case(rng):
    S = int(rng.integers(0, 5))
    rows, gts = rng.integers(0, 6, S), rng.integers(0, 5, S)
    row_offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64) + int(rng.integers(0, 2))
    gt_offs = np.concatenate([[0], np.cumsum(gts)]).astype(np.int64)
    n, G = int(row_offs[-1]) + int(rng.integers(0, 3)), int(rng.integers(1, 6))
    err = rng.integers(0, 6, (n, G)).astype(np.float64)              # many ties
    err[rng.random((n, G)) < 0.15] = np.inf
    err[rng.random((n, G)) < 0.05] = np.nan
    thresholds = rng.choice([0.0, 1.0, 2.5, 4.0, 5.0, np.inf], int(rng.integers(1, 4)))
    return err, row_offs, gt_offs, thresholds


def test_the_two_greedy_statements_agree():
    rng = np.random.default_rng(6)
    hits = 0
    for _ in range(500):
        case = random_match_case(rng)
        a, b = M.match_scores(*case), M.match_scores_loop(*case)
        assert M.same(a[0], b[0]) and M.same(a[1], b[1])
        assert a[0].shape == (len(case[3]), len(case[0])) and a[1].shape == (len(case[3]), len(case[1]) - 1)
        hits += int(a[1].sum())
    assert hits > 1000


def _match(err, thresholds, rows=None, gts=None):
    err = np.asarray(err, np.float64)
    row_offs = [0, len(err)] if rows is None else rows
    gt_offs = [0, err.shape[1]] if gts is None else gts
    a, b = M.match_scores(err, row_offs, gt_offs, thresholds), M.match_scores_loop(err, row_offs, gt_offs, thresholds)
    assert M.same(a[0], b[0]) and M.same(a[1], b[1])
    return a[0].tolist(), a[1].tolist()


def test_greedy_is_not_the_optimal_assignment():
    # row 0 takes object 0 (1 < 2) and leaves row 1 nothing; the optimal assignment matches both
    assert _match([[1.0, 2.0], [1.5, 9.0]], [5.0]) == ([[0, -1]], [[1]])


def test_the_comparison_with_the_threshold_is_strict():
    e = 3.7
    assert _match([[e]], [e, np.nextafter(e, np.inf), np.inf, 0.0]) == ([[-1], [0], [0], [-1]], [[0], [1], [1], [0]])
    assert _match([[0.0]], [0.0]) == ([[-1]], [[0]])
    assert _match([[np.inf, np.nan]], [np.inf]) == ([[-1]], [[0]])


def test_equal_errors_take_the_lowest_object():
    assert _match([[2.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]], [1.5]) == ([[1, 0]], [[2]])


def test_a_later_row_loses_its_best_object_to_an_earlier_one():
    assert _match([[1.0, 3.0], [0.5, 2.0], [0.1, 0.2]], [5.0]) == ([[0, 1, -1]], [[2]])


def test_empty_captures_on_either_side_and_rows_no_capture_owns():
    err = np.ones((5, 2))
    # rows 1-2 against no object, no row against two objects, rows 3-3 (none) against one; rows 0 and 4 unowned
    gi, tp = _match(err, [5.0], rows=[1, 3, 3, 3, 4], gts=[0, 0, 2, 3, 5])
    assert gi == [[-1, -1, -1, 0, -1]] and tp == [[0, 0, 0, 1]]
    assert _match(np.ones((0, 1)), [1.0], rows=[0], gts=[0]) == ([[]], [[]])
    # a count past the columns err holds is cut to them
    assert _match(err, [5.0], rows=[0, 5], gts=[0, 7]) == ([[0, 1, -1, -1, -1]], [[2]])
    r, p = M.recall_precision(np.array([[0, 0, 0, 1]]), [1, 3, 3, 3, 4], [0, 0, 2, 3, 5])
    assert r.tolist() == [0.2] and p.tolist() == [1 / 3]


@pytest.mark.parametrize("K", (1, 2, 8))
def test_the_model_against_the_direct_form(K):
    rng = np.random.default_rng(10 + K)
    n, G, worst = 100, 3, 0.0
    syms = M.z_symmetries(K)
    syms[1:, :3, 3] = rng.uniform(-1e3, 1e3, (K - 1, 3))
    P, Q = M.random_poses(rng, n), M.random_poses(rng, n * G)
    verts = rng.uniform(-1e3, 1e3, (257, 3))
    out = M.score_poses(P, np.arange(n), Q, np.arange(n + 1) * G, verts, syms)
    for r in range(n):
        for g in range(G):
            want = M.mssd_direct(P[r], Q[r * G + g], verts, syms)
            worst = max(worst, abs(out["err"][r, g] - want) / want)
    print(f"K={K}: largest relative difference to mssd_direct {worst:.3e}")
    assert worst <= DIRECT_BOUND
