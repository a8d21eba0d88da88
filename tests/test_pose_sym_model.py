"""tests/pose_sym_model.py, the statement of the mean under symmetries (DESIGN
§3.21), proved on the CPU: against ``pose_model.fuse_rotations`` with the
identity alone, in closed form on the cube group, against a brute force over
every assignment, and on the families of tests/pose_sym_edges.py that
tests/test_pose_sym_gpu.py sends to the device."""
from itertools import product

import numpy as np
import pytest

import pose_edges as E
import pose_model as P
import pose_sym_edges as SE
import pose_sym_model as M
from bpc_baseline_amd.synth import make_rig

ULP = 2.0 ** -52
# brute force against the model: the largest entry difference measured over the cases below is 1.72e-15 (n = 2..4
# views, K = 2 and 4, 40 rows each); the smallest power of two at least twice it
BRUTE_BOUND = 2.0 ** -48


def group_distance(R, T, S):
    """min over k of the largest entry of |R - T S_k|."""
    return min(np.abs(R - T @ S[k, :3, :3]).max() for k in range(len(S)))


@pytest.mark.parametrize("mode", ("euler", "quat", "6d"))
def test_the_identity_alone_is_the_plain_mean(mode):
    rng = np.random.default_rng(7 + P.MODES[mode][0])
    n, C, S = 300, 8, 3
    raw = P.random_raw(rng, n * C, mode).reshape(n, C, -1)
    views = rng.integers(0, 40, (n, C)).astype(np.int32)
    views[rng.random((n, C)) < 0.2] = -1
    scene = (np.arange(n) % (S + 1)).astype(np.int32)             # every fourth row has no capture
    X = rng.uniform(-300, 300, (n, 3))
    RTs = np.stack([np.stack(make_rig(rng, C)[1]) for _ in range(S)]).astype(np.float64)
    for K in range(2, 9):
        cams = [int(c) for c in rng.permutation(C)[:K]]
        want = P.fuse_rotations(raw[:, cams], scene, views, X, RTs, mode, cams=cams, fuse="mean")
        for rounds in (1, 2, 4):
            got = M.fuse_rotations_sym(raw[:, cams], scene, views, X, RTs, mode, np.eye(4)[None], cams=cams,
                                       rounds=rounds)
            for k in ("R", "pose", "spread", "rot_views", "slot_status", "row_status", "lam"):
                assert P.same(got[k], want[k]), (k, K, rounds)          # -0 == +0: numbers, not bits
            assert (got["sym_index"] == np.where(want["slot_status"] == 0, 0, -1)).all()
            assert np.isposinf(got["sym_margin"][want["slot_status"] == 0]).all()
            assert (got["n_changed"] == 0).all()
            M.invariants(got)


def test_cube_views_fuse_to_the_first_view():
    t, syms = SE.cube_views()
    G = E.cube_group()
    for rounds in (1, 2, 3):
        out = SE.model(t, syms, rounds)
        assert (out["row_status"] == 0).all() and (out["slot_status"] == 0).all()
        assert np.abs(out["R"] - G[t.tags["first"]]).max() <= 4 * ULP        # §3.19's figure for copies of one rotation
        assert out["spread"].max() <= 9 * (4 * ULP) ** 2
        assert (out["sym_index"] == t.tags["sym"]).all() and (out["n_changed"] == 0).all()
        assert (out["rot_views"] == G[t.tags["first"]][:, None]).all()
        assert (out["sym_margin"] >= 2 - 1e-12).all()                        # traces of cube rotations: 3, then <= 1
        M.invariants(out)
    # what the feature is for: the plain mean of the same rows is no answer
    plain = t.model(fuse="mean")
    mixed = (t.tags["sym"] != 0).any(axis=1)
    far = np.array([min(np.abs(plain["R"][r] - g).max() for g in G) > 0.1 for r in range(t.n)])
    lost = (((plain["row_status"] & P.AMBIGUOUS) != 0) | far)[mixed]
    print(f"plain mean ambiguous or > 0.1 from every R G_k: {lost.sum()} of {mixed.sum()} mixed rows")
    # not all of them: outliers that balance (one half turn, +90 and -90 degrees) cancel in the plain sum
    assert mixed.sum() > 300 and lost.sum() >= 0.8 * mixed.sum()         # 359 of 400


def test_a_duplicated_element_gives_the_lower_index_and_no_margin():
    t, syms = SE.duplicated()
    out = SE.model(t, syms)
    need = (-t.tags["k"] + t.tags["k"][:, :1]) % 4                 # the quarter turns back to the first view
    assert (out["sym_index"] == np.array([0, 1, 3, 4])[need]).all()
    dup = (need == 1) | (need == 3)
    assert dup.sum() > 50 and (out["sym_margin"][dup] == 0.0).all() and (out["sym_margin"][~dup] > 0.5).all()
    M.invariants(out)


def brute_force(W, S):
    """The best of all K^(n-1) assignments (the first view keeps the
    identity): the SVD mean with the smallest summed squared distance."""
    best, best_R = np.inf, None
    for assign in product(range(len(S)), repeat=len(W) - 1):
        Ws = [W[0]] + [W[c + 1] @ S[a, :3, :3] for c, a in enumerate(assign)]
        R = P.mean_rotation_svd(Ws)
        cost = sum(((w - R) ** 2).sum() for w in Ws)
        if cost < best:
            best, best_R = cost, R
    return best_R


def test_against_a_brute_force_over_every_assignment():
    worst = 0.0
    for fold, noise in ((4, 10.0), (2, 10.0)):
        for C in (2, 3, 4):
            t, syms = SE.z_views(np.random.default_rng(50 + 10 * fold + C), 40, C, fold, noise)
            out = SE.model(t, syms)
            assert (out["row_status"] == 0).all() and (out["n_changed"] == 0).all()
            for r in range(t.n):
                worst = max(worst, group_distance(out["R"][r], brute_force(t.tags["W"][r], syms), syms))
    print(f"largest entry difference to the brute force: {worst:.3g}")
    assert worst <= BRUTE_BOUND and BRUTE_BOUND < 4 * worst


def z_angle_to_truth(R, R0):
    """The angle in degrees of R0^T R about z, folded into -45 .. 45."""
    D = R0.T @ R
    return (np.degrees(np.arctan2(D[1, 0], D[0, 0])) + 45.0) % 90.0 - 45.0


def test_the_second_round_moves_a_view_near_the_boundary():
    t, syms = SE.round_two()
    one, two, three = (SE.model(t, syms, rounds) for rounds in (1, 2, 3))
    assert (one["n_changed"] == 0).all()
    assert (two["n_changed"] == 1).all() and (three["n_changed"] == 0).all()
    assert (two["sym_index"] != one["sym_index"]).sum(axis=1).tolist() == [1] * t.n
    assert P.same(three["sym_index"], two["sym_index"]) and P.same(three["R"], two["R"])
    for r in range(t.n):
        d1, d2 = (abs(z_angle_to_truth(o["R"][r], t.tags["R0"][r])) for o in (one, two))
        assert d2 < d1 - 1.0, (d1, d2)                            # 35.25 -> 32.25 degrees by the angles' means
    assert (two["sym_margin"].min(axis=1) < one["sym_margin"].max(axis=1)).all()
    for o in (one, two, three):
        M.invariants(o)


def test_the_reference_is_the_first_usable_slot():
    t, syms = SE.lost_reference()
    out = SE.model(t, syms)
    assert out["slot_status"].tolist() == [[1, 1, 0, 0, 0], [4, 1, 0, 0, 0], [4] * 5, [2] * 5]
    assert out["row_status"].tolist() == [0, 0, P.NO_ROTATION, P.NO_ROTATION]
    for r in (0, 1):
        assert out["sym_index"][r, 2] == 0                          # the reference keeps the identity
        assert np.abs(out["R"][r] - t.tags["W"][r, 2]).max() <= 4 * ULP
        assert (out["sym_index"][r, :2] == -1).all() and np.isnan(out["sym_margin"][r, :2]).all()
    # a permuted order of cameras moves the reference with it
    perm = SE.model(t, syms, cams=(4, 0, 3, 2))
    assert perm["sym_index"][0, 0] == 0 and np.abs(perm["R"][0] - t.tags["W"][0, 4]).max() <= 4 * ULP
    M.invariants(out), M.invariants(perm)


@pytest.mark.parametrize("kind", sorted(SE.BAD_VALUES))
def test_bad_symmetries_keep_the_promises(kind):
    for rounds in (1, 2, 4):
        t, syms = SE.bad_symmetries(kind, False)
        one = SE.model(t, syms, rounds)
        M.invariants(one)
        if kind in ("nan", "-inf", "zero"):                         # never the largest score: the row keeps its views
            assert (one["slot_status"] == 0).all() and (one["row_status"] == 0).all()
        elif rounds == 1:                                           # may be the largest: such a view leaves
            assert (one["slot_status"] == M.NO_SYM).any()
        t, syms = SE.bad_symmetries(kind, True)
        every = SE.model(t, syms, rounds)
        M.invariants(every)
        if kind == "zero":                                          # a score of 0 is taken: the zero matrix, finite
            assert (every["slot_status"] == 0).all() and (every["rot_views"] == 0).all()
            assert (every["row_status"] == P.AMBIGUOUS).all()
        else:                                                       # a row that loses every slot
            assert (every["slot_status"] == M.NO_SYM).all() and (every["row_status"] == P.NO_ROTATION).all()
            assert np.isnan(every["R"]).all() and (every["sym_index"] == -1).all() and (every["n_changed"] == 0).all()
        t, syms = SE.one_bad_entry(kind)
        M.invariants(SE.model(t, syms, rounds))

def test_arguments():
    t, syms = SE.duplicated()
    for bad in (dict(rounds=0), dict(rounds=5)):
        with pytest.raises(ValueError):
            SE.model(t, syms, **bad)
    for bad in (np.eye(4), np.zeros((0, 4, 4)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            SE.model(t, bad)


def test_the_euler_filter_drops_within_its_cap():
    """Every Euler draw of the CPU and GPU cases, with its own seed and size:
    the share ``euler_filter`` drops stays within ``random_raw``'s 1 % cap.
    tests/test_pose_gpu.py's ``Case`` seeds with 100 n + 10 C + the mode's code
    (0) + seed and draws n C vectors; ``random_raw`` draws m + m // 50 + 8."""
    draws = [(100 * n + 10 * C + seed, n * C) for n, C, seed in SE.EULER_CASES] + [(7, 300 * 8)]
    assert len(set(draws)) == len(draws)
    for seed, m in draws:
        rng = np.random.default_rng(seed)
        draw = rng.uniform(-6 * np.pi, 6 * np.pi, (m + m // 50 + 8, 3)).astype(np.float32)
        dropped = int((~M.euler_filter(draw)).sum())
        assert dropped <= len(draw) // 100, (seed, m, dropped)
        assert P.same(P.random_raw(np.random.default_rng(seed), m, "euler"), draw[M.euler_filter(draw)][:m])
