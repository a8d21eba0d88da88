"""The inputs of tests/test_view_prune_gpu.py, proved on the CPU to be what
they are meant to be (tests/view_prune_model.py builds them and restates the
definition of DESIGN §3.15): no decision is closer than the kernel's DLT and
numpy's can differ, every kind of row occurs, and pruning helps."""
import numpy as np
import pytest

import view_prune_model as M

FINITE = [g for g in M.GATES if np.isfinite(g)]


@pytest.mark.parametrize("name,C", M.CASES)
def test_no_decision_within_the_margin(name, C):
    """(a) Every residual compared with a gate is more than MARGIN = 1e-6 px
    away from it, and no two candidates of a pass are within MARGIN of each
    other (the duplicated camera's exact tie apart).  MARGIN is not taken on
    trust: after a drop the kernel's X and the restatement's differ by at most
    §3.8's 1e-9 + 1e-10 |X_i| mm per component, which moves a residual by at
    most that vector's length times the 2-norm of the projection's Jacobian;
    per case that product stays below MARGIN / 10."""
    c = M.case(name, C)
    worst_move = 0.0
    for gate in M.GATES:
        trace = M.expected(name, C, gate)[5]
        assert trace
        for t in trace:
            r = t["r"]
            for d, q in r.items():
                if np.isfinite(gate) and not np.isnan(q):
                    assert abs(q - gate) > M.MARGIN, (name, C, gate, t["row"], d, q)
                if t["passno"] > 0 and np.isfinite(q):
                    b = M.ATOL + M.RTOL * np.abs(t["X"])
                    worst_move = max(worst_move, float(np.linalg.norm(b))
                                     * M.jacobian_norm(c.proj[t["scene"], d], t["X"]))
            cand = sorted((q, d) for d, q in r.items() if not q <= gate and not np.isnan(q))
            for (qa, da), (qb, db) in zip(cand, cand[1:]):
                if name == "tie" and {da, db} == {3, 4}:
                    assert qa == qb
                    continue
                assert qb - qa > M.MARGIN or qa == qb == np.inf, (name, C, gate, t["row"], da, db)
            assert sum(np.isnan(q) for q in r.values()) <= 1        # one NaN view at most: no NaN tie
    assert worst_move < M.MARGIN / 10, worst_move


def _outcomes(name, C, gate):
    """Per row of the captures: (extra views kept on entry, dropped, over the
    gate on the first pass and kept in the end)."""
    c = M.case(name, C)
    views, _, _, pruned, touched, trace = M.expected(name, C, gate)
    out = {}
    for row in np.nonzero(touched)[0]:
        if c.kind[row] != "skip":
            out[int(row)] = [int((c.views[row, 3:] >= 0).sum()), bin(int(pruned[row])).count("1"), 0]
    for t in trace:
        if t["passno"] == 0:
            out[t["row"]][2] = sum(1 for d, q in t["r"].items() if not q <= gate and views[t["row"], d] >= 0)
    return out


@pytest.mark.parametrize("C", (5, 8))
def test_every_kind_of_row_occurs(C):
    """(b) At the gate of 5 px the per-capture-count input holds at least
    three rows that drop nothing, one view, two or more in sequence, every
    extra view (V = 3), and three "masking" rows: a view over the gate on the
    first pass that is kept in the end."""
    o = np.array(list(_outcomes("counts", C, M.MAIN_GATE).values()))
    kept, dropped, masked = o[:, 0], o[:, 1], o[:, 2]
    assert ((dropped == 0) & (kept > 0)).sum() >= 3
    assert (dropped == 1).sum() >= 3
    assert (dropped >= 2).sum() >= 3
    assert ((dropped == kept) & (kept > 0)).sum() >= 3
    assert (masked > 0).sum() >= 3
    # ... and at the other gates something is dropped and something kept, 0 and +inf apart
    for gate in (1.0, 20.0):
        o = np.array(list(_outcomes("counts", C, gate).values()))
        assert (o[:, 1] > 0).any() and (o[:, 1] < o[:, 0]).any()
    o = np.array(list(_outcomes("counts", C, 0.0).values()))
    assert (o[:, 1] == o[:, 0]).all()                       # every residual is above 0
    o = np.array(list(_outcomes("counts", C, float("inf")).values()))
    assert (o[:, 1] == 0).all()


def test_four_cameras_drop_or_keep_the_one_extra_view():
    o = np.array(list(_outcomes("counts", 4, M.MAIN_GATE).values()))
    assert ((o[:, 1] == 0) & (o[:, 0] == 1)).sum() >= 3 and (o[:, 1] == 1).sum() >= 3


@pytest.mark.parametrize("name,C", M.CASES)
def test_pruning_moves_X_towards_the_true_point(name, C):
    """(c) At the gate of 5 px the pruned X is nearer the true point than the X
    that came in on every row with a grossly shifted view (the greedy order
    now and then drops a good view beside the shifted ones -- X is then the
    DLT over fewer, good views -- so the dropped set is not asserted); at the
    gates of 1 and 20 px on every such row that dropped all its shifted views
    (a 30 px shift in one of four views shows as 15 px: under a gate of 20 it
    stays, and X with it).  Of the "nan" input the ordinary third capture
    counts; the first two have a broken P, no true point to be near."""
    c = M.case(name, C)
    first = int(c.match_offs[2]) if name == "nan" else 0
    rows = [r for r in range(first, len(c.kind)) if c.kind[r] not in ("", "skip") and c.gross[r].any()]
    assert len(rows) >= 1
    for gate in (1.0, 5.0, 20.0):
        _, _, X, pruned, _, _ = M.expected(name, C, gate)
        hit = 0
        for r in rows:
            gross = sum(1 << d for d in np.nonzero(c.gross[r])[0])
            if gate == M.MAIN_GATE or int(pruned[r]) & gross == gross:
                hit += 1
                assert int(pruned[r]) & gross
                assert np.linalg.norm(X[r] - c.truth[r]) < np.linalg.norm(c.X[r] - c.truth[r]), (gate, r)
        assert hit >= 1 or gate != M.MAIN_GATE


def test_special_views_and_rows():
    """The NaN view goes first, the inf view next to it is dropped at every
    finite gate, a row with a seed or an extra-view index out of range is left
    alone, an empty extra view stays empty."""
    for C in (4, 5):
        c = M.case("nan", C)
        for gate in M.GATES:
            views, _, _, pruned, _, trace = M.expected("nan", C, gate)
            first = {t["row"]: t for t in trace if t["passno"] == 0}
            for row in range(int(c.match_offs[0]), int(c.match_offs[0]) + 12):
                assert np.isnan(first[row]["r"][C - 1]) and first[row]["dropped"] == C - 1
            for row in range(int(c.match_offs[1]), int(c.match_offs[1]) + 12):
                assert np.isinf(first[row]["r"][C - 1])
                assert bool(pruned[row] >> (C - 1) & 1) == np.isfinite(gate)
    c = M.case("counts", 5)
    views, ext, X, pruned, touched, _ = M.expected("counts", 5, 0.0)
    skip = np.nonzero(c.kind == "skip")[0]
    assert skip.size == 3 and (pruned[skip] == 0).all() and touched[skip].all()
    assert np.array_equal(views[skip], c.views[skip]) and np.array_equal(X[skip], c.X[skip])
    rows = slice(int(c.match_offs[4]), int(c.match_offs[4]) + int(c.count[4]))
    assert (c.views[rows, 3] == -1).all() and (pruned[rows] & 8 == 0).all()
    assert touched.sum() == c.count.sum() and (pruned[~touched] == 0).all()


def test_tie_drops_the_lower_camera_first():
    for C in (5, 8):
        trace = M.expected("tie", C, M.MAIN_GATE)[5]
        tied = [t for t in trace if t["dropped"] in (3, 4) and 3 in t["r"] and 4 in t["r"]
                and t["r"][3] == t["r"][4]]
        assert len(tied) >= 3 and all(t["dropped"] == 3 for t in tied)


def test_worst_ranks_nan_first_then_size_then_camera():
    nan = float("nan")
    assert M._worst({3: 9.0, 4: nan, 5: 1e300}) == 4
    assert M._worst({3: nan, 4: nan}) == 3
    assert M._worst({3: 2.0, 4: 7.0, 5: 7.0}) == 4
    assert M._worst({5: float("inf"), 6: 1e308}) == 5
