"""tests/box_fit_model.py, the statement of the box fit, is the
thing under test here: its Jacobian against central differences, the
invariants of the descent, the accuracy it buys on exact rotations, the tie
rule, and a count of every regime the GPU test then compares bit for bit."""
import math

import numpy as np
import pytest

import box_fit_inputs as I
import box_fit_model as M

# The analytic gradient against central differences of the cost with h = 1e-3
# mm at the starts of the "truth" rows (generic points: no vertex changes its
# extreme within h): the largest relative difference measured is 8.8e-9
# (truncation h^2 / depth^2 ~ 4e-13 and rounding eps cost / (h g) ~ 1e-9
# explain it); the bound is ten times that.
JACOBIAN_MEASURED = 8.8e-9
JACOBIAN_BOUND = 10 * JACOBIAN_MEASURED


def _row_inputs(c, w):
    K = [d for d in range(c.C) if c.views[w][d] >= 0]
    s = int(c.scene[w])
    P = [c.proj[s, d].reshape(12).tolist() for d in K]
    bx = [[float(b) for b in c.boxes[w][d]] for d in K]
    return P, c.pose[w][:3, :3].reshape(9).tolist(), bx, c.verts.tolist(), c.pose[w][:3, 3].tolist()


def test_gradient_equals_central_differences():
    """g = J^T r: d(cost)/dt = 2 g, so the analytic rows of J are checked
    through the gradient they give, at the generic points where the cost is
    smooth."""
    c = I.case("truth", 4)
    worst, h = 0.0, 1e-3
    for w in range(40):
        P, R, bx, verts, t = _row_inputs(c, w)
        _, _, g, _ = M.evaluate(P, R, bx, verts, t)
        for j in range(3):
            tp, tm = list(t), list(t)
            tp[j] += h
            tm[j] -= h
            fd = (M.evaluate(P, R, bx, verts, tp)[0] - M.evaluate(P, R, bx, verts, tm)[0]) / (2 * h)
            worst = max(worst, abs(fd - 2 * g[j]) / max(abs(fd), abs(2 * g[j])))
    print("largest relative difference", worst)
    assert worst <= JACOBIAN_BOUND


@pytest.mark.parametrize("C", I.CAMS)
def test_no_cost_rises_and_rms_is_its_root(C):
    c = I.case("regimes", C)
    out, _ = I.expected("regimes", C)
    fitted = 0
    for w in range(len(c.kind)):
        if out["info"][w, 0] == M.SKIPPED:
            assert np.isnan(out["rms"][w]).all() and M.same(out["pose"][w], c.pose[w])
            assert np.isnan(out["cov"][w]).all() and np.isnan(out["resid"][w]).all()
            continue
        P, R, bx, verts, t = _row_inputs(c, w)
        c0 = M.evaluate(P, R, bx, verts, t)[0]
        c1, _, _, resid = M.evaluate(P, R, bx, verts, out["pose"][w][:3, 3].tolist())
        assert c1 <= c0
        n4 = 4.0 * len(P)
        assert M.same(out["rms"][w], np.array([math.sqrt(c0 / n4), math.sqrt(c1 / n4)]))
        assert M.same(out["pose"][w][:3, :3], c.pose[w][:3, :3]) and M.same(out["pose"][w][3], c.pose[w][3])
        K = [d for d in range(C) if c.views[w][d] >= 0]
        assert M.same(out["resid"][w][K], np.array(resid))
        assert np.isnan(np.delete(out["resid"][w], K, axis=0)).all()
        if out["info"][w, 0] == M.FAILED:
            assert M.same(out["pose"][w], c.pose[w])
        fitted += 1
    assert fitted >= 12


# Mean |t - t_true| in mm before and after the fit, exact rotations, boxes the
# truncated exact extents, 240 rows per C, from the DLT of all views' box
# centres, every row keeping a random 1..C views ("truth"); measured on the
# model (DESIGN §3.22 holds the table):
#   C   rows |K| >= 2: before  after    rows |K| = 1: before  after
#   3                  32.3    0.36                   32.8    1.94
#   4                  33.2    0.32                   32.8    2.24
#   8                  34.4    0.35                   34.1    1.93
# The single-view figure holds too, so both inequalities are asserted.
@pytest.mark.parametrize("C", I.CAMS)
def test_translation_error_falls(C):
    c = I.case("truth", C)
    out, _ = I.expected("truth", C)
    before = np.linalg.norm(c.pose[:, :3, 3] - c.truth, axis=1)
    after = np.linalg.norm(out["pose"][:, :3, 3] - c.truth, axis=1)
    k = (c.views >= 0).sum(axis=1)
    st = out["info"][:, 0]
    print(C, "K>=2:", before[k >= 2].mean(), after[k >= 2].mean(), "K=1:", before[k == 1].mean(), after[k == 1].mean(),
          "status", np.bincount(st, minlength=4).tolist(), "evals mean", out["info"][:, 1].mean(),
          "max", out["info"][:, 1].max())
    assert (k >= 2).sum() >= 100 and (k == 1).sum() >= 10
    assert after[k >= 2].mean() < before[k >= 2].mean()
    assert after[k == 1].mean() < before[k == 1].mean()


def test_tie_keeps_the_lowest_vertex():
    """Two vertices share the maximal u exactly, at different depths: which
    one is taken decides the Jacobian's row, so swapping them in ``verts``
    changes the output's bits and a wrong tie-break on the device shows."""
    a, b = (M.fit_boxes(*I.tie_case(s).args(), 10) for s in (False, True))
    c = I.tie_case(False)
    P, R, bx, verts, t = _row_inputs(c, 0)
    ext, invalid = M.extremes(P[0], R, verts, t)
    assert not invalid and ext[2] == [0.5, 2.0]                      # vertex 0's depth, not vertex 1's 4.0
    assert M.extremes(P[0], R, I.tie_case(True).verts.tolist(), t)[0][2] == [0.5, 4.0]
    assert not M.same(a["pose"], b["pose"])
    assert not M.same(a["cov"], b["cov"]) or not M.same(a["info"], b["info"])


@pytest.mark.parametrize("C", I.CAMS)
def test_every_regime_is_reached(C):
    c = I.case("regimes", C)
    out, tr = I.expected("regimes", C)
    st, kind = out["info"][:, 0], c.kind
    assert ((kind == "behind") & (st == M.FAILED)).sum() >= 3
    assert all(tr[w]["failed_at"] == "start" for w in np.nonzero(kind == "behind")[0])
    # behind only at a trial point: rejected, the row goes on
    assert sum(tr[w]["invalid_trials"] > 0 and tr[w]["accepted"] > 0 and st[w] != M.FAILED
               for w in np.nonzero(kind == "near")[0]) >= 3
    az = np.nonzero(kind == "azero")[0]
    assert len(az) >= 3 and (st[az] == M.FAILED).all() and all(tr[w]["failed_at"] == "pivot" for w in az)
    assert ((kind == "noview") & (st == M.SKIPPED)).sum() >= 3 and ((kind == "noscene") & (st == M.SKIPPED)).sum() >= 3
    assert ((kind == "fit") & (st == M.CONVERGED)).sum() >= 3
    for cap in (1, 2):
        capped = I.expected("regimes", C, cap)[0]["info"]
        assert ((capped[:, 0] == M.CAPPED) & (capped[:, 1] == cap)).sum() >= 3
    # a start that already satisfies the stop rule: converged with no evaluation
    again = I.expected("restart", C)[0]["info"]
    assert ((again[:, 0] == M.CONVERGED) & (again[:, 1] == 0)).sum() >= 3


def test_every_number_of_kept_views():
    c = I.case("truth", 8)
    k = (c.views >= 0).sum(axis=1)
    st = I.expected("truth", 8)[0]["info"][:, 0]
    for n in range(1, 9):
        assert ((k == n) & (st <= M.CAPPED)).sum() >= 3, n


@pytest.mark.parametrize("V", (64, 65, 129))
def test_last_vertex_holds_every_kind_of_extreme(V):
    c = I.case(f"last{V}")
    P, R, bx, verts, t = _row_inputs(c, 0)
    last = verts[-1]
    for p, kinds in zip(P, ((2, 3), (0, 1))):                        # camera 0: umax, vmax; camera 1: umin, vmin
        ext, _ = M.extremes(p, R, verts, t)
        alone, _ = M.extremes(p, R, [last], t)
        for e in kinds:
            assert ext[e] == alone[e]
    assert (I.expected(f"last{V}")[0]["info"][:, 0] == M.CONVERGED).all()


def test_second_stride_holds_the_extremes():
    c = I.case("stride2", 4)
    P, R, bx, verts, t = _row_inputs(c, 0)
    for p in P:
        ext, _ = M.extremes(p, R, verts, t)
        far = [M.extremes(p, R, [verts[i]], t)[0] for i in (69, 70, 71, 72)]
        for e in range(4):
            assert any(ext[e] == f[e] for f in far)                  # an outlier of the second stride, whichever
