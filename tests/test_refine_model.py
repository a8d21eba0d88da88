"""The statement of the point refinement (tests/refine_model.py)
checked on the CPU: against scipy's Levenberg-Marquardt from the same start,
against LAPACK's inverse, and for the properties the kernel test relies on
(no row's cost rises, every regime occurs, the inputs behave as described)."""
import functools

import numpy as np
import pytest

import refine_model as M

# Measured on these inputs; the assertions allow ten times as much.
SCIPY_REL_MEASURED = 2.4e-6      # max |X_model - X_scipy| / |X_scipy|: scipy's own stopping rule and its
#                                  forward-difference Jacobian set this floor, not the model
INV_REL_MEASURED = 1.6e-15       # max |cov - inv(A)| / max |inv(A)| against numpy.linalg.inv


def _row_views(c, row):
    """(P [V, 3, 4], centroids [V, 2]) of the row's kept views."""
    C = c.C
    s = int(np.searchsorted(c.match_offs, row, side="right") - 1)
    co = c.cam_offs[C * s:C * s + C + 1]
    K = [d for d in range(C) if c.views[row, d] >= 0]
    return c.proj[s, K], np.stack([c.pts[co[d] + c.views[row, d]] for d in K])


def _full(A):
    return np.array([[A[0], A[1], A[2]], [A[1], A[3], A[4]], [A[2], A[4], A[5]]])


def _cost(c, row, X):
    P, cent = _row_views(c, row)
    return M.cost([p.ravel().tolist() for p in P], cent.tolist(), [float(x) for x in X])


@functools.lru_cache(maxsize=None)
def _scipy(C):
    """scipy's minimiser of every row of the "counts" case -> {row: x}."""
    from scipy.optimize import least_squares
    c = M.case("counts", C)

    def resid(X, P, cent):
        h = P[:, :, :3] @ X + P[:, :, 3]
        return (h[:, :2] / h[:, 2:3] - cent).ravel()

    return {int(row): least_squares(resid, c.X[row], args=_row_views(c, row), method="lm", xtol=1e-15,
                                    ftol=1e-15, gtol=1e-15).x for row in c.rows()}


@pytest.mark.parametrize("C", M.CAMS)
def test_model_returns_scipys_minimiser(C):
    """Every row of the wave-edge inputs converges within 10 evaluations and
    lands on scipy's Levenberg-Marquardt result from the same DLT start."""
    c = M.case("counts", C)
    X_out, rms, info, cov = M.expected("counts", C)
    rows = c.rows()
    assert (info[rows, 0] == M.CONVERGED).all() and (info[rows, 1] <= 10).all()       # every row takes part
    ref = _scipy(C)
    rel = np.array([np.linalg.norm(X_out[r] - ref[int(r)]) / np.linalg.norm(ref[int(r)]) for r in rows])
    print(f"C={C}: max relative difference to scipy {rel.max():.3g} over {rows.size} rows")
    assert rel.max() <= 10 * SCIPY_REL_MEASURED
    # and the model's cost is not above scipy's: to the rounding of the sum, and to what the last step
    # not taken can be worth (below 1e-10 |X| ~ 1e-8 mm, under 1e-6 px in every view of these rigs)
    for r in rows:
        assert _cost(c, r, X_out[r]) <= _cost(c, r, ref[int(r)]) * (1 + 1e-12) + 1e-12


@pytest.mark.parametrize("max_evals", M.MAX_EVALS)
@pytest.mark.parametrize("C", M.CAMS)
def test_cost_never_rises_and_rms_matches(C, max_evals):
    for name in ("counts", "regimes", "far", "origin", "centres", "neardup", "flat", "mixed", "scaled"):
        c = M.case(name, C)
        X_out, rms, info, cov = M.expected(name, C, max_evals)
        for r in c.rows():
            if info[r, 0] == M.SKIPPED:
                assert np.isnan(rms[r]).all() and np.isnan(cov[r]).all() and M.same(X_out[r], c.X[r])
                continue
            n = int((c.views[r] >= 0).sum())
            c0, c1 = _cost(c, r, c.X[r]), _cost(c, r, X_out[r])
            assert M.same(rms[r], np.array([np.sqrt(np.float64(c0) / n), np.sqrt(np.float64(c1) / n)]))
            assert not c1 > c0
            if info[r, 0] == M.FAILED:
                assert M.same(X_out[r], c.X[r]) and info[r, 1] <= max_evals
            assert 0 <= info[r, 1] <= max_evals


def test_every_regime_occurs():
    seen_k = set()
    for C in M.CAMS:
        c = M.case("counts", C)
        rows = c.rows()
        info = M.expected("counts", C)[2][rows]
        exact = c.kind[rows] == "exact"
        assert exact.sum() >= 3 and (info[exact] == (M.CONVERGED, 0)).all()            # exact projections
        for cap in (1, 2):
            capped = M.expected("counts", C, cap)[2][rows]
            assert ((capped[:, 0] == M.CAPPED) & (capped[:, 1] == cap)).sum() >= 3      # stopped at the cap
        seen_k |= set((c.views[rows] >= 0).sum(axis=1).tolist())
        r = M.case("regimes", C)
        rows = r.rows()
        X_out, rms, info, cov = M.expected("regimes", C)
        kind = r.kind[rows]
        zero3, azero, skip = (rows[kind == k] for k in ("zero3", "azero", "skip"))
        assert len(zero3) >= 3 and len(azero) >= 3 and len(skip) >= 6
        assert (info[zero3, 0] == M.FAILED).all() and not np.isfinite(rms[zero3]).any()
        assert (info[azero, 0] == M.FAILED).all() and np.isfinite(rms[azero]).all()     # A = 0: the pivot fails
        assert (info[skip] == (M.SKIPPED, 0)).all()
        single = (r.views[skip] >= 0).sum(axis=1) == 1
        assert single.sum() >= 3 and (~single).sum() >= 3                              # |K| = 1, a bad index
        for rows_ in (zero3, azero, skip):
            assert M.same(X_out[rows_], r.X[rows_]) and np.isnan(cov[rows_]).all()
    assert seen_k == set(range(2, 9))                                                  # |K| = 2 .. 8


@pytest.mark.parametrize("C", M.CAMS)
def test_covariance_is_the_inverse_normal_matrix(C):
    worst = 0.0
    for name in ("counts", "regimes"):
        c = M.case(name, C)
        X_out, rms, info, cov = M.expected(name, C)
        for r in c.rows():
            if info[r, 0] == M.SKIPPED:
                continue
            P, cent = _row_views(c, r)
            A = M.normal_equations([p.ravel().tolist() for p in P], cent.tolist(), X_out[r].tolist())[0]
            if M.ldlt(A) is None:                    # NaN exactly where a pivot fails
                assert np.isnan(cov[r]).all()
                continue
            assert np.isfinite(cov[r]).all()
            inv = np.linalg.inv(_full(A))[np.triu_indices(3)]
            worst = max(worst, float(np.abs(cov[r] - inv).max() / np.abs(inv).max()))
    print(f"C={C}: max relative difference to numpy.linalg.inv {worst:.3g}")
    assert worst <= 10 * INV_REL_MEASURED


def test_refined_points_are_no_further_from_the_truth_on_average():
    """600 rigs a camera count, one noisy point each over all its views: a
    property of these inputs, on the mean only."""
    for C in M.CAMS:
        c = M.case("truth", C)
        rows = c.rows()
        X_out, rms, info, cov = M.expected("truth", C)
        assert rows.size >= 500 and (c.kind[rows] == "noisy").all() and (info[rows, 0] <= M.CAPPED).all()
        before = np.linalg.norm(c.X[rows] - c.truth[rows], axis=1).mean()
        after = np.linalg.norm(X_out[rows] - c.truth[rows], axis=1).mean()
        print(f"C={C}: mean distance to the truth {before:.4f} mm (DLT) -> {after:.4f} mm (refined)")
        assert after <= before
