"""Where the descent of tests/refine_model.py rejects, stalls and fails
(DESIGN §3.17), pinned on the CPU: ``refine_trace`` counts what every row of
the inputs of tests/refine_edges.py did, and each branch an input is there to
reach must be reached, by at least three rows at every camera count.  The
counts are conditions on the seeds, not measurements.  The invariants of
tests/test_refine_model.py run over the same inputs there; here also the
covariance on ill-conditioned rows and scipy from the far starts."""
import functools

import numpy as np
import pytest

import refine_edges as E
import refine_model as M
from test_refine_model import _full, _row_views

# Measured on these inputs; the assertions allow ten times as much.
INV_COND_MEASURED = 0.61         # max |cov - inv(A)| / (max |inv(A)| cond(A) 2.2e-16)
SCIPY_FAR_MEASURED = 1.03e-7     # max |X_model - X_scipy| / |X_scipy| on the rows where both reach one minimum
EPS = 2.2e-16

# (input, max_evals, branch) -> what a trace of it must show; every one by >= 3 rows at every C
REACHED = {
    ("far", 64, "a run of five or more rejections"): lambda t: t["longest_run"] >= 5,
    ("far", 64, "more than ten evaluations"): lambda t: t["evals"] > 10,
    ("far", 64, "capped after an accepted step"): lambda t: t["status"] == M.CAPPED and not t["capped_in_run"],
    ("far", 64, "capped inside a run of rejections"): lambda t: t["status"] == M.CAPPED and t["capped_in_run"],
    ("far", 10, "capped inside a run of rejections"): lambda t: t["status"] == M.CAPPED and t["capped_in_run"],
    ("far", 64, "the damping at its floor"): lambda t: t["floor_steps"] > 0,
    ("far", 64, "a rejection with c1 == c"): lambda t: t["ties"] > 0,
    ("origin", 64, "X.X = 0 in the convergence test"): lambda t: t["xx_zero"] > 0,
    ("origin", 64, "a run of five or more rejections"): lambda t: t["longest_run"] >= 5,
    ("centres", 64, "the damping at its floor"): lambda t: t["floor_steps"] > 0,
    ("centres", 64, "more than ten evaluations"): lambda t: t["evals"] > 10,
    ("neardup", 64, "every evaluation used"): lambda t: t["evals"] == 64,
    ("neardup", 64, "the damping at its floor"): lambda t: t["floor_steps"] > 0,
    ("flat", 10, "the second pivot fails"): lambda t: t["failed_at"] == "pivot" and t["pivot"] == 1,
    ("flat", 10, "the third pivot fails"): lambda t: t["failed_at"] == "pivot" and t["pivot"] == 2,
    ("scaled", 64, "failed after an accepted step"): lambda t: t["failed_after_accept"],
    ("scaled", 64, "a rejection with c1 = +inf"): lambda t: t["inf_trials"] > 0,
    ("scaled", 64, "the start cost not finite"): lambda t: t["failed_at"] == "start",
    ("scaled", 64, "the first pivot fails"): lambda t: t["failed_at"] == "pivot" and t["pivot"] == 0,
    ("mixed", 64, "the start cost not finite"): lambda t: t["failed_at"] == "start",
    ("mixed", 64, "capped inside a run of rejections"): lambda t: t["status"] == M.CAPPED and t["capped_in_run"],
    ("mixed", 64, "a rejection with c1 == c"): lambda t: t["ties"] > 0,
    ("mixed", 64, "the damping at its floor"): lambda t: t["floor_steps"] > 0,
}


@functools.lru_cache(maxsize=None)
def _traces(name, C, max_evals):
    """{row: trace with the row's status} of the rows not skipped."""
    (X_out, rms, info, cov), traces = E.traced(name, C, max_evals)
    return {r: dict(t, status=int(info[r, 0])) for r, t in traces.items()}


def test_the_tracer_is_the_definition():
    """refine_trace returns refine_row's values, and its counters add up."""
    c = M.case("far", 4)
    for r in c.rows()[:40]:
        P, cent = _row_views(c, r)
        P, cent = [p.ravel().tolist() for p in P], cent.tolist()
        plain = M.refine_row(P, cent, c.X[r], 64)
        traced, t = M.refine_trace(P, cent, c.X[r], 64)
        for a, b in zip(plain, traced):
            assert M.same(np.asarray(a, np.float64), np.asarray(b, np.float64))
        assert t["evals"] == plain[3] == t["accepted"] + t["rejections"]
        assert t["ties"] + t["nan_trials"] + t["inf_trials"] <= t["rejections"] >= t["longest_run"]


@pytest.mark.parametrize("C", M.CAMS)
def test_every_claimed_branch_is_reached(C):
    for (name, max_evals, branch), pred in REACHED.items():
        n = sum(1 for t in _traces(name, C, max_evals).values() if pred(t))
        print(f"C={C} {name} max_evals={max_evals}: {branch}: {n} rows")
        assert n >= 3, (name, max_evals, branch, n)


@pytest.mark.parametrize("C", M.CAMS)
def test_the_kinds_do_what_they_are_named_for(C):
    for name in ("flat", "mixed", "origin"):
        c = M.case(name, C)
        rows = c.rows()
        info = M.expected(name, C, 64)[2]
        kind = c.kind[rows]
        for k, status in (("flat", M.FAILED), ("huge", M.FAILED), ("single", M.SKIPPED), ("badidx", M.SKIPPED)):
            assert (info[rows[kind == k], 0] == status).all()
        assert (info[rows[kind == "exact"]] == (M.CONVERGED, 0)).all()
    c = M.case("origin", C)
    assert (c.X[c.rows()] == 0.0).all() and np.signbit(c.X[c.rows()[-1], 0]) and not np.signbit(c.X[c.rows()[0], 0])
    c = M.case("neardup", C)                 # the twins: equal, a shifted fourth column, a scaled matrix
    assert M.same(c.proj[0, 1], c.proj[0, 0]) and M.same(c.proj[1, 1, :, :3], c.proj[1, 0, :, :3])
    assert not M.same(c.proj[1, 1], c.proj[1, 0]) and not M.same(c.proj[2, 1], c.proj[2, 0])
    np.testing.assert_allclose(c.proj[1, 1], c.proj[1, 0], rtol=2e-7)
    np.testing.assert_allclose(c.proj[2, 1], c.proj[2, 0], rtol=2e-9)
    for s in range(3):
        rows = np.arange(c.match_offs[s], c.match_offs[s] + c.count[s])
        assert ((c.views[rows] >= 0) == (np.arange(C) < 2)).all()          # the twin views only


@pytest.mark.parametrize("C", M.CAMS)
def test_mixed_statuses_within_one_wave(C):
    """The 257-row capture: every 64 consecutive rows hold all four statuses,
    a row of no evaluation and one of 30 or more; row 0, whose lane alone has
    a fifth row, is a long one; and a failed start, both kinds of skipped row
    and a row that uses all 64 evaluations sit within eight lanes."""
    c = M.case("mixed", C)
    info = M.expected("mixed", C, 64)[2]
    n = int(c.count[0])
    assert n == 257 and int(c.count[1]) == 65
    st, ev, kind = info[:n, 0], info[:n, 1], c.kind[:n]
    for w in range(n - 63):
        b = slice(w, w + 64)
        assert len(set(st[b].tolist())) >= 4, w
        assert (ev[b] == 0).any() and (ev[b] >= 30).any(), w
    assert ev[0] >= 30
    long_first = [l for l in range(64) if ev[l] >= 30 and len(set(st[l::64].tolist())) >= 2]
    assert len(long_first) >= 3
    together = [w for w in range(n - 7) if (ev[w:w + 8] == 64).any() and (st[w:w + 8] == M.FAILED).any()
                and {"single", "badidx"} <= set(kind[w:w + 8]) and w // 64 == (w + 7) // 64]
    assert together, "no eight lanes with a failed, both skipped and a 64-evaluation row"


@pytest.mark.parametrize("C", M.CAMS)
def test_covariance_on_ill_conditioned_rows(C):
    """The rule of test_covariance_is_the_inverse_normal_matrix on the new
    inputs: NaN exactly where ``ldlt`` fails, otherwise numpy's inverse, to
    cond(A) 2.2e-16 times a measured margin (twin cameras leave A close to
    rank 2, so the well-conditioned bound there does not apply)."""
    worst, worst_cond, undetermined = 0.0, 0.0, 0
    for name in E.NAMES:
        c = M.case(name, C)
        for max_evals in (10, 64):
            X_out, rms, info, cov = M.expected(name, C, max_evals)
            for r in c.rows():
                if info[r, 0] == M.SKIPPED:
                    continue
                P, cent = _row_views(c, r)
                A = M.normal_equations([p.ravel().tolist() for p in P], cent.tolist(), X_out[r].tolist())[0]
                if M.ldlt(A) is None:
                    assert np.isnan(cov[r]).all()
                    continue
                full = _full(A)
                if not 2.0 ** -900 <= np.abs(full).max() <= 2.0 ** 900:
                    continue                 # "scaled": 1 / d overflows or A is subnormal; the GPU test has the bits
                assert np.isfinite(cov[r]).all()
                kappa = float(np.linalg.cond(full))
                if not kappa * EPS < 1.0:    # no digit of the inverse is determined (LAPACK calls some singular)
                    undetermined += 1
                    continue
                inv = np.linalg.inv(full)[np.triu_indices(3)]
                ratio = float(np.abs(cov[r] - inv).max() / np.abs(inv).max()) / (kappa * EPS)
                worst, worst_cond = max(worst, ratio), max(worst_cond, kappa)
    print(f"C={C}: max |cov - inv| / (max |inv| cond 2.2e-16) = {worst:.3g}; largest cond {worst_cond:.3g}; "
          f"{undetermined} rows of cond >= 1 / 2.2e-16 not compared")
    assert worst_cond >= 1e12                # the ill-conditioned rows took part
    assert worst <= 10 * INV_COND_MEASURED


@functools.lru_cache(maxsize=None)
def _scipy(name, C, rows):
    from scipy.optimize import least_squares
    c = M.case(name, C)

    def resid(X, P, cent):
        h = P[:, :, :3] @ X + P[:, :, 3]
        return (h[:, :2] / h[:, 2:3] - cent).ravel()

    return {int(r): least_squares(resid, c.X[r], args=_row_views(c, r), method="lm", xtol=1e-15, ftol=1e-15,
                                  gtol=1e-15) for r in rows}


@pytest.mark.parametrize("C", M.CAMS)
def test_far_starts_reach_scipys_minimum(C):
    """A reference that is not the model: scipy's Levenberg-Marquardt from
    the same start, on the converged rows of the starts 100 and 1000 mm off
    and at the origin.  Rows where scipy's cost is within 1e-9 relative of the
    model's are compared (another local minimum is no error); they must be at
    least half of the converged rows."""
    worst, n_conv, n_same = 0.0, 0, 0
    for name in ("far", "origin"):
        c = M.case(name, C)
        X_out, rms, info, cov = M.expected(name, C, 64)
        rows = tuple(int(r) for r in c.rows()
                     if info[r, 0] == M.CONVERGED and c.kind[r] in ("far2", "far3", "origin", "negzero"))
        ref = _scipy(name, C, rows)
        for r in rows:
            n = int((c.views[r] >= 0).sum())
            cm, cs = rms[r, 1] ** 2 * n, 2.0 * ref[r].cost
            n_conv += 1
            if abs(cs - cm) <= 1e-9 * cm:
                n_same += 1
                worst = max(worst, float(np.linalg.norm(X_out[r] - ref[r].x) / np.linalg.norm(ref[r].x)))
    print(f"C={C}: {n_same} of {n_conv} converged rows at scipy's minimum; max relative difference {worst:.3g}")
    assert n_conv >= 30 and 2 * n_same >= n_conv
    assert worst <= 10 * SCIPY_FAR_MEASURED
