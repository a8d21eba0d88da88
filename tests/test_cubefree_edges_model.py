"""The inputs of tests/test_cubefree_edges_gpu.py, pinned on the CPU so that
the GPU tests cannot pass vacuously (tests/cubefree_inputs.py builds them):

* the closed form of a rectified scene equals oracle.cube and
  oracle.residuals bit for bit on every rectified scene the GPU file uses;
* the solver model (oracle/lsap_sparse.py, the kernels' own parameters, 16-bit
  keys) equals scipy on every assignment case, and its counters prove the
  regime each case claims: "lists" (ties settled inside the candidate lists:
  no dense scan, yet rows with tied minima) or "overflow" (lists past their
  capacity, dense tie scans);
* the arithmetic model of the float32 block minima (tests/test_minima_approx.py)
  on the rectified cases: the straddling triple's approximate key differs from
  the exact one and sits within kApproxMargin of a carry (the kernel must
  recheck, and the recheck changes the key); at least half the coarse-grid
  blocks fail the float32 test; zero and tiny costs fall below kApproxTiny.
"""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment as scipy_lsa

import cubefree_inputs as CI
from oracle import lsap as L
from oracle import lsap_sparse as SP
from oracle import oracle as O

MARGIN = 8                     # kApproxMargin (csrc/mvm_cube.hip)
TINY = 0x0D800000              # kApproxTiny: the bits of 2^-100


@pytest.fixture(scope="module")
def minima():
    return CI.minima_cases()


@pytest.fixture(scope="module")
def assign():
    return CI.assign_cases()


def _rect_batches(minima, assign):
    out = dict(minima)
    out.update({"assign_" + k: c.batch for k, c in assign.items()})
    out["select"] = CI.select_batch()
    return out


def test_closed_form_equals_oracle(minima, assign):
    n_rect = 0
    for name, b in _rect_batches(minima, assign).items():
        S = len(b.scenes)
        oc, _, _, offs, _ = O.cube(b.pts, b.co, b.F, S)
        max_n = max(max(c) for c in b.counts)
        R = O.residuals(b.pts, b.co, b.F, S, max_n)
        for s, sc in enumerate(b.scenes):
            if not sc.rect:
                continue
            n_rect += 1
            want = CI.closed_form_cube(*sc.ys).reshape(-1)
            assert np.array_equal(want.view(np.int32), oc[offs[s]:offs[s + 1]].view(np.int32)), (name, s)
            wr = CI.closed_form_residuals(*sc.ys, max_n)
            assert np.array_equal(wr.view(np.int64), R[s].view(np.int64)), (name, s)
    assert n_rect >= 40


def test_cases_hold_what_they_are_about(minima):
    """Zeros and ties on the coarse grids; 2^64 exactly and the next double;
    +inf float32 costs without NaN; residuals that are +inf (1.7e308)."""
    b = minima["coarse"]
    for sc in b.scenes:
        c = CI.closed_form_cube(*sc.ys)
        assert (c == 0).any() and len(np.unique(c)) <= 40
    assert len(np.unique(CI.closed_form_cube(*b.scenes[-1].ys))) == 1          # the all-zero cube
    for sc in minima["two64"].scenes:
        e = np.concatenate([CI.closed_form_pair(sc.ys[a], sc.ys[c]).reshape(-1) for a, c in ((0, 1), (0, 2), (1, 2))])
        assert (e == CI.TWO64).any() and (e == CI.TWO64_UP).any()
        assert np.isfinite(CI.closed_form_cube(*sc.ys)).all()
    kinds = set()
    for sc in minima["huge"].scenes:
        c = CI.closed_form_cube(*sc.ys)
        e = np.concatenate([CI.closed_form_pair(sc.ys[a], sc.ys[d]).reshape(-1) for a, d in ((0, 1), (0, 2), (1, 2))])
        assert not np.isnan(c).any() and np.isfinite(c).any()
        kinds.add((bool(np.isinf(c).any()), bool(np.isinf(e).any())))
        assert e.max() > CI.TWO64
    # 1e30: finite costs; 1e200: +inf costs of finite residuals; 1.7e308: +inf residuals
    assert kinds == {(False, False), (True, False), (True, True)}
    for sc in minima["tiny"].scenes:
        c = CI.closed_form_cube(*sc.ys)
        assert ((c > 0) & (c < 2.0 ** -100)).mean() > 0.9


# ------------------------------------------------------------- the solver ----
def _flat(sc):
    N, M, P = sc.counts
    if sc.rect:
        return CI.closed_form_cube(*sc.ys).reshape(N * M, P)
    b = CI.batch_of([sc])
    return O.cube(b.pts, b.co, b.F, 1)[0].reshape(N * M, P)


@pytest.mark.parametrize("name", ["lists", "overflow", "constant", "f13_zero", "dup10", "dup30",
                                  "inf_feasible", "infeasible", "min_cols"])
def test_model_equals_scipy_in_the_claimed_regime(assign, name):
    case = assign[name]
    status = case.status or [0] * len(case.batch.scenes)
    for s, sc in enumerate(case.batch.scenes):
        flat = _flat(sc)
        stats = {}
        if status[s] == 2:
            with pytest.raises(ValueError, match="infeasible"):
                scipy_lsa(flat)
            with pytest.raises(L.LsapError, match="infeasible"):
                SP.linear_sum_assignment(flat, **SP.DEFAULTS, key16=True)
            continue
        got = SP.linear_sum_assignment(flat, **SP.DEFAULTS, key16=True, stats=stats)
        ref = scipy_lsa(flat)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (name, s)
        W = flat.T                                   # short side first, as the solver takes it
        tied_rows = int(((W == W.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum())
        if case.regime[s] == "lists":
            assert stats["dense_min"] == 0 and stats["dense_ties"] == 0 and stats["dense_rows"] == 0, (name, s, stats)
            assert tied_rows >= 1, (name, s)
        elif case.regime[s] == "overflow":
            assert stats["dense_rows"] > 0 and stats["dense_ties"] > 0, (name, s, stats)
            assert tied_rows >= 1, (name, s)
    if name in ("dup10", "dup30"):                   # identical short-side rows and long-side columns
        sc = case.batch.scenes[0]
        for v in range(3):
            assert len(np.unique(sc.views[v], axis=0)) < len(sc.views[v])
    if name == "inf_feasible":
        assert all(np.isinf(_flat(sc)).any() for sc in case.batch.scenes)


# --------------------------------------------- the float32 block minima ----
def _block_model(sc):
    """(approximate bits, exact bits) int64 [N, ceil(M/32), P] of a rectified
    scene's 32-column block minima: the kernel's float32 form (e12 padded with
    0, e23 with +inf past the view) and float32(min fp64 sum / 3)."""
    y0, y1, y2 = sc.ys
    e12, e13, e23 = CI.closed_form_pair(y0, y1), CI.closed_form_pair(y0, y2), CI.closed_form_pair(y1, y2)
    N, M, P = sc.counts
    nb = (M + 31) // 32
    a12 = np.zeros((N, nb * 32))
    a12[:, :M] = e12
    a23 = np.full((nb * 32, P), np.inf)
    a23[:M] = e23
    s64 = (a12[:, :, None] + e13[:, None, :]) + a23[None, :, :]
    exact = (s64.reshape(N, nb, 32, P).min(axis=2) / 3.0).astype(np.float32)
    v = a12.astype(np.float32)[:, :, None] + a23.astype(np.float32)[None, :, :]
    m32 = v.reshape(N, nb, 32, P).min(axis=2)
    approx = ((m32 + e13.astype(np.float32)[:, None, :]) * np.float32(1.0 / 3.0)).astype(np.float32)
    return approx.view(np.uint32).astype(np.int64), exact.view(np.uint32).astype(np.int64)


def _ok(bits):
    lo = bits & 0xFFFF
    return (lo >= MARGIN) & (lo <= 0xFFFF - MARGIN) & (bits >= TINY)


def test_straddle_needs_the_recheck(minima):
    assert len(CI.straddle_sums()) >= 30
    for sc in minima["straddle"].scenes:
        i, j, k, s = sc.note["straddle"]
        approx, exact = _block_model(sc)
        a, e = approx[i, j // 32, k], exact[i, j // 32, k]
        # the triple is the block's strict minimum, with the sum s
        c = CI.closed_form_cube(*sc.ys)[i, j // 32 * 32:j // 32 * 32 + 32, k]
        assert (c == c.min()).sum() == 1 and c.argmin() == j % 32
        assert c.min().view(np.uint32) == e == np.float32(s / 3.0).view(np.uint32)
        assert CI.key16(a) != CI.key16(e), (hex(a), hex(e))
        lo = a & 0xFFFF
        assert lo < MARGIN or lo > 0xFFFF - MARGIN              # the kernel rechecks ...
        assert not _ok(np.array([a]))[0]
        # ... and everywhere the float32 test passes, the key is already exact
        ok = _ok(approx)
        assert ok.any() and np.array_equal(CI.key16(approx[ok]), CI.key16(exact[ok]))


def test_coarse_grids_fail_the_float32_test(minima):
    fails, blocks = 0, 0
    for sc in minima["coarse"].scenes:
        approx, exact = _block_model(sc)
        ok = _ok(approx)
        assert np.array_equal(CI.key16(approx[ok]), CI.key16(exact[ok]))
        assert np.abs(approx - exact).max() <= 6                # the bound DESIGN 3.11 derives
        fails += int((~ok).sum())
        blocks += ok.size
    assert fails >= 0.5 * blocks, (fails, blocks)


def test_zero_and_tiny_costs_fall_below_tiny(minima):
    zero_blocks = 0
    for sc in minima["coarse"].scenes:
        approx, exact = _block_model(sc)
        z = exact == 0
        zero_blocks += int(z.sum())
        assert (approx[z] < TINY).all() and not _ok(approx[z]).any()
    assert zero_blocks > 1000
    for sc in minima["tiny"].scenes:
        approx, exact = _block_model(sc)
        assert (approx < TINY).all() and not _ok(approx).any()
        lo = approx & 0xFFFF
        # blocks whose lower bits are safe: only the b >= kApproxTiny term
        # sends them to the recheck
        safe = (lo >= MARGIN) & (lo <= 0xFFFF - MARGIN)
        assert (safe & (approx > 0)).mean() > 0.5
        # with IEEE subnormals the float32 form stays within the margin down
        # here too (a subnormal's ulp is absolute: the three conversions, two
        # adds and the multiply err by under two units), so the term guards a
        # flushing float32 mode, not these values
        assert np.abs(approx - exact).max() <= 2
        assert np.array_equal(CI.key16(approx[safe]), CI.key16(exact[safe]))
