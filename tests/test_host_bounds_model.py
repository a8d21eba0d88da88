"""CPU checks of tests/host_bounds.py: the GPU tests of loose host bounds
(test_host_bounds_gpu.py) cannot pass on inputs that miss what they are about.
Every bounds-grid entry holds for its batch (the header's bounds "must hold":
violated bounds are not what is tested), every batch has the properties its
docstring claims, and the expected results exist."""
import numpy as np
import pytest

import host_bounds as H


# ------------------------------------------------------------ assignment ----
def test_lsap_batch_is_the_issues_shapes_twice():
    mats = H.lsap_batch()
    assert len(mats) == 2 * len(H.LSAP_SHAPES) == 38
    assert sorted(set(H.LSAP_SHAPES)) == sorted(H.LSAP_DENSE + H.LSAP_LISTS + H.LSAP_EMPTY)
    for q, shape in enumerate(H.LSAP_SHAPES):
        assert mats[2 * q].shape == mats[2 * q + 1].shape == shape
    for dtype in ("float32", "float64"):
        for m in H.lsap_batch(dtype):
            assert m.dtype == np.dtype(dtype) and not m.flags.writeable


def test_the_ties_really_tie():
    """The tied form holds half-integers only; every tied matrix of 30 or more
    entries repeats values inside a long-side line, so the solver meets equal
    reduced costs; the normal form has next to no repeated value."""
    for dtype in ("float32", "float64"):
        mats = H.lsap_batch(dtype)
        for q in range(len(H.LSAP_SHAPES)):
            normal, tied = mats[2 * q], mats[2 * q + 1]
            assert np.array_equal(tied * 2, np.round(tied * 2))
            if tied.size >= 30:
                assert np.unique(normal).size > 0.99 * normal.size > np.unique(tied).size
                line = tied if tied.shape[1] >= tied.shape[0] else tied.T
                assert all(np.unique(row).size < row.size for row in line), tied.shape


def test_lsap_expected_is_a_full_assignment():
    for dtype in ("float32", "float64"):
        for m, (r, c) in zip(H.lsap_batch(dtype), H.lsap_expected(dtype)):
            assert r.size == c.size == min(m.shape) and r.dtype == np.int64
            assert np.unique(r).size == r.size and np.unique(c).size == c.size


def test_every_bounds_grid_entry_holds():
    shapes = H.shapes_of(H.lsap_batch())
    grid = H.lsap_bounds_grid(shapes)
    assert list(grid)[0] == "tight" and grid["tight"] == (1, 5000, 64)
    assert grid["loosest"] == (1, 2 ** 62, 2 ** 62) and grid["capacity"] == (1, 65536, 1024)
    assert {f"L{L}" for L in (5000, 8192, 8193, 65536, 65537)} <= set(grid) and len(grid) == 9
    for name, b in grid.items():
        assert H.bounds_hold(b, shapes), name
    # loose: above every real size and across class limits no problem reaches
    # (8192: the 256-thread workspace class, 65536: the split-register and
    # candidate-list classes)
    long_maxes = [b[1] for b in grid.values()]
    assert H.crossed((1024, 4096, 8192, 65536), 5000, long_maxes) == {8192, 65536}
    assert H.straddles(long_maxes, 8192, 8193) and H.straddles(long_maxes, 65536, 65537)
    assert not H.bounds_hold((1, 4999, 64), shapes) and not H.bounds_hold((2, 5000, 64), shapes)
    assert not H.bounds_hold((1, 5000, 63), shapes)


def test_sub_batches_leave_classes_without_work():
    shapes = H.shapes_of(H.lsap_batch())
    sub = H.lsap_sub_batches()
    pick = lambda name: [shapes[k] for k in sub[name]]
    assert pick("upto64") and all(0 < min(s) and max(s) <= 64 for s in pick("upto64"))
    assert sorted(set(pick("empties"))) == [(0, 4), (4, 0)] and len(sub["empties"]) == 4
    assert sorted(set(pick("workgroup"))) == [(1100, 5), (2500, 11)] and len(sub["workgroup"]) == 4
    assert set(pick("lists")) == {(4500, 64)} and len(sub["lists"]) == 2
    for name in sub:
        assert H.bounds_hold(H.LOOSEST, pick(name)) and H.bounds_hold(H.CAPACITY, pick(name))
    assert H.tight_bounds(pick("empties")) == (0, 0, 0)


def test_batch_y_statuses_per_the_oracle():
    """The second batch differs from the first in shapes and count, fits the
    capacity bounds, and oracle/lsap.py gives its NaN problem status 1 and its
    all-+inf column status 2, each between valid problems and both of the
    candidate-list class (long side >= 4096, short side <= 1024)."""
    y = H.lsap_batch_y()
    assert [H.oracle_status(m) for m in y] == list(H.LSAP_Y_STATUS)
    assert H.LSAP_Y_STATUS[0] == 0 and H.LSAP_Y_STATUS[2] == 0 and H.LSAP_Y_STATUS[4] == 0
    for k, st in enumerate(H.LSAP_Y_STATUS):
        if st:
            assert 4096 <= max(y[k].shape) <= 65536 and min(y[k].shape) <= 1024
            assert H.lsap_expected_y()[k] is None
    assert np.isnan(y[1]).sum() == 1 and np.isposinf(y[3][:, 2]).all()
    assert not set(H.shapes_of(y)) & set(H.LSAP_SHAPES)
    assert H.bounds_hold(H.CAPACITY, H.shapes_of(y)) and H.bounds_hold(H.CAPACITY, H.shapes_of(H.lsap_batch()))


# ------------------------------------------------------------------ cubes ----
@pytest.mark.parametrize("name", sorted(H.CUBE_SETS))
def test_cube_max_n_cross_limits_no_view_reaches(name):
    counts, max_ns = H.CUBE_SETS[name]
    b = H.cube_batch(name)
    assert {v for c in counts for v in c} == H.CUBE_VIEWS[name] and 3 <= len(counts) <= 4
    assert max_ns[0] == b.max_view == max(H.CUBE_VIEWS[name])          # the tight run
    assert all(m >= b.max_view for m in max_ns)
    # the issue's values, none dropped: both sides of 16 / 17, 64 / 65, 48 / 49, 256 / 257
    assert max_ns == {"v16": (16, 17, 33, 64, 65, 257), "v32": (32, 48, 49, 97, 193, 256, 300),
                      "v100": (100, 128, 161, 256, 257, 520)}[name]
    for lo, hi in {"v16": [(16, 17), (64, 65)], "v32": [(48, 49)], "v100": [(256, 257)]}[name]:
        assert H.straddles(max_ns, lo, hi)
    assert H.crossed(H.CLASS_LIMITS, b.max_view, max_ns) == H.CUBE_CROSSED[name]
    for L in H.CUBE_CROSSED[name]:           # a run on each side of every crossed limit, no view above it
        assert any(m <= L for m in max_ns) and any(m > L for m in max_ns) and b.max_view <= L
    for s, (N, M, P) in enumerate(counts):
        assert b.cubes[s].size == N * M * P and b.amins[s].size == N * M == b.mins[s].size
        assert b.bm8[s].size == (N * ((M + 7) // 8) * P if N * M * P else 0)


def test_bmin8_batch_is_of_the_list_class():
    b = H.bmin8_batch()
    for (N, M, P), st in zip(b.counts, b.status):
        assert 70 <= min(N, M, P) and max(N, M, P) <= 100 and st == 0
        assert 4096 <= N * M <= 65536 and P <= 1024
    assert H.bounds_hold(H.CAPACITY, [(N * M, P) for N, M, P in b.counts])


def test_chain_batches():
    """Both chain batches: views of 64..100 (N * M >= 4096: the cube-free
    class), max_n values >= every view and across 128 and up to the 256 limit;
    batch Y's scene 1 has NaN entries (status 1), its scene 2 an all-+inf
    column (status 2), per oracle/lsap.py on the oracle's cubes."""
    x, y = H.chain_batch("x"), H.chain_batch("y")
    for b in (x, y):
        for N, M, P in b.counts:
            assert 64 <= min(N, M, P) and max(N, M, P) <= 100 and N * M >= 4096
    assert x.status == (0, 0) and y.status == H.CHAIN_Y_STATUS == (0, 1, 2, 0)
    assert np.isnan(y.cubes[1]).any() and not np.isnan(y.cubes[2]).any()
    assert np.isposinf(y.flat(2)[:, 3]).all() and np.isfinite(y.flat(2)[:, 4]).all()
    assert H.CHAIN_MAX_N[0] == x.max_view and all(m >= x.max_view for m in H.CHAIN_MAX_N)
    assert H.CHAIN_CAPACITY >= max(x.max_view, y.max_view) and H.CHAIN_CAPACITY in H.CHAIN_MAX_N
    assert sorted(x.counts) != sorted(y.counts) and x.S != y.S
    r = x.residuals(128)
    assert r.shape == (2, 3, 128, 128) and np.isnan(r[0, 0, 64:, :]).all()


# --------------------------------------------------------------- pairwise ----
@pytest.mark.parametrize("C", [3, 4])
def test_pair_batches(C):
    b = H.pair_batch(C)
    assert {v for c in H.PAIR_COUNTS[C] for v in c} == H.PAIR_VIEWS
    max_ns = H.pair_max_ns(C)
    assert max_ns[:6] == (300, 301, 512, 1024, 1025, 2600) and all(m >= 300 for m in max_ns)
    assert H.crossed(H.CLASS_LIMITS, 300, max_ns) == {1024} and H.straddles(max_ns, 1024, 1025)
    assert H.straddles(max_ns, 300, 301) and H.straddles(H.PAIR_F64_MAX_N, 300, 1025)
    # the launch's own rule for 4 write fronts: the padded bound reaches 8 GB
    # at the last max_n and not one below it
    sp = b.S * len(b.pairs)
    assert float(sp) * max_ns[-1] ** 2 * 4 >= 8e9 > float(sp) * (max_ns[-1] - 1) ** 2 * 4
    assert all(float(sp) * m * m * 4 < 8e9 for m in max_ns[:-1])
    assert max_ns[-1] == {3: 12910, 4: 9129}[C]
    assert np.isnan(b.pts).any() and np.isinf(b.pts).any() and (b.F[len(b.pairs) + 2] == 0).all()
    assert any(np.isnan(m).any() for m in b.mats) and any((m == np.float32(9999.0)).any() for m in b.mats)
    assert any(a.size and (a == -1).all() for a in b.amins)              # an empty view b
    for q, e in enumerate(b.f64()):
        assert e.shape == b.mats[q].shape
        with np.errstate(over="ignore"):
            assert np.array_equal(e.astype(np.float32).view(np.uint32), b.mats[q].view(np.uint32))


def test_extend_and_graph_bounds():
    assert H.EXTEND_MAX_ROWS[0] == max(H.EXTEND_COUNTS) and all(m >= 65 for m in H.EXTEND_MAX_ROWS)
    assert H.crossed((64, 128, 1024), 65, H.EXTEND_MAX_ROWS) == {128, 1024}
    for which in (0, 1):
        g = H.graph_batch(which)
        assert max(max(c) for c in H.GRAPH_PAIR_COUNTS[which]) <= 300 < H.GRAPH_PAIR_MAX_N
        assert g.cube.max_view <= 100 < H.GRAPH_CUBE_MAX_N
        assert g.dist.size == g.dist_offs[-1] and g.cube_offs[-1] == sum(c.size for c in g.cube.cubes)
    a, b = H.graph_batch(0), H.graph_batch(1)
    assert a.p_co.size == b.p_co.size and a.cube.co.size == b.cube.co.size    # same scene counts
    assert not np.array_equal(a.p_co, b.p_co) and not np.array_equal(a.cube.co, b.cube.co)


def test_select_sort_drops_pairs_that_are_no_indices():
    """oracle/pipeline.select_sort, the checker of the select kernels: a pair
    with r outside [0, N*M) or c outside [0, P) is dropped, the others are
    selected as if the dropped ones were not there."""
    from oracle import pipeline as OP
    cube = np.arange(24, dtype=np.float32)[::-1].copy()            # N*M = 6 rows, P = 4
    r = np.array([5, -1, 6, 0, 2 ** 63 - 1, 3, -2 ** 63 + 7, 1], np.int64)
    c = np.array([3, 0, 0, 4, 1, -1, 2, 2], np.int64)
    m, v = OP.select_sort(cube, 2, 4, r, c, float("inf"))
    wm, wv = OP.select_sort(cube, 2, 4, r[[0, 7]], c[[0, 7]], float("inf"))
    assert np.array_equal(m, wm) and np.array_equal(v, wv) and v.tolist() == [0.0, 17.0]
    assert OP.select_sort(np.zeros(0, np.float32), 5, 16, r, c, 30.0)[0].shape == (0, 3)
    assert OP.select_sort(np.zeros(0, np.float32), 5, 0, r, c, 30.0)[1].size == 0
