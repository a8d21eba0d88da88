"""Loose host bounds, the plain assignment entry points and buffer reuse.

include/mvmatch.h lets the host pass UPPER bounds (max_n, long_max, short_max,
max_rows; long_min a lower one) while the real sizes stay on the device, so a
caller sizes once for a capacity and feeds batches whose counts change.  The
plans, and with them every other GPU test, pass the batch's exact maxima.
Here every hot-path op is called directly with bounds above every real size
and across the limits at which the host picks another kernel class, lane
shape, grid or LDS size (tests/host_bounds.py builds the batches and grids,
test_host_bounds_model.py pins their properties on the CPU), and:

* outputs equal the oracle's / scipy's AND the tight-bound run's, bit for bit;
* every output lies in a sentinel-filled buffer that is compared whole, and
  status arrays start from a value that is no status, so a problem no kernel
  class claimed, or one two classes wrote, shows;
* a second, different batch runs into the same workspace and outputs, and a
  graph captured with capacity bounds is replayed on new device data.

The bounds always hold: the header says they must (the kernels size LDS from
them).  No tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import host_bounds as H
import layouts as L
from test_gpu_parity import CUBE_PATHS
from test_layouts_gpu import TAIL, _assert_tail, _host, _opts, _t, _ws_bytes
from test_lsap_gpu import LSAP_PATHS

pytestmark = pytest.mark.gpu

PAD = 64              # sentinel elements behind an index or status array


def _blank(n, dtype, dev):
    """A device buffer of n elements holding the sentinel of ``dtype``."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return torch.full((int(n),), L.U8_SENTINEL, dtype=torch.uint8, device=dev)
    return _t(L.blank(n, dtype), dev)


def _same(got, want, what):
    """Whole arrays bit for bit (floats as bit patterns)."""
    g, w = L._bits(np.asarray(got)).reshape(-1), L._bits(np.asarray(want)).reshape(-1)
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:5]}"


def _tight_layout(offs, n_total):
    offs = np.asarray(offs, np.int64)
    return L.Layout("tight", 1, offs[:-1].copy(), np.diff(offs), int(n_total))


# ============================================================ assignment ====
class _Lsap:
    """One assignment batch on the device: the plan's offsets, the costs in a
    gapped layout, the expected index images (sentinel outside the regions; a
    failed problem's region is not compared) and statuses."""

    def __init__(self, dev, mats, expected, statuses=None):
        from bpc_baseline_amd import ops
        self.mats, self.expected, self.n = mats, expected, len(mats)
        self.statuses = [0] * self.n if statuses is None else list(statuses)
        dtype = mats[0].dtype
        self.plan = ops.LsapPlan([m.shape[0] for m in mats], [m.shape[1] for m in mats], device=dev,
                                 dtype=torch.float32 if dtype == np.float32 else torch.float64)
        lay = L.layout([m.size for m in mats], "gaps", 1, seed=self.n)
        self.cost, self.cost_offs = _t(L.image(lay, dtype, list(mats)), dev), _t(lay.offs, dev)
        self.nws, self.n_out = self.plan.workspace.numel(), self.plan.n_out
        self.out_lay = _tight_layout(self.plan.out_offs_host, self.n_out)
        self.shapes = H.shapes_of(mats)

    def solve(self, bounds, opts, ws, ri, ci, st):
        p = self.plan
        torch.ops.mvmatch.lsap_solve_out(self.cost, self.cost_offs, p.dims, p.ws_offs, p.out_offs, ws[:self.nws],
                                         ri, ci, st[:self.n], bounds[0], bounds[1], opts, bounds[2])

    def fresh(self, dev):
        return (_blank(self.nws + TAIL, np.uint8, dev), _blank(self.n_out + PAD, np.int64, dev),
                _blank(self.n_out + PAD, np.int64, dev), _blank(self.n + PAD, np.int32, dev))

    def check_regions(self, ri, ci, st, tag):
        """Statuses and, for the solved problems, scipy's assignment."""
        r, c, s = _host(ri), _host(ci), _host(st)
        assert list(s[:self.n]) == self.statuses, (tag, list(s[:self.n]))
        o = self.plan.out_offs_host
        for k in range(self.n):
            if self.statuses[k] == 0:
                assert np.array_equal(r[o[k]:o[k + 1]], self.expected[k][0]) and \
                    np.array_equal(c[o[k]:o[k + 1]], self.expected[k][1]), (tag, k, self.shapes[k])

    def check_whole(self, ws, ri, ci, st, tag):
        """... and nothing else written: the index arrays whole, the tails."""
        assert all(x == 0 for x in self.statuses)
        self.check_regions(ri, ci, st, tag)
        for got, col, what in ((ri, 0, "row_ind"), (ci, 1, "col_ind")):
            want = L.image(self.out_lay, np.int64, [e[col] for e in self.expected], tail=PAD)
            L.assert_image(_host(got), want, self.out_lay, f"{what}, {tag}")
        _assert_tail(st, self.n, f"status, {tag}")
        _assert_tail(ws, self.nws, f"workspace, {tag}")


@functools.lru_cache(maxsize=None)
def _lsap_x(dev, dtype):
    return _Lsap(dev, H.lsap_batch(dtype), H.lsap_expected(dtype))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("path", H.LSAP_OPTION_SETS)
def test_lsap_loose_bounds(cuda, path, dtype):
    """The ragged batch of every kernel class in one launch under every entry
    of the bounds grid: each status 0 (from a non-status fill), each assignment
    scipy's, row_ind / col_ind whole and equal to the tight-bound run's."""
    b = _lsap_x(cuda, dtype)
    opts = _opts(LSAP_PATHS[path])
    base = None
    for name, bounds in H.lsap_bounds_grid(b.shapes).items():
        assert H.bounds_hold(bounds, b.shapes)
        ws, ri, ci, st = b.fresh(cuda)
        b.solve(bounds, opts, ws, ri, ci, st)
        tag = f"{path}/{dtype}, bounds {name} {bounds}"
        b.check_whole(ws, ri, ci, st, tag)
        got = (_host(ri), _host(ci), _host(st))
        if base is None:
            assert name == "tight"
            base = got
        for g, w, what in zip(got, base, ("row_ind", "col_ind", "status")):
            _same(g, w, f"{what} against the tight run, {tag}")


@pytest.mark.parametrize("path", H.LSAP_OPTION_SETS)
def test_lsap_classes_launched_without_work(cuda, path):
    """Sub-batches under the loosest bound: every kernel class is launched and
    most find no problem of theirs; every problem is still solved by exactly
    one (status 0 from a non-status fill, scipy's assignment, nothing else
    written), as under the sub-batch's own tight bounds."""
    opts = _opts(LSAP_PATHS[path])
    for dtype in ("float32", "float64"):
        mats, want = H.lsap_batch(dtype), H.lsap_expected(dtype)
        for name, idx in H.lsap_sub_batches().items():
            b = _Lsap(cuda, [mats[k] for k in idx], [want[k] for k in idx])
            for bounds in (H.tight_bounds(b.shapes), H.LOOSEST):
                ws, ri, ci, st = b.fresh(cuda)
                b.solve(bounds, opts, ws, ri, ci, st)
                b.check_whole(ws, ri, ci, st, f"{path}/{dtype}, sub-batch {name}, bounds {bounds}")


def test_plain_entry_points(cuda):
    """mvm_lsap_solve and mvm_lsap_solve_bounded (tight and (1, 65537) bounds)
    through ctypes with mvm_lsap_plan's offsets, and lsap_solve_out with its
    default long_max / short_max, on the float32 batch: scipy's assignments,
    status 0 everywhere, nothing else written."""
    from bpc_baseline_amd import _native
    lib = _native.load()
    b = _lsap_x(cuda, "float32")
    n = b.n
    rows = np.ascontiguousarray([s[0] for s in b.shapes], np.int64)
    cols = np.ascontiguousarray([s[1] for s in b.shapes], np.int64)
    ws_offs, out_offs = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    total = lib.mvm_lsap_plan(n, rows.ctypes.data, cols.ctypes.data, ws_offs.ctypes.data, out_offs.ctypes.data)
    assert total == b.nws and np.array_equal(out_offs, b.plan.out_offs_host)
    assert np.array_equal(ws_offs, b.plan.ws_offs_host)
    dims = _t(np.stack([rows, cols], axis=1).reshape(-1), cuda)
    wo, oo = _t(ws_offs, cuda), _t(out_offs, cuda)
    stream = torch.cuda.current_stream(cuda).cuda_stream
    lo, hi, _ = H.tight_bounds(b.shapes)

    def plain(ws, ri, ci, st):
        return lib.mvm_lsap_solve(b.cost.data_ptr(), b.cost_offs.data_ptr(), dims.data_ptr(), n, wo.data_ptr(),
                                  oo.data_ptr(), ws.data_ptr(), total, ri.data_ptr(), ci.data_ptr(),
                                  st.data_ptr(), stream)

    def bounded(long_min, long_max):
        def call(ws, ri, ci, st):
            return lib.mvm_lsap_solve_bounded(b.cost.data_ptr(), b.cost_offs.data_ptr(), dims.data_ptr(), n,
                                              wo.data_ptr(), oo.data_ptr(), ws.data_ptr(), total, ri.data_ptr(),
                                              ci.data_ptr(), st.data_ptr(), long_min, long_max, stream)
        return call

    def op_defaults(ws, ri, ci, st):
        torch.ops.mvmatch.lsap_solve_out(b.cost, b.cost_offs, dims, wo, oo, ws[:total], ri, ci, st[:n])
        return 0

    for what, call in (("mvm_lsap_solve", plain), ("mvm_lsap_solve_bounded tight", bounded(lo, hi)),
                       ("mvm_lsap_solve_bounded (1, 65537)", bounded(1, 65537)),
                       ("lsap_solve_out defaults", op_defaults)):
        ws, ri, ci, st = b.fresh(cuda)
        _native.check(what, call(ws, ri, ci, st))
        torch.cuda.synchronize(cuda)
        b.check_whole(ws, ri, ci, st, what)


def test_bmin8_assignment_under_capacity_bounds(cuda):
    """mvm_lsap_solve_ex3 reducing the 8-row minima of two flattened cubes of
    70..100 detections per view under (1, 65536, 1024): scipy's assignment on
    the oracle's cube, and the tight-bound run's."""
    from bpc_baseline_amd import ops
    b = H.bmin8_batch()
    plan = ops.TripletPlan(b.co, b.S, device=cuda)
    bm8 = _blank(plan.n_bmin8, np.int16, cuda)
    cube, _, _ = ops.triplet_cost_argmin(_t(b.pts, cuda), _t(b.co, cuda), _t(b.F, cuda), plan, bmin8=bm8)
    _same(_host(cube), np.concatenate(b.cubes), "cube")
    c3 = np.asarray(b.counts, np.int64)
    lp = ops.LsapPlan(c3[:, 0] * c3[:, 1], c3[:, 2], device=cuda)
    nws, base = lp.workspace.numel(), None
    lay = _tight_layout(lp.out_offs_host, lp.n_out)
    for bounds in ((lp.long_min, lp.long_max, lp.short_max), H.CAPACITY):
        ws, ri, ci, st = (_blank(nws + TAIL, np.uint8, cuda), _blank(lp.n_out + PAD, np.int64, cuda),
                          _blank(lp.n_out + PAD, np.int64, cuda), _blank(b.S + PAD, np.int32, cuda))
        torch.ops.mvmatch.lsap_solve_bmin8_out(cube, plan.cube_offs[:-1].contiguous(), lp.dims, lp.ws_offs,
                                               lp.out_offs, ws[:nws], ri, ci, st[:b.S], bm8, plan.bmin8_offs,
                                               plan.segs, bounds[0], bounds[1], bounds[2], None)
        tag = f"bounds {bounds}"
        assert list(_host(st)[:b.S]) == [0] * b.S, tag
        for got, col, what in ((ri, 0, "row_ind"), (ci, 1, "col_ind")):
            L.assert_image(_host(got), L.image(lay, np.int64, [a[col] for a in b.assignment], tail=PAD), lay,
                           f"{what}, {tag}")
        _assert_tail(st, b.S, f"status, {tag}")
        _assert_tail(ws, nws, f"workspace, {tag}")
        got = (_host(ri), _host(ci))
        base = base or got
        _same(got[0], base[0], f"row_ind against tight, {tag}")
        _same(got[1], base[1], f"col_ind against tight, {tag}")


# ========================================================== cube + bmin8 ====
def _cube_cases():
    for name, (_, max_ns) in H.CUBE_SETS.items():
        for path in H.CUBE_ARGMIN_PATHS:
            if path != "small" or max_ns[0] < H.SMALL_KERNEL_BELOW:
                yield name, path


@pytest.mark.parametrize("name,path", list(_cube_cases()))
def test_cube_loose_max_n(cuda, name, path):
    """triplet_cost_argmin_out (and triplet_cost_bmin8_out on its paths) with
    max_n above every view and across the kernel, lane-shape and tile limits:
    cube, argmin, minimum and 8-row minima whole in gapped buffers, equal to
    the oracle's and to the tight run's; the offsets are the caller's, so the
    images do not move with max_n."""
    b = H.cube_batch(name)
    max_ns = [m for m in H.CUBE_SETS[name][1] if path != "small" or m < H.SMALL_KERNEL_BELOW]
    assert max_ns[0] == b.max_view and len(max_ns) >= 3
    P_, C_, F_ = _t(b.pts, cuda), _t(b.co, cuda), _t(b.F, cuda)
    opts = _opts(CUBE_PATHS[path])
    lc = L.layout([c.size for c in b.cubes], "gaps", 4, seed=1)
    lr = L.layout([a.size for a in b.amins], "gaps", 1, seed=2)
    lb = L.layout([k.size for k in b.bm8], "gaps", 4, seed=3)
    want = (L.image(lc, np.float32, b.cubes), L.image(lr, np.int32, b.amins), L.image(lr, np.float32, b.mins),
            L.image(lb, np.uint16, b.bm8))
    offs = [_t(x.offs, cuda) for x in (lc, lr, lb)]
    for with_bm8 in (False, True) if path in H.CUBE_BMIN8_PATHS else (False,):
        base = None
        for max_n in max_ns:
            wsb = _ws_bytes(b.S, max_n)
            cube, amin, mn = (_blank(lc.total, np.float32, cuda), _blank(lr.total, np.int32, cuda),
                              _blank(lr.total, np.float32, cuda))
            keys = _blank(lb.total, np.int16, cuda)
            ws = _blank(wsb + TAIL, np.uint8, cuda)
            if with_bm8:
                torch.ops.mvmatch.triplet_cost_bmin8_out(P_, C_, F_, b.S, max_n, offs[0], offs[1], cube, amin, mn,
                                                         keys, offs[2], ws[:wsb], opts)
            else:
                torch.ops.mvmatch.triplet_cost_argmin_out(P_, C_, F_, b.S, max_n, offs[0], offs[1], cube, amin,
                                                          mn, ws[:wsb], opts)
            tag = f"{name}/{path}/{'bmin8' if with_bm8 else 'argmin'}, max_n {max_n}"
            got = (_host(cube), _host(amin), _host(mn), _host(keys, np.uint16))
            L.assert_image(got[0], want[0], lc, f"cube, {tag}")
            L.assert_image(got[1], want[1], lr, f"argmin, {tag}")
            L.assert_image(got[2], want[2], lr, f"minval, {tag}")
            L.assert_image(got[3], want[3] if with_bm8 else L.blank(lb.total, np.uint16), lb, f"bmin8, {tag}")
            _assert_tail(ws, wsb, f"workspace, {tag}")
            base = base or got
            for g, w, what in zip(got, base, ("cube", "argmin", "minval", "bmin8")):
                _same(g, w, f"{what} against the tight run, {tag}")


# ============================================================== pairwise ====
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("opt", sorted(H.PAIR_OPTIONS))
def test_pairwise_loose_max_n(cuda, C, opt):
    """pairwise_residual_argmin_out at row_align 1 and 32 with max_n from the
    tight 300 over the column-tile limit (1024 / 1025) up to the max_n at which
    the launch's own rule picks 4 XCD write fronts on this tiny batch: the
    matrices (padding +inf), argmins and minima whole, the oracle's and the
    tight run's, NaN / inf centroids and degenerate F included."""
    b = H.pair_batch(C)
    P_, C_, F_ = _t(b.pts, cuda), _t(b.co, cuda), _t(b.F, cuda)
    opts = _opts(H.PAIR_OPTIONS[opt])
    pa, pb = [int(x) for x in b.pairs[:, 0]], [int(x) for x in b.pairs[:, 1]]
    for row_align in (1, 32):
        regions = b.pitched(row_align)
        ld_ = L.layout([r.size for r in regions], "gaps", row_align, seed=10 + row_align)
        lr = L.layout([a.size for a in b.amins], "gaps", 1, seed=20 + row_align)
        want = (L.image(ld_, np.float32, regions), L.image(lr, np.int32, b.amins), L.image(lr, np.float32, b.mins))
        od, orow = _t(ld_.offs, cuda), _t(lr.offs, cuda)
        base = None
        for max_n in H.pair_max_ns(C):
            dist, amin, mn = (_blank(ld_.total, np.float32, cuda), _blank(lr.total, np.int32, cuda),
                              _blank(lr.total, np.float32, cuda))
            torch.ops.mvmatch.pairwise_residual_argmin_out(P_, C_, F_, pa, pb, b.S, C, max_n, od, orow, dist, amin,
                                                           mn, opts, row_align)
            tag = f"C {C}/{opt}, row_align {row_align}, max_n {max_n}"
            got = (_host(dist), _host(amin), _host(mn))
            L.assert_image(got[0], want[0], ld_, f"dist, {tag}")
            L.assert_image(got[1], want[1], lr, f"argmin, {tag}")
            L.assert_image(got[2], want[2], lr, f"minval, {tag}")
            base = base or got
            for g, w, what in zip(got, base, ("dist", "argmin", "minval")):
                _same(g, w, f"{what} against the tight run, {tag}")


@pytest.mark.parametrize("C", [3, 4])
def test_pairwise_f64_loose_max_n(cuda, C):
    """pairwise_residual_f64_out with ld and mat_stride the tight ones and
    max_n 300, 301 and 1025: every defined entry the oracle's; of the padding,
    columns n_b .. min(ld, roundup(n_b, 256)) - 1 of rows i < n_a hold +inf and
    nothing else is written (include/mvmatch.h), whatever max_n."""
    b = H.pair_batch(C)
    want = b.f64()
    na, nb = b.na, b.nb
    ld = (int(nb.max()) + 3) // 4 * 4
    stride = int(na.max()) * ld + 4
    lay = L.Layout("strided", 1, np.arange(na.size, dtype=np.int64) * stride, np.full(na.size, stride, np.int64),
                   na.size * stride)
    regions = []
    for q in range(na.size):
        r = L.blank(stride, np.float64)
        m = r[:na[q] * ld].reshape(na[q], ld)
        m[:, nb[q]:min(ld, (nb[q] + 255) // 256 * 256)] = np.inf
        m[:, :nb[q]] = want[q]
        regions.append(r)
    image = L.image(lay, np.float64, regions, tail=PAD)
    P_, C_, F_ = _t(b.pts, cuda), _t(b.co, cuda), _t(b.F, cuda)
    pa, pb = [int(x) for x in b.pairs[:, 0]], [int(x) for x in b.pairs[:, 1]]
    base = None
    for max_n in H.PAIR_F64_MAX_N:
        e = _blank(lay.total + PAD, np.float64, cuda)
        torch.ops.mvmatch.pairwise_residual_f64_out(P_, C_, F_, pa, pb, b.S, C, max_n, stride, ld, e)
        got = _host(e)
        L.assert_image(got, image, lay, f"e, C {C}, max_n {max_n}")
        base = got if base is None else base
        _same(got, base, f"e against the tight run, C {C}, max_n {max_n}")


# ======================================================= cube-free chain ====
class _ChainBufs:
    """Workspaces and outputs of the cube-free chain for a capacity: S scenes
    of views up to max_n, n_out assignment rows, nws bytes of list workspace."""

    def __init__(self, dev, batches, max_n):
        self.S = max(b.S for b in batches)
        self.plans = {id(b): self._plans(b, dev) for b in batches}
        self.n8 = max(int(p[1].total) for p in self.plans.values())
        self.n32 = max(int(p[2].total) for p in self.plans.values())
        self.n_out = max(p[0].n_out for p in self.plans.values())
        self.nws = max(p[0].workspace.numel() for p in self.plans.values())
        self.wsb = _ws_bytes(self.S, max_n)
        self.k8 = _blank(self.n8 + PAD, np.int16, dev)
        self.k32 = _blank(self.n32 + PAD, np.int16, dev)
        self.resid = _blank(self.wsb + TAIL, np.uint8, dev)
        self.ws = _blank(self.nws + TAIL, np.uint8, dev)
        self.ri, self.ci = _blank(self.n_out + PAD, np.int64, dev), _blank(self.n_out + PAD, np.int64, dev)
        self.st = _blank(self.S + PAD, np.int32, dev)
        cap = self.n_out + PAD
        self.outs = (_blank(3 * cap, np.int32, dev).view(cap, 3), _blank(cap, np.float32, dev),
                     _blank(3 * cap, np.float64, dev).view(cap, 3), _blank(self.S + PAD, np.int32, dev))
        self.proj = _t(np.random.default_rng(12).normal(size=(self.S, 3, 3, 4)), dev)

    @staticmethod
    def _plans(b, dev):
        from bpc_baseline_amd import ops
        c3 = np.asarray(b.counts, np.int64)
        lres = ops.LsapPlan(c3[:, 0] * c3[:, 1], c3[:, 2], device=dev, resid=True)
        return lres, L.layout([k.size for k in b.bm8], "tight", 4), L.layout([k.size for k in b.bm32], "tight", 16)


def _chain_run(dev, b, max_n, bounds, bufs):
    """minima -> assignment -> select of batch ``b`` into ``bufs`` (no buffer
    is cleared here).  A failed problem's index region holds no assignment but
    whatever it held before (the sentinel, an earlier batch's indices); it goes
    to the select kernel untouched, which ignores the pairs that are no indices
    of the scene.  -> host copies."""
    lres, l8, l32 = bufs.plans[id(b)]
    S, wsb = b.S, _ws_bytes(b.S, max_n)
    P_, C_, F_ = _t(b.pts, dev), _t(b.co, dev), _t(b.F, dev)
    o8, o32 = _t(l8.offs, dev), _t(l32.offs, dev)
    segs = _t(np.asarray(b.counts, np.int64)[:, 1], dev)
    torch.ops.mvmatch.triplet_minima_out(P_, C_, F_, S, max_n, bufs.k8, o8, bufs.k32, o32, bufs.resid[:wsb], None)
    nws = lres.workspace.numel()
    torch.ops.mvmatch.lsap_solve_resid_out(lres.dims, lres.ws_offs, lres.out_offs, bufs.ws[:nws], bufs.ri, bufs.ci,
                                           bufs.st[:S], bufs.k8, o8, bufs.k32, o32, segs, bufs.resid[:wsb], max_n,
                                           bounds[0], bounds[1], bounds[2], None)
    res = dict(k8=_host(bufs.k8, np.uint16), k32=_host(bufs.k32, np.uint16), resid=_host(bufs.resid),
               ws=_host(bufs.ws), ri=_host(bufs.ri), ci=_host(bufs.ci), st=_host(bufs.st))
    assert list(res["st"][:S]) == list(b.status), (max_n, bounds, list(res["st"][:S]))
    n_out = lres.n_out
    match, cost, X, count = bufs.outs
    torch.ops.mvmatch.select_triangulate_resid_out(bufs.resid[:wsb], max_n, C_, lres.out_offs, bufs.ri[:n_out],
                                                   bufs.ci[:n_out], P_, bufs.proj[:S].contiguous(), float("inf"),
                                                   match, cost, X, count[:S])
    res.update(match=_host(match), cost=_host(cost), X=_host(X), count=_host(count))
    return res


def _chain_check(b, max_n, res, bufs, tag, whole):
    """``res`` against the oracle for batch ``b``: the keys, the residuals'
    defined entries, scipy's assignment on the oracle's cube, select_sort's
    matches, order and costs -- for a failed scene select_sort's over whatever
    its index region held (pairs that are no indices of the scene dropped).
    whole: the buffers started from the sentinel, so everything outside the
    regions and the kept rows still holds it."""
    lres, l8, l32 = bufs.plans[id(b)]
    S, o = b.S, lres.out_offs_host
    if whole:
        L.assert_image(res["k8"], L.image(l8, np.uint16, b.bm8, tail=bufs.n8 + PAD - l8.total), l8, f"bmin8, {tag}")
        L.assert_image(res["k32"], L.image(l32, np.uint16, b.bm32, tail=bufs.n32 + PAD - l32.total), l32,
                       f"bm32, {tag}")
        for key, n in (("resid", _ws_bytes(S, max_n)), ("ws", lres.workspace.numel()), ("st", S)):
            tail = res[key][n:]
            assert (tail == L.sentinel(tail.dtype)).all(), f"{key} written past its {n} elements, {tag}"
        for key in ("ri", "ci"):
            tail = res[key][lres.n_out:]
            assert (tail == L.I64_SENTINEL).all(), f"{key} written past its {lres.n_out} elements, {tag}"
    else:
        for got, lay, want in ((res["k8"], l8, b.bm8), (res["k32"], l32, b.bm32)):
            for s in range(S):
                _same(got[lay.offs[s]:lay.offs[s] + lay.sizes[s]], want[s], f"keys of scene {s}, {tag}")
    ld = (max_n + 3) // 4 * 4
    got_r = res["resid"][:_ws_bytes(S, max_n)].view(np.float64).reshape(S, 3, max_n, ld)
    want_r = b.residuals(max_n)
    for s, (N, M, P) in enumerate(b.counts):
        for m, (x, y) in enumerate(((N, M), (P, N), (P, M))):
            _same(got_r[s, m, :x, :y], want_r[s, m, :x, :y], f"resid scene {s} matrix {m}, {tag}")
    rows = []
    cap = bufs.n_out + PAD
    want_match, want_cost = L.blank(3 * cap, np.int32).reshape(cap, 3), L.blank(cap, np.float32)
    want_count = L.blank(bufs.S + PAD, np.int32)
    for s, (N, M, P) in enumerate(b.counts):
        r, c = res["ri"][o[s]:o[s + 1]], res["ci"][o[s]:o[s + 1]]     # the select does not write them
        if b.status[s] == 0:
            assert np.array_equal(r, b.assignment[s][0]) and np.array_equal(c, b.assignment[s][1]), (tag, s)
        wm, wc = b.select(s, r, c, float("inf"))
        k = int(res["count"][s])
        assert k == wc.size, (tag, s, k, wc.size)
        assert np.array_equal(res["match"][o[s]:o[s] + k], wm), (tag, s)
        _same(res["cost"][o[s]:o[s] + k], wc, f"cost scene {s}, {tag}")
        want_match[o[s]:o[s] + k], want_cost[o[s]:o[s] + k], want_count[s] = wm, wc, k
        rows.append(np.arange(o[s], o[s] + k))
    rows = np.concatenate(rows)
    if whole:                                # match, cost, count whole; X outside the kept rows
        _same(res["match"], want_match, f"match whole, {tag}")
        _same(res["cost"], want_cost, f"cost whole, {tag}")
        _same(res["count"], want_count, f"count whole, {tag}")
        other = np.setdiff1d(np.arange(cap), rows)
        assert (res["X"][other].view(np.uint64) == L.F64_SENTINEL_BITS).all(), f"X written outside its rows, {tag}"
    return res["count"][:S].copy(), res["match"][rows], res["cost"][rows].view(np.int32), \
        res["X"][rows].view(np.int64)


def test_chain_loose_max_n(cuda):
    """triplet_minima_out -> lsap_solve_resid_out -> select_triangulate_resid_out
    with max_n tight, 128 and 256 (the resid layout's ld and stride follow it)
    and the solve's bounds tight and (4096, 65536, 1024): keys, residuals,
    assignment, matches, order and costs the oracle's; keys, assignment,
    matches, costs and points equal to the tight run's."""
    b = H.chain_batch("x")
    base = None
    for max_n in H.CHAIN_MAX_N:
        for loose in (False, True):
            bufs = _ChainBufs(cuda, [b], max_n)
            lres = bufs.plans[id(b)][0]
            bounds = (4096, 65536, 1024) if loose else (lres.long_min, lres.long_max, lres.short_max)
            tag = f"max_n {max_n}, bounds {bounds}"
            res = _chain_run(cuda, b, max_n, bounds, bufs)
            got = _chain_check(b, max_n, res, bufs, tag, whole=True)
            got += (res["k8"], res["k32"], res["ri"], res["ci"])
            base = base or got
            for g, w, what in zip(got, base, ("count", "match", "cost", "X", "bmin8", "bm32", "row_ind", "col_ind")):
                _same(g, w, f"{what} against the tight run, {tag}")


def test_select_ignores_pairs_that_are_no_indices(cuda):
    """select_triangulate_out (the cube form; the residual form runs in the
    chain tests) over index regions as a failed assignment leaves them: pairs
    of the scene mixed with rows at and past N*M, columns at and past P,
    negative values and the int64 extremes, a scene with an empty view
    included.  Matches, order, costs and counts are select_sort's over the
    pairs that are indices; every output whole."""
    b = H.cube_batch("v16")
    rng = np.random.default_rng(8)
    per = 24
    offs = np.arange(b.S + 1, dtype=np.int64) * per
    ri, ci = np.zeros(b.S * per, np.int64), np.zeros(b.S * per, np.int64)
    bad = np.array([-1, -2 ** 63 + 7, 2 ** 63 - 1, 2 ** 40], np.int64)
    for s, (N, M, P) in enumerate(b.counts):
        r = rng.integers(0, max(N * M, 1), per)
        c = rng.integers(0, max(P, 1), per)
        r[1::4] = np.concatenate([bad, [N * M, N * M + 1]])
        c[2::4] = np.concatenate([bad, [P, P + 1]])
        ri[s * per:(s + 1) * per], ci[s * per:(s + 1) * per] = r, c
    cap = b.S * per + PAD
    match, cost, X, count = (_blank(3 * cap, np.int32, cuda).view(cap, 3), _blank(cap, np.float32, cuda),
                             _blank(3 * cap, np.float64, cuda).view(cap, 3), _blank(b.S + PAD, np.int32, cuda))
    cube_offs = np.concatenate([[0], np.cumsum([c.size for c in b.cubes])]).astype(np.int64)
    proj = _t(np.random.default_rng(12).normal(size=(b.S, 3, 3, 4)), cuda)
    torch.ops.mvmatch.select_triangulate_out(_t(np.concatenate(b.cubes), cuda), _t(cube_offs, cuda), _t(b.co, cuda),
                                             _t(offs, cuda), _t(ri, cuda), _t(ci, cuda), _t(b.pts, cuda), proj,
                                             float("inf"), match, cost, X, count[:b.S])
    want_match, want_cost = L.blank(3 * cap, np.int32).reshape(cap, 3), L.blank(cap, np.float32)
    want_count, kept = L.blank(b.S + PAD, np.int32), []
    for s in range(b.S):
        wm, wc = b.select(s, ri[offs[s]:offs[s + 1]], ci[offs[s]:offs[s + 1]], float("inf"))
        k = wc.size
        want_match[offs[s]:offs[s] + k], want_cost[offs[s]:offs[s] + k], want_count[s] = wm, wc, k
        kept.append(np.arange(offs[s], offs[s] + k))
    assert want_count[2] == 0 and (want_count[[0, 1, 3]] > 0).all() and (want_count[:b.S] < per).all()
    _same(_host(match), want_match, "match")
    _same(_host(cost), want_cost, "cost")
    _same(_host(count), want_count, "count")
    other = np.setdiff1d(np.arange(cap), np.concatenate(kept))
    assert (_host(X)[other].view(np.uint64) == L.F64_SENTINEL_BITS).all(), "X written outside its rows"


# ================================================================ extend ====
def test_extend_loose_max_rows(cuda):
    """extend_costs_out on one C = 5 batch with counts {0, 1, 63, 65} and
    max_rows tight, 66, 128 and 4096 (a grid of workgroups past every count):
    E equals the model of test_extend_gpu.py and the tight run bit for bit,
    and nothing behind the matrices is written."""
    from test_extend_gpu import SENT, CostBatch, _same_bits
    b = CostBatch(91, 5, list(H.EXTEND_COUNTS), H.EXTEND_COLS, True)
    want = b.expected(PAD)
    dev = [_t(x, cuda) for x in (b.pts, b.cam_offs, b.F, b.match, b.match_offs, b.rows.astype(np.int32), b.ext_offs)]
    base = None
    for max_rows in H.EXTEND_MAX_ROWS:
        assert max_rows >= b.rows.max()
        out = _t(np.full(want.size, SENT, np.float32), cuda)
        torch.ops.mvmatch.extend_costs_out(*dev, b.C, max_rows, out)
        got = _host(out)
        _same_bits(got, want)
        base = got if base is None else base
        _same_bits(got, base)


# ===================================== second batch on the same buffers =====
def _sparse_counters(b, ws_host, k):
    from bpc_baseline_amd import _native
    r, c = b.shapes[k]
    off = int(b.plan.ws_offs_host[k]) + int(_native.load().mvm_lsap_sparse_stats_offset(r, c))
    return ws_host[off:off + 16].view(np.int32)


def test_lsap_second_batch_on_the_same_buffers(cuda):
    """One workspace and one set of outputs sized for the larger of two
    batches, bounds (1, 65536, 1024): batch X, then Y (other shapes and data,
    a NaN problem and an infeasible one between valid ones), then X again,
    nothing reallocated or cleared in between; then each batch on a workspace
    of 0x00 and of 0xFF bytes.  Every run gives its own batch's statuses and
    scipy's assignments; the candidate-list counters of the failed problems
    are 0 and those of a solved problem of the class count its steps."""
    x = _lsap_x(cuda, "float32")
    y = _Lsap(cuda, H.lsap_batch_y(), H.lsap_expected_y(), H.LSAP_Y_STATUS)
    nws, n_out, n = max(x.nws, y.nws), max(x.n_out, y.n_out), max(x.n, y.n)
    ws = _blank(nws + TAIL, np.uint8, cuda)
    ri, ci, st = _blank(n_out + PAD, np.int64, cuda), _blank(n_out + PAD, np.int64, cuda), _blank(n + PAD, np.int32, cuda)

    def run(b, tag):
        b.solve(H.CAPACITY, None, ws, ri, ci, st)
        b.check_regions(ri, ci, st, tag)
        if b is y:
            h = _host(ws)
            for k, status in enumerate(y.statuses):
                if status:
                    assert (_sparse_counters(y, h, k) == 0).all(), (tag, k, _sparse_counters(y, h, k))
            assert _sparse_counters(y, h, 6)[3] > 0, tag       # the solved 6000 x 12 problem's steps
        for buf, m, what in ((ws, nws, "workspace"), (ri, n_out, "row_ind"), (ci, n_out, "col_ind"), (st, n, "status")):
            _assert_tail(buf, m, f"{what}, {tag}")

    for step, b in enumerate((x, y, x)):
        run(b, f"step {step} of X, Y, X")
    for fill in (0x00, 0xFF):
        for b, name in ((x, "X"), (y, "Y")):
            ws[:nws].fill_(fill)
            run(b, f"{name} on a workspace of {fill:#04x}")


def test_chain_second_batch_on_the_same_buffers(cuda):
    """The cube-free chain with max_n = 256 and the solve's bounds (4096,
    65536, 1024) over one set of buffers sized for the larger batch: X, Y (a
    NaN scene, status 1, and an infeasible one, status 2, between valid
    ones), X again without clearing; then each batch on list and residual
    workspaces of 0x00 and of 0xFF bytes; and Y once on fresh buffers.  Every
    run equals the oracle for its own batch.  The failed scenes' index regions
    go to the select as the solve left them: in the reused buffers they hold
    X's indices (rows up to 6,999 against a 4,480-row scene), in the fresh ones
    the sentinel; the select keeps what select_sort keeps of them and reads
    nothing outside the scene.  (The candidate-list counters of failed
    problems are checked by the assignment's reuse test: the header's
    mvm_lsap_sparse_stats_offset describes mvm_lsap_plan's regions, and the
    regions of mvm_lsap_plan_resid used here have no such accessor.)"""
    x, y = H.chain_batch("x"), H.chain_batch("y")
    max_n, bounds = H.CHAIN_CAPACITY, (4096, 65536, 1024)
    bufs = _ChainBufs(cuda, [x, y], max_n)
    first = None
    for step, b in enumerate((x, y, x)):
        tag = f"step {step} of X, Y, X"
        got = _chain_check(b, max_n, _chain_run(cuda, b, max_n, bounds, bufs), bufs, tag, whole=False)
        if step == 0:
            first = got
        if step == 2:
            for g, w, what in zip(got, first, ("count", "match", "cost", "X")):
                _same(g, w, f"{what} of X after Y against X before, {tag}")
    for fill in (0x00, 0xFF):
        for b, name in ((x, "X"), (y, "Y")):
            bufs.ws[:bufs.nws].fill_(fill)
            bufs.resid[:bufs.wsb].fill_(fill)
            tag = f"{name} on workspaces of {fill:#04x}"
            _chain_check(b, max_n, _chain_run(cuda, b, max_n, bounds, bufs), bufs, tag, whole=False)
    for buf, m, what in ((bufs.ws, bufs.nws, "list workspace"), (bufs.resid, bufs.wsb, "resid"),
                         (bufs.ri, bufs.n_out, "row_ind"), (bufs.ci, bufs.n_out, "col_ind"),
                         (bufs.st, bufs.S, "status"), (bufs.k8, bufs.n8, "bmin8"), (bufs.k32, bufs.n32, "bm32"),
                         (bufs.outs[0], bufs.n_out, "match"), (bufs.outs[1], bufs.n_out, "cost"),
                         (bufs.outs[2], bufs.n_out, "X"), (bufs.outs[3], bufs.S, "count")):
        _assert_tail(buf, m, what)
    fresh = _ChainBufs(cuda, [x, y], max_n)
    _chain_check(y, max_n, _chain_run(cuda, y, max_n, bounds, fresh), fresh, "Y on fresh buffers", whole=True)


# ================================================ graph replay on new data ==
def test_graph_replay_on_new_device_data(cuda):
    """Pairwise + cube captured once with capacity bounds (max_n 1025 and 257)
    over fixed device tensors; replayed, then pts, F, cam_offs and the offset
    tables are overwritten in place with a batch of other counts and the graph
    is replayed again (outputs re-filled with the sentinel in between): each
    replay equals the oracle for the data it ran on, whole buffers."""
    g0, g1 = H.graph_batch(0), H.graph_batch(1)
    pairs = H.GRAPH_PAIRS
    pa, pb = [int(v) for v in pairs[:, 0]], [int(v) for v in pairs[:, 1]]
    pS, cS = g0.pS, g0.cube.S
    cap = lambda f: max(f(g0), f(g1))
    zeros = lambda n, dt: torch.zeros(int(n), dtype=dt, device=cuda)
    p_pts = torch.zeros((cap(lambda g: g.p_pts.shape[0]), 2), dtype=torch.float64, device=cuda)
    c_pts = torch.zeros((cap(lambda g: g.cube.pts.shape[0]), 2), dtype=torch.float64, device=cuda)
    p_F, c_F = _t(np.zeros_like(g0.p_F), cuda), _t(np.zeros_like(g0.cube.F), cuda)
    p_co, c_co = zeros(g0.p_co.size, torch.int64), zeros(g0.cube.co.size, torch.int64)
    d_offs, r_offs = zeros(pS * len(pairs), torch.int64), zeros(pS * len(pairs), torch.int64)
    cu_offs, cr_offs = zeros(cS, torch.int64), zeros(cS, torch.int64)
    n_dist, n_rows = cap(lambda g: g.dist.size), cap(lambda g: g.amin.size)
    n_cube, n_crow = cap(lambda g: int(g.cube_offs[-1])), cap(lambda g: int(g.crow_offs[-1]))
    outs = dict(dist=_blank(n_dist + PAD, np.float32, cuda), amin=_blank(n_rows + PAD, np.int32, cuda),
                minv=_blank(n_rows + PAD, np.float32, cuda), cube=_blank(n_cube + PAD, np.float32, cuda),
                camin=_blank(n_crow + PAD, np.int32, cuda), cminv=_blank(n_crow + PAD, np.float32, cuda))
    blanks = {k: v.clone() for k, v in outs.items()}
    ws = _blank(_ws_bytes(cS, H.GRAPH_CUBE_MAX_N), np.uint8, cuda)

    def load(g):
        for dst, src in ((p_pts, g.p_pts), (c_pts, g.cube.pts), (p_F, g.p_F), (c_F, g.cube.F), (p_co, g.p_co),
                         (c_co, g.cube.co), (d_offs, g.dist_offs[:-1]), (r_offs, g.row_offs[:-1]),
                         (cu_offs, g.cube_offs[:-1]), (cr_offs, g.crow_offs[:-1])):
            dst[:src.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(src)))
        for k in outs:
            outs[k].copy_(blanks[k])

    def step():
        torch.ops.mvmatch.pairwise_residual_argmin_out(p_pts, p_co, p_F, pa, pb, pS, 3, H.GRAPH_PAIR_MAX_N, d_offs,
                                                       r_offs, outs["dist"], outs["amin"], outs["minv"], None, 1)
        torch.ops.mvmatch.triplet_cost_argmin_out(c_pts, c_co, c_F, cS, H.GRAPH_CUBE_MAX_N, cu_offs, cr_offs,
                                                  outs["cube"], outs["camin"], outs["cminv"], ws, None)

    def check(g, tag):
        torch.cuda.synchronize(cuda)
        for key, want, n in (("dist", g.dist, n_dist), ("amin", g.amin, n_rows), ("minv", g.minv, n_rows),
                             ("cube", np.concatenate(g.cube.cubes), n_cube),
                             ("camin", np.concatenate(g.cube.amins), n_crow),
                             ("cminv", np.concatenate(g.cube.mins), n_crow)):
            got = _host(outs[key])
            _same(got[:want.size], want, f"{key}, {tag}")
            assert (got[want.size:] == L.sentinel(got.dtype)).all(), f"{key} written past its batch, {tag}"

    load(g0)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        step()                                   # warm-up on the side stream
    torch.cuda.current_stream(cuda).wait_stream(side)
    check(g0, "eager, first batch")
    load(g0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    graph.replay()
    check(g0, "replay, first batch")
    load(g1)
    graph.replay()
    check(g1, "replay, second batch in place")
    load(g0)
    graph.replay()
    check(g0, "replay, first batch again")
