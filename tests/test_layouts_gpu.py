"""Caller-built offset tables, gaps and base pointers at the C ABI.

include/mvmatch.h gives the offset arrays (dist_offs, row_offs, cube_offs,
bmin8_offs, bm32_offs, cost_offs) to the caller: entry s is read on its own.
The plans lay regions back to back in fresh allocations, so the other GPU
tests never see a region at an odd residue, below its predecessor, or with
memory of someone else's behind it.  Here every hot-path op is called
directly with the layouts of tests/layouts.py, into buffers filled with a
sentinel, and the WHOLE buffer is compared with the image the oracle's
values make under that layout: a store one lane too far, or a vector store
chosen for an offset that cannot take it, changes a gap.  Expected values
(oracle/, scipy) are computed once per batch; they do not depend on the layout.
Bit-exact, no tolerance."""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

import layouts as L
from test_cubefree_gpu import _scenes
from test_gpu_parity import ARGMIN_PATHS, CUBE_PATHS, KPL_MAX_VIEW
from test_lsap_bmin8_gpu import _keys
from test_lsap_gpu import LSAP_PATHS

pytestmark = pytest.mark.gpu

TAIL = 4096           # sentinel bytes behind a workspace


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _blank(n, dtype, dev):
    """A device buffer of n elements holding the sentinel of ``dtype``."""
    return _t(L.blank(n, dtype), dev)


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _opts(options):
    from bpc_baseline_amd import ops
    return ops._opts_list(dict(options) if options else None)


def _family_of(i, k):
    """Family of table k in iteration i: over the seven iterations every
    table takes every family, and the tables of one launch differ."""
    return L.FAMILIES[(i + k) % len(L.FAMILIES)]


def _ws_bytes(S, max_n):
    from bpc_baseline_amd import _native
    return int(_native.load().mvm_triplet_workspace_bytes(S, max_n))


def _assert_tail(buf, n, what):
    tail = _host(buf[n:])
    assert (tail == L.sentinel(tail.dtype)).all(), f"{what}: written past its {n} elements"


# ===================================================== cube + bmin8 ========
# one batch per kernel class (the largest view picks the kernel)
CUBE_BATCHES = {
    "small": [(16, 16, 16), (5, 3, 7), (8, 12, 4), (0, 4, 9), (1, 1, 1), (12, 16, 8)],
    "rows8": [(32, 32, 32), (17, 24, 20), (9, 31, 28), (32, 8, 32)],
    "j48": [(48, 40, 48), (33, 35, 36)],
    "rows4": [(64, 64, 64), (40, 33, 52), (7, 64, 12)],
    "rows2": [(20, 100, 96), (6, 97, 128), (11, 66, 100)],
    "rows1": [(6, 130, 256), (4, 200, 132), (3, 9, 255)],
    "chunked": [(3, 20, 260), (2, 5, 512)],
}
# the batch behind the cube-free chain (no kernel class of its own)
CHAIN_COUNTS = [(40, 33, 52), (64, 64, 64), (20, 100, 96), (12, 90, 7)]
ALL_BATCHES = dict(CUBE_BATCHES, chain=CHAIN_COUNTS)


@functools.lru_cache(maxsize=None)
def _cube_expected(batch):
    """The batch's inputs and, per scene, the oracle's cube, argmin, minimum
    and the 8-row minima numpy takes over that cube (read-only)."""
    from oracle import oracle as O
    counts = ALL_BATCHES[batch]
    pts, F, co = _scenes(counts, 31 + len(batch))
    rc, ra, rm, coffs, roffs = O.cube(pts, co, F, len(counts))
    cubes, amins, mins, bm8 = [], [], [], []
    for s, (N, M, P) in enumerate(counts):
        c = rc[coffs[s]:coffs[s + 1]]
        cubes.append(c)
        amins.append(ra[roffs[s]:roffs[s + 1]])
        mins.append(rm[roffs[s]:roffs[s + 1]])
        g8 = (M + 7) // 8
        pad = np.full((N, g8 * 8, P), np.inf, np.float32)
        pad[:, :M] = c.reshape(N, M, P)
        bm8.append(_keys(pad.reshape(N, g8, 8, P).min(axis=2).reshape(-1)) if N * g8 * P
                   else np.zeros(0, np.uint16))
    for a in cubes + amins + mins + bm8:
        a.setflags(write=False)
    return pts, F, co, cubes, amins, mins, bm8


def _cube_cases():
    for batch, counts in CUBE_BATCHES.items():
        big = max(max(c) for c in counts)
        for path in CUBE_PATHS:
            if big <= KPL_MAX_VIEW.get(path, 1 << 30):
                yield batch, path


@pytest.mark.parametrize("batch,path", list(_cube_cases()))
def test_cube_layouts(cuda, batch, path):
    """triplet_cost_argmin_out and triplet_cost_bmin8_out: cube, argmin,
    minimum and 8-row minima whole, under every family of cube_offs, row_offs
    and bmin8_offs (unit 1: the phases reach the scalar key store under a
    4-divisible P and the scalar cube rows under a 4-divisible P)."""
    counts = CUBE_BATCHES[batch]
    pts, F, co, cubes, amins, mins, bm8 = _cube_expected(batch)
    S, max_n = len(counts), max(max(c) for c in counts)
    P_, C_, F_ = _t(pts, cuda), _t(co, cuda), _t(F, cuda)
    opts = _opts(CUBE_PATHS[path])
    wsb = _ws_bytes(S, max_n)
    for i in range(len(L.FAMILIES)):
        lc = L.layout([c.size for c in cubes], _family_of(i, 0), 1, seed=i)
        lr = L.layout([a.size for a in amins], _family_of(i, 3), 1, seed=100 + i)
        lb = L.layout([b.size for b in bm8], _family_of(i, 5), 1, seed=200 + i)
        want = (L.image(lc, np.float32, cubes), L.image(lr, np.int32, amins),
                L.image(lr, np.float32, mins), L.image(lb, np.uint16, bm8))
        offs = [_t(x.offs, cuda) for x in (lc, lr, lb)]
        for with_bm8 in (False, True):
            cube, amin, mn = (_blank(lc.total, np.float32, cuda), _blank(lr.total, np.int32, cuda),
                              _blank(lr.total, np.float32, cuda))
            keys = _blank(lb.total, np.int16, cuda)
            ws = _blank(wsb + TAIL, np.uint8, cuda)
            if with_bm8:
                torch.ops.mvmatch.triplet_cost_bmin8_out(P_, C_, F_, S, max_n, offs[0], offs[1], cube, amin,
                                                         mn, keys, offs[2], ws[:wsb], opts)
            else:
                torch.ops.mvmatch.triplet_cost_argmin_out(P_, C_, F_, S, max_n, offs[0], offs[1], cube,
                                                          amin, mn, ws[:wsb], opts)
            tag = f"{batch}/{path}/{'bmin8' if with_bm8 else 'argmin'} op"
            L.assert_image(_host(cube), want[0], lc, f"cube, {tag}")
            L.assert_image(_host(amin), want[1], lr, f"argmin, {tag}")
            L.assert_image(_host(mn), want[2], lr, f"minval, {tag}")
            L.assert_image(_host(keys, np.uint16), want[3] if with_bm8 else L.blank(lb.total, np.uint16), lb,
                           f"bmin8, {tag}")
            _assert_tail(ws, wsb, f"workspace, {tag}")


# ====================================== cube-free minima and its chain =====
@functools.lru_cache(maxsize=None)
def _minima_expected(batch):
    """... the cube batch's 32-column block minima (rows i >= N 0xFFFF) and
    fp64 pair residuals, from the oracle."""
    from oracle import oracle as O
    counts = ALL_BATCHES[batch]
    pts, F, co, cubes, _, _, bm8 = _cube_expected(batch)
    bm32 = []
    for (N, M, P), c in zip(counts, cubes):
        if N * M * P == 0:
            bm32.append(np.zeros(0, np.uint16))
            continue
        b = np.ascontiguousarray(O.bm32_keys(O.bmin8_keys(c.reshape(N, M, P)), N, M, P).reshape(-1))
        assert b.size == P * ((M + 31) // 32) * ((N + 15) // 16 * 16)
        b.setflags(write=False)
        bm32.append(b)
    resid = O.residuals(pts, co, F, len(counts), max(max(c) for c in counts))
    return bm32, resid


BM32_FAMILIES = ("tight", "gaps", "reversed")


def _run_minima(cuda, batch, i, f8, f32, shift=0):
    """One mvm_triplet_minima launch under layouts (f8, f32) -> the buffers
    (bmin8 behind ``shift`` elements of an aligned allocation)."""
    counts = ALL_BATCHES[batch]
    pts, F, co, _, _, _, bm8 = _cube_expected(batch)
    bm32, _ = _minima_expected(batch)
    S, max_n = len(counts), max(max(c) for c in counts)
    l8 = L.layout([b.size for b in bm8], f8, 1, seed=300 + i)
    l32 = L.layout([b.size for b in bm32], f32, 16, seed=400 + i)
    wsb = _ws_bytes(S, max_n)
    k8 = _blank(shift + l8.total, np.int16, cuda)
    k32 = _blank(max(l32.total, 16), np.int16, cuda)
    resid = _blank(wsb + TAIL, np.uint8, cuda)
    dev = dict(pts=_t(pts, cuda), co=_t(co, cuda), F=_t(F, cuda), o8=_t(l8.offs, cuda), o32=_t(l32.offs, cuda))
    torch.ops.mvmatch.triplet_minima_out(dev["pts"], dev["co"], dev["F"], S, max_n, k8[shift:], dev["o8"], k32,
                                         dev["o32"], resid[:wsb], None)
    return l8, l32, k8, k32, resid, wsb, dev


@pytest.mark.parametrize("batch", ["rows4", "rows2", "rows1"])
def test_minima_layouts(cuda, batch):
    """triplet_minima_out: bmin8 under every family (its stores are scalar, so
    also behind a base shifted off 16 bytes), bm32 under tight / gaps /
    reversed in units of 16 keys; both carry the tight layout's bits, bm32 rows
    i >= N hold 0xFFFF, nothing else is written, and the residuals behind them
    are the oracle's with an untouched tail."""
    counts = CUBE_BATCHES[batch]
    bm8 = _cube_expected(batch)[6]
    bm32, want_r = _minima_expected(batch)
    S, max_n = len(counts), max(max(c) for c in counts)
    ld = (max_n + 3) // 4 * 4
    for i, f8 in enumerate(L.FAMILIES):
        shift = i % 4
        l8, l32, k8, k32, resid, wsb, _ = _run_minima(cuda, batch, i, f8, BM32_FAMILIES[i % 3], shift)
        tag = f"{batch}, bm32 {l32.family}, bmin8 base +{shift}"
        assert (_host(k8[:shift], np.uint16) == L.K16_SENTINEL).all(), f"bmin8 written below its base, {tag}"
        L.assert_image(_host(k8[shift:], np.uint16), L.image(l8, np.uint16, bm8), l8, f"bmin8, {tag}")
        got32 = _host(k32, np.uint16)
        L.assert_image(got32[:l32.total], L.image(l32, np.uint16, bm32), l32, f"bm32, {tag}")
        assert (got32[l32.total:] == L.K16_SENTINEL).all()
        _assert_tail(resid, wsb, f"resid, {tag}")
        got_r = _host(resid[:wsb], np.float64).reshape(S, 3, max_n, ld)
        for s, (N, M, P) in enumerate(counts):
            if N * M * P == 0:
                continue
            for m, (a, b) in enumerate(((N, M), (P, N), (P, M))):
                assert np.array_equal(got_r[s, m, :a, :b].view(np.int64), want_r[s, m, :a, :b].view(np.int64)), \
                    (tag, s, m)


def test_chain_behind_minima_layouts(cuda):
    """lsap_solve_resid_out reading the tables of every layout, then
    select_triangulate_resid_out: assignment and status equal scipy's on the
    oracle cube; matches, order, costs and points equal the tight-layout run
    bit for bit."""
    from bpc_baseline_amd import ops
    counts = CHAIN_COUNTS
    cubes = _cube_expected("chain")[3]
    S, max_n = len(counts), max(max(c) for c in counts)
    c3 = np.asarray(counts, np.int64)
    opts = _opts({"lsap_sparse_min_cols": 1025})          # the existing sparse_lo setting
    lres = ops.LsapPlan(c3[:, 0] * c3[:, 1], c3[:, 2], device=cuda, resid=True)
    segs = _t(c3[:, 1], cuda)
    proj = _t(np.random.default_rng(12).normal(size=(S, 3, 3, 4)), cuda)
    want_rc = [scipy_lsa(c.reshape(N * M, P)) for c, (N, M, P) in zip(cubes, counts)]
    o = lres.out_offs_host
    base = None
    for i, f8 in enumerate(L.FAMILIES):                   # i = 0: tight / tight
        l8, l32, k8, k32, resid, wsb, dev = _run_minima(cuda, "chain", i, f8, BM32_FAMILIES[i % 3])
        ri = _blank(lres.n_out + 64, np.int64, cuda)
        ci = _blank(lres.n_out + 64, np.int64, cuda)
        st = _blank(S + 8, np.int32, cuda)
        ws = _blank(lres.workspace.numel() + TAIL, np.uint8, cuda)
        nws = lres.workspace.numel()
        torch.ops.mvmatch.lsap_solve_resid_out(lres.dims, lres.ws_offs, lres.out_offs, ws[:nws], ri, ci,
                                               st[:S], k8, dev["o8"], k32, dev["o32"], segs, resid[:wsb], max_n,
                                               lres.long_min, lres.long_max, lres.short_max, opts)
        r, c = _host(ri), _host(ci)
        tag = f"bmin8 {f8}, bm32 {l32.family}"
        assert list(_host(st[:S])) == [0] * S, tag
        for s in range(S):
            assert np.array_equal(r[o[s]:o[s + 1]], want_rc[s][0]), (tag, s)
            assert np.array_equal(c[o[s]:o[s + 1]], want_rc[s][1]), (tag, s)
        for b, n, what in ((ri, lres.n_out, "row_ind"), (ci, lres.n_out, "col_ind"), (st, S, "status"),
                           (ws, nws, "lsap workspace")):
            _assert_tail(b, n, f"{what}, {tag}")
        outs = ops._select_outputs(ri[:lres.n_out], lres.out_offs, cuda)
        torch.ops.mvmatch.select_triangulate_resid_out(resid[:wsb], max_n, dev["co"], lres.out_offs,
                                                       ri[:lres.n_out], ci[:lres.n_out], dev["pts"], proj,
                                                       float("inf"), *outs)
        match, cost, X, count = (_host(x) for x in outs)
        rows = np.concatenate([np.arange(o[s], o[s] + count[s]) for s in range(S)])
        got = (count, match[rows], cost[rows].view(np.int32), X[rows].view(np.int64))
        if base is None:
            assert i == 0 and (count == np.minimum(c3[:, 0] * c3[:, 1], c3[:, 2])).all()
            base = got
        for g, w, what in zip(got, base, ("count", "match", "cost", "X")):
            assert np.array_equal(g, w), (what, tag)


# ============================================================ pairwise =====
PAIR_BATCHES = {
    "mid": [(32, 64, 96), (33, 7, 100)],
    "wide_empty": [(256, 128, 260), (1, 255, 0)],
    "tall_thin": [(1024, 4, 36), (31, 1000, 8)],
}
PAIRS = np.array([[a, b] for a in range(3) for b in range(3) if a != b], np.int32)


@functools.lru_cache(maxsize=None)
def _pair_inputs(batch):
    rng = np.random.default_rng(len(batch))
    cnt = np.asarray(PAIR_BATCHES[batch], np.int64)
    co = np.zeros(cnt.size + 1, np.int64)
    np.cumsum(cnt.reshape(-1), out=co[1:])
    pts = np.floor(rng.uniform(0, 4800, size=(int(co[-1]), 2))) / 2
    F = rng.normal(size=(cnt.shape[0] * len(PAIRS), 9))
    na = cnt[:, PAIRS[:, 0]].reshape(-1)
    nb = cnt[:, PAIRS[:, 1]].reshape(-1)
    return pts, F, co, na, nb


@functools.lru_cache(maxsize=None)
def _pair_expected(batch):
    """Per (scene, pair): the oracle's float32 matrix (n_a, n_b), argmin and minimum."""
    from oracle import oracle as O
    pts, F, co, na, nb = _pair_inputs(batch)
    rd, ra, rm, doffs, roffs = O.pairwise(pts, co, F, PAIRS, len(PAIR_BATCHES[batch]), 3)
    mats = [rd[doffs[q]:doffs[q + 1]].reshape(na[q], nb[q]) for q in range(na.size)]
    amins = [ra[roffs[q]:roffs[q + 1]] for q in range(na.size)]
    mins = [rm[roffs[q]:roffs[q + 1]] for q in range(na.size)]
    return mats, amins, mins


def _pitched(mats, row_align):
    """The matrices with rows of roundup(n_b, row_align), padding +inf."""
    out = []
    for m in mats:
        ld = (m.shape[1] + row_align - 1) // row_align * row_align
        p = np.full((m.shape[0], ld), np.inf, np.float32)
        p[:, :m.shape[1]] = m
        out.append(p.reshape(-1))
    return out


@pytest.mark.parametrize("path", sorted(ARGMIN_PATHS))
@pytest.mark.parametrize("batch", sorted(PAIR_BATCHES))
def test_pairwise_layouts(cuda, batch, path):
    """pairwise_residual_argmin_out at row_align 1, 4 and 32: dist_offs of
    every family (the pitch as unit where the family keeps one; the phases and
    offsets = 4 (mod 32) under every pitch), row_offs gapped and reversed.
    Padding columns hold +inf, gaps the sentinel; argmin and minimum whole."""
    pts, F, co, na, nb = _pair_inputs(batch)
    mats, amins, mins = _pair_expected(batch)
    S, max_n = len(PAIR_BATCHES[batch]), int(max(na.max(), nb.max()))
    P_, C_, F_ = _t(pts, cuda), _t(co, cuda), _t(F, cuda)
    options = {k: v for k, v in ARGMIN_PATHS[path].items() if k != "_row_align"}
    opts = _opts(options)
    pa, pb = [int(x) for x in PAIRS[:, 0]], [int(x) for x in PAIRS[:, 1]]
    for row_align in (1, 4, 32):
        regions = _pitched(mats, row_align)
        for i, fam in enumerate(L.FAMILIES):
            unit = row_align if fam in ("tight", "gaps", "reversed") else 1
            ld_ = L.layout([r.size for r in regions], fam, unit, seed=500 + i)
            lr = L.layout([a.size for a in amins], ("gaps", "reversed")[i % 2], 1, seed=600 + i)
            dist, amin, mn = (_blank(ld_.total, np.float32, cuda), _blank(lr.total, np.int32, cuda),
                              _blank(lr.total, np.float32, cuda))
            torch.ops.mvmatch.pairwise_residual_argmin_out(P_, C_, F_, pa, pb, S, 3, max_n, _t(ld_.offs, cuda),
                                                           _t(lr.offs, cuda), dist, amin, mn, opts, row_align)
            tag = f"{batch}/{path}, row_align {row_align}"
            L.assert_image(_host(dist), L.image(ld_, np.float32, regions), ld_, f"dist, {tag}")
            L.assert_image(_host(amin), L.image(lr, np.int32, amins), lr, f"argmin, {tag}")
            L.assert_image(_host(mn), L.image(lr, np.float32, mins), lr, f"minval, {tag}")


@functools.lru_cache(maxsize=None)
def _pair_expected_f64(batch):
    """Per (scene, pair) the oracle's fp64 residuals: the pair as views 0 and 1
    of a three-view scene with an empty third view (oracle.residuals' e12)."""
    from oracle import oracle as O
    pts, F, co, na, nb = _pair_inputs(batch)
    out = []
    for q in range(na.size):
        s, p = divmod(q, len(PAIRS))
        a, b = (int(co[3 * s + c]) for c in PAIRS[p])
        sub = np.concatenate([pts[a:a + na[q]], pts[b:b + nb[q]]])
        sco = np.array([0, na[q], na[q] + nb[q], na[q] + nb[q]], np.int64)
        n = int(max(na[q], nb[q], 1))
        e = O.residuals(sub, sco, np.repeat(F[q:q + 1], 3, axis=0), 1, n)[0, 0, :na[q], :nb[q]].copy()
        e.setflags(write=False)
        out.append(e)
    return out


@pytest.mark.parametrize("batch", sorted(PAIR_BATCHES))
def test_pairwise_f64_strides(cuda, batch):
    """pairwise_residual_f64_out with ld = max columns, + 1, and rounded up
    to 4, and mat_stride = max_rows * ld + 13 (odd: three matrices of four
    start off 16 bytes).  Every defined entry is the oracle's; of a matrix's
    padding, columns n_b .. min(ld, roundup(n_b, 256)) - 1 of rows i < n_a
    hold +inf and nothing else is written (include/mvmatch.h); neither is the
    tail past S * P * mat_stride."""
    pts, F, co, na, nb = _pair_inputs(batch)
    want = _pair_expected_f64(batch)
    S, max_rows, max_cols = len(PAIR_BATCHES[batch]), int(na.max()), int(nb.max())
    max_n = max(max_rows, max_cols)
    P_, C_, F_ = _t(pts, cuda), _t(co, cuda), _t(F, cuda)
    pa, pb = [int(x) for x in PAIRS[:, 0]], [int(x) for x in PAIRS[:, 1]]
    for ld in (max_cols, max_cols + 1, (max_cols + 3) // 4 * 4):
        stride = max_rows * ld + 13
        lay = L.Layout("strided", 1, np.arange(na.size, dtype=np.int64) * stride,
                       np.full(na.size, stride, np.int64), na.size * stride)
        regions = []
        for q in range(na.size):
            r = L.blank(stride, np.float64)
            m = r[:na[q] * ld].reshape(na[q], ld)
            m[:, nb[q]:min(ld, (nb[q] + 255) // 256 * 256)] = np.inf
            m[:, :nb[q]] = want[q]
            regions.append(r)
        e = _blank(lay.total + 64, np.float64, cuda)
        torch.ops.mvmatch.pairwise_residual_f64_out(P_, C_, F_, pa, pb, S, 3, max_n, stride, ld, e)
        L.assert_image(_host(e), L.image(lay, np.float64, regions, tail=64), lay, f"e, {batch}, ld {ld}")


# ========================================================== assignment =====
LSAP_SHAPES = [(3, 5), (40, 9), (9, 40), (64, 16), (300, 20), (24, 600), (1100, 5), (4097, 3)]
COST_FAMILIES = ("gaps", "reversed", "phase1", "phase2", "phase3")


@functools.lru_cache(maxsize=None)
def _lsap_problems(dtype):
    """Every shape as random, half-integer ties, repeated columns and all
    zero, with scipy's assignment of each (in ``dtype``)."""
    rng = np.random.default_rng(21)
    mats = []
    for shape in LSAP_SHAPES:
        for variant in range(4):
            c = rng.normal(size=shape)
            if variant == 1:
                c = np.round(c * 2) / 2
            if variant == 2:
                c[:, :shape[1] // 2] = c[:, :1]
            if variant == 3:
                c = np.zeros(shape)
            c = np.ascontiguousarray(c.astype(dtype))
            c.setflags(write=False)
            mats.append(c)
    return mats, [scipy_lsa(m) for m in mats]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("path", sorted(LSAP_PATHS))
def test_lsap_cost_layouts(cuda, path, dtype):
    """lsap_solve_out with cost_offs gapped, reversed and at every phase (and
    the cost base 0-3 elements off its allocation: the dense kernels load cost
    element by element, the candidate-list ones read the address), ws_offs and
    out_offs the plan's: scipy's assignment, and untouched tails behind
    row_ind, col_ind, status and the workspace."""
    from bpc_baseline_amd import ops
    mats, want = _lsap_problems(dtype)
    n = len(mats)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    plan = ops.LsapPlan([m.shape[0] for m in mats], [m.shape[1] for m in mats], device=cuda, dtype=tdt)
    nws = plan.workspace.numel()
    opts = _opts(LSAP_PATHS[path])
    o = plan.out_offs_host
    for i, fam in enumerate(COST_FAMILIES):
        shift = i % 4
        lay = L.layout([m.size for m in mats], fam, 1, seed=700 + i)
        cost = _t(np.concatenate([L.blank(shift, dtype), L.image(lay, dtype, mats)]), cuda)
        ri, ci = _blank(plan.n_out + 64, np.int64, cuda), _blank(plan.n_out + 64, np.int64, cuda)
        st = _blank(n + 8, np.int32, cuda)
        ws = _blank(nws + TAIL, np.uint8, cuda)
        torch.ops.mvmatch.lsap_solve_out(cost[shift:], _t(lay.offs, cuda), plan.dims, plan.ws_offs,
                                         plan.out_offs, ws[:nws], ri, ci, st[:n], plan.long_min, plan.long_max,
                                         opts, plan.short_max)
        r, c, s = _host(ri), _host(ci), _host(st)
        tag = f"{path}, cost_offs {fam}, base +{shift}"
        assert (s[:n] == 0).all(), (tag, np.flatnonzero(s[:n]))
        for k in range(n):
            assert np.array_equal(r[o[k]:o[k + 1]], want[k][0]) and np.array_equal(c[o[k]:o[k + 1]], want[k][1]), \
                (tag, k, mats[k].shape)
        for b, m, what in ((ri, plan.n_out, "row_ind"), (ci, plan.n_out, "col_ind"), (st, n, "status"),
                           (ws, nws, "workspace")):
            _assert_tail(b, m, f"{what}, {tag}")


def test_sparse_counters_defined_after_a_failed_solve(cuda):
    """The candidate-list solver's four counters are written by every solve
    of a problem of the class (include/mvmatch.h): a problem with a NaN
    (status 1) and an infeasible one (status 2), between two valid ones, leave
    zeros in a workspace that held the sentinel, and the valid problems'
    results stay scipy's."""
    from bpc_baseline_amd import ops
    rng = np.random.default_rng(4)
    mats = [rng.normal(size=(1100, 5)).astype(np.float32) for _ in range(4)]
    mats[1][700, 3] = np.nan
    mats[2][:, 2] = np.inf                                # a short-side column nothing can take
    plan = ops.LsapPlan([1100] * 4, [5] * 4, device=cuda)
    plan.workspace.fill_(L.U8_SENTINEL)
    offs = np.arange(4, dtype=np.int64) * 5500
    r, c, st = ops.linear_sum_assignment_batched(_t(np.concatenate([m.reshape(-1) for m in mats]), cuda),
                                                 _t(offs, cuda), plan,
                                                 options={"lsap_sparse_min_cols": 1025})
    assert list(_host(st)) == [0, 1, 2, 0]
    stats = ops.lsap_sparse_stats(plan, min_cols=1025)
    assert (stats[[1, 2]] == 0).all(), stats
    assert (stats[[0, 3]] >= 0).all() and (stats[[0, 3], 3] > 0).all(), stats
    o = plan.out_offs_host
    for k in (0, 3):
        r0, c0 = scipy_lsa(mats[k])
        assert np.array_equal(_host(r)[o[k]:o[k + 1]], r0) and np.array_equal(_host(c)[o[k]:o[k + 1]], c0)


# ======================================================= base pointers =====
def _raises_untouched(call, outs):
    from bpc_baseline_amd._native import MvmError
    with pytest.raises(MvmError, match="aligned") as err:
        call()
    assert err.value.status == 1                          # MVM_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    for name, t in outs.items():
        h = _host(t)
        assert (h == L.sentinel(h.dtype)).all(), f"{name} written by a refused call"


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_bases_are_refused(cuda, shift):
    """The kernels choose 16-byte cube / dist / e accesses and 8-byte bmin8
    stores from the offsets alone, so the entry points refuse a base off that
    alignment (MVM_ERR_INVALID_ARGUMENT) before any launch: nothing is written."""
    pts, F, co, cubes, amins, _, bm8 = _cube_expected("rows8")
    S, max_n = 4, 32
    P_, C_, F_ = _t(pts, cuda), _t(co, cuda), _t(F, cuda)
    lc, lr, lb = (L.layout([x.size for x in xs], "tight", 4) for xs in (cubes, amins, bm8))
    oc, orow, ob = (_t(x.offs, cuda) for x in (lc, lr, lb))
    wsb = _ws_bytes(S, max_n)

    def bufs():
        return dict(cube=_blank(lc.total + 4, np.float32, cuda), argmin=_blank(lr.total, np.int32, cuda),
                    minval=_blank(lr.total, np.float32, cuda), bmin8=_blank(lb.total + 4, np.int16, cuda),
                    ws=_blank(wsb, np.uint8, cuda))
    b = bufs()
    _raises_untouched(lambda: torch.ops.mvmatch.triplet_cost_argmin_out(
        P_, C_, F_, S, max_n, oc, orow, b["cube"][shift:], b["argmin"], b["minval"], b["ws"], None), b)
    b = bufs()
    _raises_untouched(lambda: torch.ops.mvmatch.triplet_cost_bmin8_out(
        P_, C_, F_, S, max_n, oc, orow, b["cube"][shift:], b["argmin"], b["minval"], b["bmin8"], ob, b["ws"],
        None), b)
    b = bufs()
    _raises_untouched(lambda: torch.ops.mvmatch.triplet_cost_bmin8_out(
        P_, C_, F_, S, max_n, oc, orow, b["cube"], b["argmin"], b["minval"], b["bmin8"][shift:], ob, b["ws"],
        None), b)

    pts, F, co, na, nb = _pair_inputs("mid")
    mats, amins, _ = _pair_expected("mid")
    P_, C_, F_ = _t(pts, cuda), _t(co, cuda), _t(F, cuda)
    pa, pb = [int(x) for x in PAIRS[:, 0]], [int(x) for x in PAIRS[:, 1]]
    ld_ = L.layout([m.size for m in mats], "tight", 4)
    lr = L.layout([a.size for a in amins], "tight")
    b = dict(dist=_blank(ld_.total + 4, np.float32, cuda), argmin=_blank(lr.total, np.int32, cuda),
             minval=_blank(lr.total, np.float32, cuda))
    _raises_untouched(lambda: torch.ops.mvmatch.pairwise_residual_argmin_out(
        P_, C_, F_, pa, pb, 2, 3, 100, _t(ld_.offs, cuda), _t(lr.offs, cuda), b["dist"][shift:], b["argmin"],
        b["minval"], None, 1), b)
    if shift % 2:                                         # doubles: 8 bytes off 16
        e = dict(e=_blank(12 * 100 * 100 + 4, np.float64, cuda))
        _raises_untouched(lambda: torch.ops.mvmatch.pairwise_residual_f64_out(
            P_, C_, F_, pa, pb, 2, 3, 100, 100 * 100, 100, e["e"][shift:]), e)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_scalar_outputs_take_a_shifted_base(cuda, shift):
    """argmin and minval are stored element by element on every path: behind
    a base 1-3 elements off its allocation they hold the same values."""
    pts, F, co, cubes, amins, mins, _ = _cube_expected("rows4")
    S, max_n = len(cubes), 64
    lc, lr = L.layout([c.size for c in cubes], "tight"), L.layout([a.size for a in amins], "gaps", 1, seed=shift)
    cube, amin, mn = (_blank(lc.total, np.float32, cuda), _blank(shift + lr.total, np.int32, cuda),
                      _blank(shift + lr.total, np.float32, cuda))
    ws = _blank(_ws_bytes(S, max_n), np.uint8, cuda)
    torch.ops.mvmatch.triplet_cost_argmin_out(_t(pts, cuda), _t(co, cuda), _t(F, cuda), S, max_n, _t(lc.offs, cuda),
                                              _t(lr.offs, cuda), cube, amin[shift:], mn[shift:], ws, None)
    for got, want, what in ((amin, L.image(lr, np.int32, amins), "argmin"), (mn, L.image(lr, np.float32, mins), "minval")):
        h = _host(got)
        assert (h[:shift] == L.sentinel(h.dtype)).all()
        L.assert_image(h[shift:], want, lr, f"{what}, base +{shift}")


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_extend_matrices_take_a_shifted_base(cuda, shift):
    """mvm_extend_costs tests the address of each matrix before it stores 16
    bytes per lane: E 1-3 floats off its allocation (matrices whose offsets are
    multiples of 4, column counts that are and are not) holds the same bits,
    and nothing is written below the base or behind the matrices."""
    from bpc_baseline_amd import ops
    from test_extend_gpu import SENT, CostBatch, _same_bits
    b = CostBatch(31 + shift, 5, [9, 64, 3], [(12, 8), (64, 4), (260, 5)], True)
    want = np.concatenate([np.full(shift, SENT, np.float32), b.expected(64)])
    out = _t(np.full(want.size, SENT, np.float32), cuda)
    ops.extend_costs(_t(b.pts, cuda), _t(b.cam_offs, cuda), _t(b.F, cuda), _t(b.match, cuda),
                     _t(b.match_offs, cuda), _t(b.rows.astype(np.int32), cuda), _t(b.ext_offs, cuda), b.C,
                     int(b.rows.max()), out=out[shift:])
    _same_bits(_host(out), want)
