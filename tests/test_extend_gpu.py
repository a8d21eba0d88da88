"""The extension of three-view matches into the extra cameras of a 4..8 camera
rig on the GPU: ops.extend_costs and
ops.extend_select_triangulate on their own, then match_captures(n_cams=C)
against the composition of the CPU restatements.

E is checked bit for bit (uint32 views) against
``np.float32(((e0 + e1) + e2) / 3)`` of the oracle's fp64 pair residuals
(oracle.residuals on a three-view arrangement: anchors, view d, nothing); X
against oracle.pipeline.triangulate within the DLT's rtol 1e-10 / atol 1e-9
(DESIGN §3.8)."""
import functools

import numpy as np
import pytest
import torch

from bpc_baseline_amd import ops
from bpc_baseline_amd.inference.batch_match import extension_pairs, match_captures
from bpc_baseline_amd.inference.utils.camera_utils import (fundamental_matrices_batched,
                                                           projection_matrices)
from bpc_baseline_amd.synth import make_capture, make_rig
from oracle import lsap as OL
from oracle import oracle as O
from oracle import pipeline as OP

pytestmark = pytest.mark.gpu

SENT = np.array([0x7FA5A5A5], np.uint32).view(np.float32)[0]    # a NaN no kernel produces
ROWS = (0, 1, 63, 64, 65, 255, 256, 257)
COLS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)
# the kernel keeps 512 columns' lines in LDS: its own tile edge beside the 1025 above
COLS_TILE = (511, 512, 513)
ANCHOR_VIEWS = (5, 6, 7)      # detections of cameras 0, 1, 2 in the hand-built captures
RTOL, ATOL = 1e-10, 1e-9


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _half_px(rng, n):
    return rng.integers(0, 4800, size=(n, 2)).astype(np.float64) / 2


def oracle_E(anchors, q, F3):
    """float32 [n, n_d] of the definition: anchors = three [n, 2] arrays (the
    matches' detections in cameras 0, 1, 2), q [n_d, 2], F3 [3, 9] = F_0d, F_1d,
    F_2d.  The fp64 e_cd come from oracle.residuals as the e12 of a three-view
    scene (anchors of c, view d, an empty view) under (F_cd, 0, 0)."""
    n, nd = anchors[0].shape[0], q.shape[0]
    if n == 0 or nd == 0:
        return np.zeros((n, nd), np.float32)
    pts = np.concatenate([np.concatenate([anchors[c], q]) for c in range(3)])
    co = np.zeros(10, np.int64)
    co[1:] = np.cumsum([n, nd, 0] * 3)
    F = np.zeros((9, 9))
    F[0::3] = F3
    mx = max(n, nd)
    r = O.residuals(pts, co, F, 3, mx)
    e = [r[c, 0, :n, :nd] for c in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        return (((e[0] + e[1]) + e[2]) / 3).astype(np.float32)


def _rig_F(rng, C):
    """(F_ext [C-3, 3, 9], proj [C, 3, 4]) of one make_rig rig."""
    Ks, RTs = make_rig(rng, C)
    Ks, RTs = np.stack(Ks)[None], np.stack(RTs)[None]
    F = fundamental_matrices_batched(Ks, RTs, extension_pairs(C))[3:].reshape(C - 3, 3, 9)
    return F, projection_matrices(Ks, RTs)[0]


class CostBatch:
    """A hand-built batch for ops.extend_costs: capture s has ``rows[s]``
    matches over three anchor views of ANCHOR_VIEWS detections and extra views
    of ``cols[s]`` detections; ``pad``: matrices start on 16-byte boundaries."""

    def __init__(self, seed, C, rows, cols, pad, slack=3):
        rng = np.random.default_rng(seed)
        S, n_ext = len(rows), C - 3
        self.C, self.S, self.rows = C, S, np.asarray(rows, np.int64)
        counts = np.array([list(ANCHOR_VIEWS) + list(cols[s]) for s in range(S)], np.int64)
        self.cam_offs = np.zeros(S * C + 1, np.int64)
        np.cumsum(counts.reshape(-1), out=self.cam_offs[1:])
        self.pts = _half_px(rng, int(self.cam_offs[-1]))
        self.F = np.stack([_rig_F(rng, C)[0] for _ in range(S)]) if S else np.zeros((0, n_ext, 3, 9))
        # match rows: slack rows behind each capture's matches, as the select kernels leave
        self.match_offs = np.zeros(S + 1, np.int64)
        np.cumsum(self.rows + slack, out=self.match_offs[1:])
        self.match = np.full((int(self.match_offs[-1]), 3), -7, np.int32)
        for s in range(S):
            o = self.match_offs[s]
            self.match[o:o + rows[s]] = np.stack([rng.integers(0, v, rows[s]) for v in ANCHOR_VIEWS], 1)
        sizes = (self.rows[:, None] * counts[:, 3:]).reshape(-1)
        if pad:
            sizes = (sizes + 3) // 4 * 4
        self.ext_offs = np.zeros(S * n_ext + 1, np.int64)
        np.cumsum(sizes, out=self.ext_offs[1:])
        self.counts = counts

    def view(self, s, c):
        o = self.cam_offs[s * self.C + c]
        return self.pts[o:o + self.counts[s, c]]

    def anchors(self, s):
        m = self.match[self.match_offs[s]:self.match_offs[s] + self.rows[s]]
        return [self.view(s, c)[m[:, c]] for c in range(3)]

    def expected(self, tail):
        """The whole output buffer: SENT outside the matrices."""
        out = np.full(int(self.ext_offs[-1]) + tail, SENT, np.float32)
        for s in range(self.S):
            a = self.anchors(s)
            for e in range(self.C - 3):
                E = oracle_E(a, self.view(s, 3 + e), self.F[s, e])
                o = self.ext_offs[s * (self.C - 3) + e]
                out[o:o + E.size] = E.reshape(-1)
        return out

    def run(self, dev, tail=64):
        out = torch.full((int(self.ext_offs[-1]) + tail,), float("nan"), dtype=torch.float32, device=dev)
        out.view(torch.int32).fill_(int(SENT.view(np.int32)))
        ops.extend_costs(_t(self.pts, dev), _t(self.cam_offs, dev), _t(self.F, dev), _t(self.match, dev),
                         _t(self.match_offs, dev), _t(self.rows.astype(np.int32), dev),
                         _t(self.ext_offs, dev), self.C, int(self.rows.max()) if self.S else 0, out=out)
        return out.cpu().numpy()


def _same_bits(got, want):
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, f"{bad.size} entries differ, first at {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


@pytest.mark.parametrize("pad", (False, True))
@pytest.mark.parametrize("n", ROWS)
def test_extend_costs_shapes(cuda, n, pad):
    """Every column count under one row count in one launch (a capture each);
    packed back to back (matrices start anywhere) and on 16-byte boundaries."""
    cols = [(c,) for c in COLS + COLS_TILE]
    b = CostBatch(1000 + n, 4, [n] * len(cols), cols, pad)
    _same_bits(b.run(cuda), b.expected(64))


def test_extend_costs_batch_with_an_empty_view_between(cuda):
    """Several captures, two extra cameras (and three) in one launch, an empty
    extra view between non-empty ones, differing match counts."""
    b = CostBatch(7, 5, [9, 0, 70, 3], [(12, 5), (4, 4), (0, 33), (8, 0)], False)
    _same_bits(b.run(cuda), b.expected(64))
    b = CostBatch(8, 6, [5, 130], [(7, 0, 9), (64, 3, 260)], True)
    _same_bits(b.run(cuda), b.expected(64))


def test_extend_costs_nan_centroids(cuda):
    b = CostBatch(11, 5, [40, 6], [(9, 8), (5, 70)], False)
    b.view(0, 1)[:] = np.nan                    # every anchor of camera 1 in capture 0
    b.view(0, 3)[2] = np.nan                    # one detection of view d
    b.view(1, 4)[[0, 69]] = [[np.nan, 3.5], [7.0, np.nan]]
    want = b.expected(64)
    assert np.isnan(want[:40 * 9]).all()
    _same_bits(b.run(cuda), want)


def test_extend_costs_zero_F_is_the_sentinel(cuda):
    b = CostBatch(12, 4, [33], [(37,)], False)
    b.F[:] = 0.0
    got = b.run(cuda)
    assert (got[:33 * 37] == np.float32(9999.0)).all()
    _same_bits(got, b.expected(64))
    # one anchor camera's F only: that residual is the sentinel, the others are not
    b = CostBatch(12, 4, [33], [(37,)], False)
    b.F[0, 0, 1] = 0.0
    _same_bits(b.run(cuda), b.expected(64))


def test_extend_costs_duplicates_tie_columns(cuda):
    b = CostBatch(13, 4, [20], [(24,)], False)
    v = b.view(0, 3)
    v[12:] = v[:12]                             # exact duplicates in view d
    got = b.run(cuda)
    E = got[:20 * 24].reshape(20, 24)
    assert np.array_equal(E[:, 12:].view(np.uint32), E[:, :12].view(np.uint32))
    _same_bits(got, b.expected(64))


def test_extend_costs_rows_bounded_by_count_and_room(cuda):
    """count below max_rows, and a count the matrix has no room for: nothing
    outside [ext_offs[sd], ext_offs[sd + 1]) is written."""
    b = CostBatch(14, 4, [10, 70], [(6,), (9,)], False)
    want = b.expected(64)
    out = torch.empty(want.size, dtype=torch.float32, device=cuda)
    out.view(torch.int32).fill_(int(SENT.view(np.int32)))
    count = np.array([10, 70], np.int32)
    ops.extend_costs(_t(b.pts, cuda), _t(b.cam_offs, cuda), _t(b.F, cuda), _t(b.match, cuda),
                     _t(b.match_offs, cuda), _t(count, cuda), _t(b.ext_offs, cuda), 4, 500, out=out)
    _same_bits(out.cpu().numpy(), want)
    # capture 0 claims 13 matches (its slack rows) but its matrix holds 10 rows
    out.view(torch.int32).fill_(int(SENT.view(np.int32)))
    ops.extend_costs(_t(b.pts, cuda), _t(b.cam_offs, cuda), _t(b.F, cuda), _t(b.match, cuda),
                     _t(b.match_offs, cuda), _t(np.array([13, 70], np.int32), cuda),
                     _t(b.ext_offs, cuda), 4, 70, out=out)
    _same_bits(out.cpu().numpy(), want)


def test_extend_costs_validates(cuda):
    b = CostBatch(15, 4, [4], [(5,)], False)
    a = [_t(b.pts, cuda), _t(b.cam_offs, cuda), _t(b.F, cuda), _t(b.match, cuda), _t(b.match_offs, cuda),
         _t(b.rows.astype(np.int32), cuda), _t(b.ext_offs, cuda)]
    out = torch.zeros(20, dtype=torch.float32, device=cuda)
    for k, bad in ((0, a[0].float()), (3, a[3].long()), (5, a[5].long()), (1, a[1][:-1]), (2, a[2].cpu()),
                   (0, a[0].t())):
        args = list(a)
        args[k] = bad
        with pytest.raises(ValueError):
            ops.extend_costs(*args, 4, 4, out=out)
    with pytest.raises(ValueError):
        ops.extend_costs(*a, 9, 4, out=out)
    with pytest.raises(ValueError):
        ops.extend_costs(*a, 4, 4, out=out.double())


# ------------------------------------------------- select + triangulate ----
class SelBatch:
    """Hand-built input of ops.extend_select_triangulate, no kernel in front:
    capture s has ``ns[s]`` matches of true 3-D points seen by all C cameras
    (views 0-2 permuted), extra views of ``nds[s][e]`` detections, a random
    partial assignment per (s, d) and an E whose assigned entries ``cost(s, e,
    m)`` chooses.  X arrives holding the oracle's three-view triangulation."""

    def __init__(self, seed, C, ns, nds, cost, slack=2):
        rng = np.random.default_rng(seed)
        S, n_ext = len(ns), C - 3
        self.C, self.S, self.ns = C, S, np.asarray(ns, np.int64)
        counts = np.array([[ns[s]] * 3 + list(nds[s]) for s in range(S)], np.int64).reshape(S, C)
        self.counts = counts
        self.cam_offs = np.zeros(S * C + 1, np.int64)
        np.cumsum(counts.reshape(-1), out=self.cam_offs[1:])
        self.pts = _half_px(rng, int(self.cam_offs[-1]))
        self.proj = np.zeros((S, C, 3, 4))
        self.match_offs = np.zeros(S + 1, np.int64)
        np.cumsum(self.ns + slack, out=self.match_offs[1:])
        cap = int(self.match_offs[-1])
        self.match = np.full((cap, 3), -5, np.int32)
        self.X0 = rng.normal(size=(cap, 3))           # slack rows: never touched
        rows = np.repeat(self.ns, n_ext)
        cols = counts[:, 3:].reshape(-1)
        self.ext_offs = np.zeros(S * n_ext + 1, np.int64)
        np.cumsum(rows * cols, out=self.ext_offs[1:])
        self.lsap_offs = np.zeros(S * n_ext + 1, np.int64)
        np.cumsum(np.minimum(rows, cols), out=self.lsap_offs[1:])
        self.E = rng.uniform(0.0, 60.0, int(self.ext_offs[-1])).astype(np.float32)
        self.row_ind = np.zeros(int(self.lsap_offs[-1]), np.int64)
        self.col_ind = np.zeros(int(self.lsap_offs[-1]), np.int64)
        for s in range(S):
            n = int(ns[s])
            Ks, RTs = make_rig(rng, C)
            P = projection_matrices(np.stack(Ks)[None], np.stack(RTs)[None])[0]
            self.proj[s] = P
            Xw = np.stack([rng.uniform(-250, 250, n), rng.uniform(-250, 250, n), rng.uniform(-80, 80, n)], 1)
            uv = np.einsum("cij,nj->cni", P, np.concatenate([Xw, np.ones((n, 1))], 1))
            uv = np.round((uv[..., :2] / uv[..., 2:3] + rng.normal(0, 1.5, (C, n, 2))) * 2) / 2
            mo = self.match_offs[s]
            for c in range(3):
                perm = rng.permutation(n)
                self.match[mo:mo + n, c] = perm
                self.view(s, c)[perm] = uv[c]
            for e in range(n_ext):
                sd, nd = s * n_ext + e, int(counts[s, 3 + e])
                k = min(n, nd)
                r = np.sort(rng.choice(n, k, replace=False))
                l = rng.permutation(nd)[:k]
                lo = self.lsap_offs[sd]
                self.row_ind[lo:lo + k], self.col_ind[lo:lo + k] = r, l
                self.view(s, 3 + e)[l] = uv[3 + e][r]
                Ed = self.E[self.ext_offs[sd]:self.ext_offs[sd + 1]].reshape(n, nd)
                Ed[r, l] = [cost(s, e, m, rng) for m in range(k)]
            if n:
                m = self.match[mo:mo + n]
                p3 = np.stack([self.view(s, c)[m[:, c]] for c in range(3)], 1)
                self.X0[mo:mo + n] = OP.triangulate(np.broadcast_to(P[:3], (n, 3, 3, 4)), p3)

    def view(self, s, c):
        o = self.cam_offs[s * self.C + c]
        return self.pts[o:o + self.counts[s, c]]

    def expected(self, thr):
        """(views, ext_cost, X, kept mask [cap]) by the definition."""
        C, n_ext = self.C, self.C - 3
        cap = self.match.shape[0]
        views = np.full((cap, C), -99, np.int32)
        ext = np.full((cap, n_ext), SENT, np.float32)
        X = self.X0.copy()
        kept = np.zeros(cap, bool)
        for s in range(self.S):
            n, mo = int(self.ns[s]), self.match_offs[s]
            views[mo:mo + n, :3] = self.match[mo:mo + n]
            views[mo:mo + n, 3:] = -1
            ext[mo:mo + n] = np.inf
            for e in range(n_ext):
                sd, nd = s * n_ext + e, int(self.counts[s, 3 + e])
                Ed = self.E[self.ext_offs[sd]:self.ext_offs[sd + 1]].reshape(n, nd)
                lo, hi = self.lsap_offs[sd], self.lsap_offs[sd + 1]
                for r, l in zip(self.row_ind[lo:hi], self.col_ind[lo:hi]):
                    if float(Ed[r, l]) < float(thr):
                        views[mo + r, 3 + e], ext[mo + r, e] = l, Ed[r, l]
            for w in range(n):
                cams = np.nonzero(views[mo + w] >= 0)[0]
                # a seed that is no detection of its view: the X that came in stands
                seeds = all(0 <= views[mo + w, c] < self.counts[s, c] for c in range(3))
                if cams.size > 3 and seeds:
                    kept[mo + w] = True
                    p = np.stack([self.view(s, c)[views[mo + w, c]] for c in cams])
                    X[mo + w] = OP.triangulate(self.proj[s, cams][None], p[None])[0]
        return views, ext, X, kept

    def run(self, dev, thr):
        cap = self.match.shape[0]
        views = torch.full((cap, self.C), -99, dtype=torch.int32, device=dev)
        ext = torch.empty((cap, self.C - 3), dtype=torch.float32, device=dev)
        ext.view(torch.int32).fill_(int(SENT.view(np.int32)))
        X = _t(self.X0, dev)
        t = lambda a: _t(a, dev)
        ops.extend_select_triangulate(t(self.E), t(self.ext_offs), t(self.lsap_offs), t(self.row_ind),
                                      t(self.col_ind), t(self.match), t(self.match_offs),
                                      t(self.ns.astype(np.int32)), t(self.pts), t(self.cam_offs),
                                      t(self.proj), thr, X, self.C, out=(views, ext))
        return views.cpu().numpy(), ext.cpu().numpy(), X.cpu().numpy()

    def check(self, dev, thr):
        views, ext, X = self.run(dev, thr)
        w_views, w_ext, w_X, kept = self.expected(thr)
        assert np.array_equal(views, w_views)
        _same_bits(ext.reshape(-1), w_ext.reshape(-1))
        # no kept view (and the slack rows): the X that came in, bit for bit
        assert np.array_equal(X[~kept].view(np.uint64), self.X0[~kept].view(np.uint64))
        np.testing.assert_allclose(X[kept], w_X[kept], rtol=RTOL, atol=ATOL)
        return w_views, kept


def _around(thr):
    t = np.float32(thr)
    return [np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf))]


@pytest.mark.parametrize("thr", (30, 0.7))
def test_extend_select_threshold_edges(cuda, thr):
    """Costs at and one float32 ulp either side of the threshold; the compare
    is float64 (float32(0.7) < 0.7 is kept, float32(30) < 30 is not)."""
    vals = _around(thr)
    b = SelBatch(21, 5, [9, 4], [(9, 12), (6, 2)], lambda s, e, m, rng: vals[m % 3])
    views, _ = b.check(cuda, thr)
    kept_vals = {float(v) for v in vals if float(v) < float(thr)}
    assert len(kept_vals) == (2 if thr == 0.7 else 1)
    assert (views[:9, 3] >= 0).sum() == 3 * len(kept_vals)


@pytest.mark.parametrize("thr", (float("inf"), 0.0, float("nan")))
def test_extend_select_special_thresholds(cuda, thr):
    vals = [np.float32(0.0), np.float32(5.0), np.float32(np.inf), np.float32(3e38)]
    b = SelBatch(22, 4, [8, 3], [(10,), (3,)], lambda s, e, m, rng: vals[m % 4])
    views, kept = b.check(cuda, thr)
    if thr == float("inf"):
        assert kept.sum() == 6 + 2               # every finite assigned cost (m % 4 != 2)
    else:
        assert not kept.any()


def test_extend_select_every_view_count(cuda):
    """C = 8: match w keeps w % 6 of its five extra views, so V = 3 .. 8 all occur."""
    n = 24

    def cost(s, e, m, rng):
        return np.float32(1.0 if e < m % 6 else 50.0)
    b = SelBatch(23, 8, [n], [(n,) * 5], cost)
    # all rows assigned in every camera, in row order: m == w
    views, kept = b.check(cuda, 30.0)
    nv = (views[:n] >= 0).sum(axis=1)
    assert sorted(set(nv.tolist())) == [3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("C", (4, 6))
def test_extend_select_counts(cuda, C):
    """Captures of 0, 1, 255, 256 and 257 matches (one, two and three sweeps of
    a workgroup), extra views smaller and larger than the match count."""
    ns = [0, 1, 255, 256, 257]
    nds = [(3, 0, 5), (2, 1, 0), (200, 255, 300), (256, 0, 257), (300, 257, 1)]
    b = SelBatch(24 + C, C, ns, [d[:C - 3] for d in nds],
                 lambda s, e, m, rng: np.float32(rng.uniform(0, 60)))
    views, kept = b.check(cuda, 30.0)
    assert kept.any() and not kept.all()


def test_extend_select_ignores_pairs_that_are_no_indices(cuda):
    """What a failed assignment leaves behind is unspecified: out-of-range
    pairs are skipped, never used as an index."""
    b = SelBatch(29, 4, [6], [(8,)], lambda s, e, m, rng: np.float32(1.0))
    b.row_ind[:3] = [-1, 6, 2 ** 40]
    b.col_ind[3] = 8
    views, ext, X = b.run(cuda, 30.0)
    assert (views[:6, 3] >= 0).sum() == 2


def test_extend_select_seed_that_is_no_detection_of_its_view(cuda):
    """One capture, C = 4, views of (3, 3, 3, 2) detections, three matches:
    row 1's seed in view 1 is 3 (the view's size), row 2's seed in view 0 is
    -1.  Every row is assigned an extra view under the threshold -- the
    two-detection view 3 holds two pairs a launch, so row 0 goes with row 1 in
    one launch and with row 2 in the next.  views and ext_cost are set as for
    any row; the X of rows 1 and 2 keeps the bits it came with (distinct finite
    sentinels) and row 0's is the four-view DLT."""
    b = SelBatch(31, 4, [3], [(2,)], lambda s, e, m, rng: np.float32(1.0))
    assert b.counts.tolist() == [[3, 3, 3, 2]]
    # row 0's detection in view 3: its three-view point seen by camera 3
    h = b.proj[0, 3] @ np.append(b.X0[0], 1.0)
    b.view(0, 3)[0] = np.round(h[:2] / h[2] * 2) / 2
    b.E[:] = np.float32(1.0)
    b.match[1, 1] = 3
    b.match[2, 0] = -1
    sent = np.arange(1.0, 1.0 + b.X0.size).reshape(b.X0.shape) * 1.25
    b.X0[:] = sent
    for bad in (1, 2):
        b.row_ind[:], b.col_ind[:] = [0, bad], [0, 1]
        views, kept = b.check(cuda, 30.0)
        assert kept.tolist() == [True, False, False, False, False]
        assert views[:3, 3].tolist() == [[0, 1, -1], [0, -1, 1]][bad - 1]
        assert np.array_equal(views[:3, :3], b.match[:3])
        X = b.run(cuda, 30.0)[2]
        assert np.array_equal(X[1:].view(np.uint64), sent[1:].view(np.uint64))
        assert np.isfinite(X[0]).all() and not np.array_equal(X[0], sent[0])


# ----------------------------------------------------------- end to end ----
class Rig:
    pass


@functools.lru_cache(maxsize=None)
def fixture(C):
    """8 captures of C cameras from make_capture, 8-24 detections per view;
    extra views get clutter added or detections dropped (n_d > n and n_d < n
    both occur), capture 2 has an empty extra view, capture 5 no match at all
    (its camera 2 saw nothing)."""
    S = 8
    rng = np.random.default_rng(500 + C)
    f = Rig()
    f.S, f.C = S, C
    f.Ks, f.RTs = np.zeros((S, C, 3, 3), np.float32), np.zeros((S, C, 4, 4))
    boxes, counts = [], []
    for s in range(S):
        n = [int(x) for x in rng.integers(8, 25, C)]
        Ks, RTs, det = make_capture(rng, C, n)
        f.Ks[s], f.RTs[s] = np.stack(Ks), np.stack(RTs)
        for c in range(C):
            b = np.array([d["bbox"] for d in det[c]], np.float64).reshape(-1, 4)
            if c >= 3 and (s + c) % 2:          # clutter added
                k = int(rng.integers(6, 16))
                ctr, half = rng.uniform(100, 2300, (k, 2)), rng.uniform(20, 60, (k, 2))
                b = np.concatenate([b, np.trunc(np.concatenate([ctr - half, ctr + half], 1))])
            elif c >= 3:                        # detections dropped
                b = b[rng.random(len(b)) < 0.5]
            if (s == 2 and c == C - 1) or (s == 5 and c == 2):
                b = b[:0]
            boxes.append(b)
            counts.append(len(b))
    f.boxes = np.concatenate(boxes).astype(np.float32)
    f.conf = np.full(len(f.boxes), 0.9, np.float32)
    f.cls = np.zeros(len(f.boxes), np.float32)
    f.img_offs = np.zeros(S * C + 1, np.int64)
    np.cumsum(counts, out=f.img_offs[1:])
    f.counts = np.asarray(counts).reshape(S, C)
    f.cent = 0.5 * (f.boxes[:, :2].astype(np.float64) + f.boxes[:, 2:].astype(np.float64))
    return f


def three_cam_inputs(f):
    """The first three cameras of every capture as a batch of their own."""
    rows = np.concatenate([np.arange(f.img_offs[f.C * s], f.img_offs[f.C * s + 3]) for s in range(f.S)])
    offs = np.zeros(3 * f.S + 1, np.int64)
    np.cumsum(f.counts[:, :3].reshape(-1), out=offs[1:])
    return f.boxes[rows], f.conf[rows], f.cls[rows], offs, f.Ks[:, :3].copy(), f.RTs[:, :3].copy()


def compose(f, F, thr=30.0):
    """The definition by the CPU restatements, per capture: (matches int [n, 3]
    in _match's order, views [n, C], ext_cost [n, C-3], X [n, 3]).  F [S, P, 9]."""
    out = []
    P = projection_matrices(f.Ks, f.RTs)
    for s in range(f.S):
        co = f.img_offs[f.C * s:f.C * s + f.C + 1]
        view = lambda c: f.cent[co[c]:co[c + 1]]
        n3 = f.counts[s, :3]
        co3 = np.concatenate([[0], np.cumsum(n3)])
        cube = O.cube(f.cent[co[0]:co[3]], co3, F[s, :3], 1)[0].reshape(n3)
        m = np.asarray(sorted(OL.match_objects(cube, thr), key=lambda t: cube[t]), np.int64).reshape(-1, 3)
        n = len(m)
        views = np.full((n, f.C), -1, np.int32)
        views[:, :3] = m
        ext = np.full((n, f.C - 3), np.inf, np.float32)
        anchors = [view(c)[m[:, c]] for c in range(3)]
        for d in range(3, f.C):
            E = oracle_E(anchors, view(d), F[s, 3 + 3 * (d - 3):6 + 3 * (d - 3)])
            r, l = OL.linear_sum_assignment(E)
            for w, q in zip(r, l):
                if float(E[w, q]) < thr:
                    views[w, d], ext[w, d - 3] = q, E[w, q]
        X = np.zeros((n, 3))
        for w in range(n):
            cams = np.nonzero(views[w] >= 0)[0]
            p = np.stack([view(c)[views[w, c]] for c in cams])
            X[w] = OP.triangulate(P[s, cams][None], p[None])[0]
        out.append((m, views, ext, X))
    return out


def assert_fixture_is_not_empty(f, comp):
    """By the oracle composition alone: a quarter of all matches keep an extra
    view, one at least keeps none, n_d < n and n_d > n both occur, one capture
    has an empty extra view and one no match."""
    views = np.concatenate([c[1] for c in comp])
    kept = (views[:, 3:] >= 0).any(axis=1)
    assert len(views) >= 16 and kept.sum() * 4 >= len(views) and (~kept).any()
    n = np.array([len(c[0]) for c in comp])
    assert (n == 0).any()
    assert ((f.counts[:, 3:] < n[:, None]) & (n[:, None] > 0)).any()
    assert ((f.counts[:, 3:] > n[:, None]) & (n[:, None] > 0)).any()
    assert ((f.counts[:, 3:] == 0) & (n[:, None] > 0)).any()


@pytest.mark.parametrize("rig", ("host", "device"))
@pytest.mark.parametrize("C", (4, 5))
def test_match_captures_extends_into_the_extra_cameras(cuda, C, rig):
    f = fixture(C)
    pairs = extension_pairs(C)
    if rig == "host":
        F = fundamental_matrices_batched(f.Ks, f.RTs, pairs)
    else:       # the composition under the F the device computed
        F = ops.rig_matrices(f.Ks, f.RTs, pairs=pairs, want_proj=False, device=cuda)[0].cpu().numpy()
    comp = compose(f, F.reshape(f.S, len(pairs), 9))
    assert_fixture_is_not_empty(f, comp)

    t = lambda a: _t(a, cuda)
    res = match_captures(t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs, rig=rig, n_cams=C)
    b3 = three_cam_inputs(f)
    ref = match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5], rig=rig)
    assert res.n_cams == C and res.views.shape[1] == C and res.ext_cost.shape[1] == C - 3
    assert np.array_equal(res.count, ref.count) and np.array_equal(res.offs, ref.offs)
    h = {k: getattr(res, k).cpu().numpy() for k in ("match", "cost", "X", "views", "ext_cost")}
    r = {k: getattr(ref, k).cpu().numpy() for k in ("match", "cost", "X")}
    for s in range(f.S):
        o, n = int(res.offs[s]), int(res.count[s])
        m, views, ext, X = comp[s]
        sl = slice(o, o + n)
        assert n == len(m)
        # the three-camera chain, unchanged: matches, costs, order
        assert np.array_equal(h["match"][sl], r["match"][sl]) and np.array_equal(h["match"][sl], m)
        assert np.array_equal(h["cost"][sl].view(np.uint32), r["cost"][sl].view(np.uint32))
        assert np.array_equal(h["views"][sl], views), s
        _same_bits(h["ext_cost"][sl].reshape(-1), ext.reshape(-1))
        none = (views[:, 3:] < 0).all(axis=1)
        assert np.array_equal(h["X"][sl][none].view(np.uint64), r["X"][sl][none].view(np.uint64))
        np.testing.assert_allclose(h["X"][sl], X, rtol=RTOL, atol=ATOL)
        pred = res.predictions(s)
        assert len(pred) == n
        for w, (pb, pc, pt, cams) in enumerate(pred):
            assert np.array_equal(cams, np.nonzero(views[w] >= 0)[0])
            assert pb.shape == (len(cams), 4) and np.array_equal(pt, h["X"][o + w])
            co = f.img_offs[C * s:]
            assert np.array_equal(pc, np.stack([f.cent[co[c] + views[w, c]] for c in cams]))
    with pytest.raises(NotImplementedError):
        res.table()


def test_n_cams_3_is_the_call_without_the_keyword(cuda):
    f = fixture(4)
    b3 = three_cam_inputs(f)
    t = lambda a: _t(a, cuda)
    a = match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5])
    b = match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5], n_cams=3)
    assert b.n_cams == 3 and b.views is None and b.ext_cost is None and a.views is None
    assert np.array_equal(a.count, b.count) and np.array_equal(a.offs, b.offs)
    assert np.array_equal(a.cam_offs, b.cam_offs)
    for s in range(f.S):
        sl = slice(int(a.offs[s]), int(a.offs[s]) + int(a.count[s]))
        for k in ("match", "cost", "X"):
            assert torch.equal(getattr(a, k)[sl], getattr(b, k)[sl]), k
    for k in ("pts", "boxes"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    ta, tb = a.table().host(), b.table().host()
    assert all(np.array_equal(ta[k], tb[k]) for k in ta)


def test_stream_passes_n_cams_through(cuda):
    from bpc_baseline_amd.inference.batch_match import match_capture_stream
    f = fixture(4)
    t = lambda a: _t(a, cuda)
    batch = (t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs)
    one = match_captures(*batch, n_cams=4)
    got = list(match_capture_stream([batch, batch], n_cams=4))
    assert len(got) == 2
    for g in got:
        assert g.n_cams == 4 and np.array_equal(g.count, one.count)
        for s in range(f.S):
            sl = slice(int(one.offs[s]), int(one.offs[s]) + int(one.count[s]))
            assert torch.equal(g.views[sl], one.views[sl]) and torch.equal(g.X[sl], one.X[sl])
