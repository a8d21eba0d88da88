"""Poses against ground truth on the GPU (mvm_score_poses, mvm_match_scores,
ops_views.score_poses / match_scores) against
tests/score_model.py.

The ops write into slices of sentinel-filled outputs with a guard row on either
side; every output is compared whole and bit for bit with the model (NaN equal
to NaN), the guards with the sentinel, and the inputs with what was uploaded."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import score_model as M
from bpc_baseline_amd import ops_views       # registers torch.ops.mvmatch_views.*
from test_crop_gpu import _graph_shape

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -777.0, -12345
BIG = 2.0 ** 200
BELOW = float(np.nextafter(BIG, 0.0))
OUTS = (("err", torch.float64), ("sym", torch.int32), ("t_err", torch.float64), ("rot_cos", torch.float64))


class Case:
    """n estimates over S captures whose ground-truth counts are ragged (the
    first holds Gmax, one holds none where S > 1), V vertices up to 1e3 and K
    turns about z with translations (two of them equal where K >= 7).  Some
    estimates are their capture's first object exactly.  Where n >= 9 the last
    rows hold a scene id on either side of the captures and estimates with a
    NaN, an infinity, +-2^200 and the float64 below it; the ground truth holds
    the same where it has the rows."""

    def __init__(self, n, S, Gmax, V, K, scene_base=0, seed=0):
        rng = np.random.default_rng(100000 * n + 1000 * Gmax + 10 * V + K + S + seed)
        self.n, self.S, self.Gmax, self.V, self.K, self.scene_base = n, S, Gmax, V, K, scene_base
        counts = rng.integers(0, Gmax + 1, S)
        counts[0] = Gmax
        if S > 1:
            counts[S - 1] = 0
        self.gt_offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        G = int(self.gt_offs[-1])
        self.gt_pose = M.random_poses(rng, G)
        self.pose = M.random_poses(rng, n)
        self.scene = (np.arange(n) % S + scene_base).astype(np.int32)
        for r in range(0, n, 3):                                     # the capture's first object, exactly
            s = r % S
            if counts[s]:
                self.pose[r] = self.gt_pose[self.gt_offs[s]]
        if n and G:
            self.pose[0, 3] = self.gt_pose[0, 3] = np.nan            # the bottom row is never read
        if G >= 4:
            self.gt_pose[1, 0, 1] = np.nan
            self.gt_pose[2, 2, 3] = -BIG
            self.gt_pose[3, 1, 2] = BELOW
        if n >= 9:
            self.scene[n - 1], self.scene[n - 2] = scene_base - 1, scene_base + S
            self.pose[n - 3, 0, 0] = np.nan
            self.pose[n - 4, 1, 3] = np.inf
            self.pose[n - 5, 2, 1] = BIG
            self.pose[n - 6, 0, 3] = -BIG
            self.pose[n - 7, 1, 1] = -BELOW
        self.verts = rng.uniform(-1e3, 1e3, (V, 3))
        self.syms = M.z_symmetries(K)
        self.syms[1:, :3, 3] = rng.uniform(-1e3, 1e3, (K - 1, 3))
        if K >= 7:
            self.syms[5] = self.syms[3]

    def device(self, dev):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t(self.pose), t(self.scene), t(self.gt_pose), t(self.gt_offs), t(self.verts), t(self.syms)

    @lru_cache(maxsize=None)
    def expected(self, rows=None):
        return M.score_poses(self.pose, self.scene, self.gt_pose, self.gt_offs, self.verts, self.syms, rows=rows,
                             scene_base=self.scene_base)


@lru_cache(maxsize=None)
def case(*a, **kw):
    return Case(*a, **kw)


def _unchanged(got, was):
    return bool(((got == was) | ((got != got) & (was != was))).all())


def run_score(c, dev, rows=None, omit=()):
    """The op on a fresh upload -> dict of the outputs on the host, after
    checking the guards and that no input changed."""
    b, e = (0, c.n) if rows is None else rows
    m = e - b
    args = c.device(dev)
    if args[2].numel() == 0:                          # the op wants a pose to point at
        args = args[:2] + (torch.zeros((1, 4, 4), dtype=torch.float64, device=dev),) + args[3:]
    keep = [a.clone() for a in args]
    bufs = {k: torch.full((m + 2, c.Gmax), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=dev)
            for k, dt in OUTS}
    out = {k: (None if k in omit else v[1:m + 1]) for k, v in bufs.items()}
    torch.ops.mvmatch_views.score_poses_out(*args, c.scene_base, c.Gmax, b, m, out["err"], out["sym"], out["t_err"],
                                            out["rot_cos"])
    torch.cuda.synchronize(dev)
    assert all(_unchanged(got, was) for got, was in zip(args, keep))
    for k, dt in OUTS:
        sent = SENT_I if dt == torch.int32 else SENT_F
        assert (bufs[k][0] == sent).all() and (bufs[k][-1] == sent).all(), k
        if k in omit:
            assert (bufs[k] == sent).all(), k
    return {k: v[1:m + 1].cpu().numpy() for k, v in bufs.items() if k not in omit}


def check(c, dev, rows=None, omit=()):
    got, want = run_score(c, dev, rows, omit), c.expected(rows)
    for k, v in got.items():
        assert M.same(v, want[k]), (k, np.argwhere(~((v == want[k]) | ((v != v) & (want[k] != want[k]))))[:5])
    return want


# 3, 4, 5 and 8: both sides of the vertex loop's unrolled step of four
@pytest.mark.parametrize("V", (1, 3, 4, 5, 8, 63, 64, 65, 255, 256, 257, 1025))
def test_vertex_counts(cuda, V):
    want = check(case(9, 2, 2, V, 2), cuda)
    assert np.isfinite(want["err"]).any()


@pytest.mark.parametrize("K", (1, 2, 7, 64))
def test_symmetry_counts(cuda, K):
    want = check(case(40, 2, 3, 5, K), cuda)
    assert len(set(want["sym"][want["sym"] >= 0])) >= min(K, 3)
    if K >= 7:
        assert not (want["sym"] == 5).any()                           # symmetry 3 again: the lower index keeps the tie


@pytest.mark.parametrize("S", (1, 5))
@pytest.mark.parametrize("Gmax", (1, 2, 63, 64, 65, 130))
def test_ground_truth_widths(cuda, Gmax, S):
    c = case(11, S, Gmax, 3, 2)
    want = check(c, cuda)
    assert want["err"].shape == (11, Gmax)
    if S > 1:
        assert (want["sym"] == M.PADDING).any() and (want["sym"] == M.NO_CAPTURE).any()
    if Gmax >= 4:
        assert (want["sym"] == M.NOT_FINITE).any()


@pytest.mark.parametrize("S", (1, 5))
@pytest.mark.parametrize("n", (0, 1, 257))
def test_row_counts(cuda, n, S):
    want = check(case(n, S, 5, 5, 2), cuda)
    if n == 257:
        # every rule and every special value of the class is met, and equal poses give exactly 0
        assert {M.NO_CAPTURE, M.NOT_FINITE, 0, 1} <= set(want["sym"].reshape(-1))
        assert (want["sym"] == M.PADDING).any() == (S > 1)
        assert (want["err"] == 0.0).any() and np.isfinite(want["err"][n - 7]).any()
        assert (want["sym"][[n - 3, n - 4, n - 5, n - 6]] < 0).all()
        assert want["sym"][0, 0] == 0 and want["err"][0, 0] == 0.0     # a NaN in the bottom row is not read
        assert (want["sym"][[n - 1, n - 2]] == M.NO_CAPTURE).all()


def test_scene_base_with_ids_outside_on_either_side(cuda):
    c = case(257, 5, 4, 5, 2, scene_base=7)
    want = check(c, cuda)
    assert (want["sym"][[c.n - 1, c.n - 2]] == M.NO_CAPTURE).all() and (want["sym"][:5, 0] >= 0).any()


def test_no_ground_truth_at_all(cuda):
    c = Case(5, 1, 1, 2, 1)
    c.gt_offs, c.gt_pose = np.zeros(2, np.int64), np.zeros((0, 4, 4))
    want = check(c, cuda)
    assert (want["sym"] == M.PADDING).all() and want["sym"].shape == (5, 1)


@pytest.mark.parametrize("rows", ((0, 0), (0, 1), (100, 180), (-1, None)))
def test_row_ranges(cuda, rows):
    c = case(257, 5, 5, 5, 2)
    rows = (c.n - 1, c.n) if rows[1] is None else rows
    check(c, cuda, rows)


@pytest.mark.parametrize("omit", (("t_err",), ("rot_cos",), ("t_err", "rot_cos")))
def test_optional_outputs(cuda, omit):
    check(case(257, 5, 5, 5, 2), cuda, omit=omit)
    check(case(257, 5, 5, 5, 2), cuda, rows=(3, 40), omit=omit)


# ------------------------------------------------------------- matching ----
class MatchCase:
    """S captures of 0..max_rows rows (the first and the last hold some), a row
    before and two behind them that no capture owns, ragged ground-truth counts
    up to Gmax (one above it where S > 2: cut to the columns), errors with many
    ties, infinities and a few NaNs."""

    def __init__(self, S, Gmax, max_rows=12, seed=0):
        rng = np.random.default_rng(1000 * S + Gmax + seed)
        rows = rng.integers(0, max_rows + 1, S)
        rows[0] = rows[-1] = max_rows
        if S > 2:
            rows[1] = 0
        counts = rng.integers(0, Gmax + 1, S)
        counts[0] = Gmax
        if S > 2:
            counts[2], counts[S - 1] = Gmax + 3, 0
        self.row_offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64) + 1
        self.gt_offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.n, self.S, self.Gmax = int(self.row_offs[-1]) + 2, S, Gmax
        self.err = rng.integers(0, max(4, Gmax // 2), (self.n, Gmax)).astype(np.float64) * 0.37
        self.err[rng.random(self.err.shape) < 0.1] = np.inf
        self.err[rng.random(self.err.shape) < 0.02] = np.nan


def run_match(c, dev, thresholds):
    T = len(thresholds)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(c.err), t(c.row_offs), t(c.gt_offs))
    keep = [a.clone() for a in args]
    gi = torch.full((T + 2, c.n), SENT_I, dtype=torch.int32, device=dev)
    tp = torch.full((T + 2, c.S), SENT_I, dtype=torch.int32, device=dev)
    torch.ops.mvmatch_views.match_scores_out(*args, [float(v) for v in thresholds], gi[1:T + 1], tp[1:T + 1])
    torch.cuda.synchronize(dev)
    assert all(_unchanged(got, was) for got, was in zip(args, keep))
    for buf in (gi, tp):
        assert (buf[0] == SENT_I).all() and (buf[-1] == SENT_I).all()
    return gi[1:T + 1].cpu().numpy(), tp[1:T + 1].cpu().numpy()


def check_match(c, dev, thresholds):
    got, want = run_match(c, dev, thresholds), M.match_scores(c.err, c.row_offs, c.gt_offs, thresholds)
    assert M.same(got[0], want[0]) and M.same(got[1], want[1])
    return want


@pytest.mark.parametrize("S", (1, 5))
@pytest.mark.parametrize("Gmax", (1, 2, 63, 64, 65, 130, 1024))
def test_match_widths_and_thresholds(cuda, Gmax, S):
    c = MatchCase(S, Gmax)
    vals = np.unique(c.err[np.isfinite(c.err)])
    an_err = float(vals[len(vals) // 2])                              # one of the errors, bit for bit
    gi, tp = check_match(c, cuda, [an_err])                           # T = 1
    assert (gi[0, [0, -1, -2]] == -1).all()
    sixteen = [0.0, np.inf, an_err, np.nextafter(an_err, np.inf)] + list(np.linspace(0.1, 4.0, 12))
    gi, tp = check_match(c, cuda, sixteen)                            # T = 16
    assert not tp[0].any() and (gi[0] == -1).all()                    # nothing is below 0
    assert tp[1].sum() > 0 and (tp <= np.diff(c.row_offs)[None, :]).all()
    if Gmax >= 130:
        assert gi.max() >= 64                                         # a column of a later chunk is taken


def test_match_of_no_rows_and_of_no_captures(cuda):
    c = MatchCase(3, 4)
    c.err, c.n, c.row_offs = c.err[:0], 0, np.zeros(4, np.int64)
    gi, tp = check_match(c, cuda, [1.0, 2.0])
    assert gi.shape == (2, 0) and not tp.any()
    c = MatchCase(1, 4)
    c.row_offs, c.gt_offs, c.S = np.zeros(1, np.int64), np.zeros(1, np.int64), 0
    gi, tp = check_match(c, cuda, [1.0, 2.0])
    assert (gi == -1).all() and gi.shape == (2, c.n) and tp.shape == (2, 0)


def test_scores_feed_the_matching(cuda):
    """score_poses -> match_scores through the wrappers on a table sorted by
    capture, with a threshold equal to one of the errors bit for bit."""
    c = Case(60, 5, 6, 9, 2)
    c.pose[0] = c.pose[1]                             # the first row: no copy of an object
    c.scene = np.sort(c.scene[:52]).astype(np.int32)
    c.scene = np.concatenate([c.scene, np.full(8, 4, np.int32)]).astype(np.int32)   # the special poses, capture 4: no object
    row_offs = np.searchsorted(c.scene, np.arange(6)).astype(np.int64)
    want = M.score_poses(c.pose, c.scene, c.gt_pose, c.gt_offs, c.verts, c.syms)
    pose, scene = torch.from_numpy(c.pose).to(cuda), torch.from_numpy(c.scene).to(cuda)
    res = ops_views.score_poses(pose, scene, c.gt_pose, c.gt_offs, c.verts, c.syms)
    for k in M.KEYS:
        assert M.same(getattr(res, k).cpu().numpy(), want[k]), k
    best = int(np.argmin(want["err"][0]))
    mid = float(want["err"][0, best])                 # the first row's smallest error, bit for bit
    assert 0.0 < mid < np.inf
    thresholds = [mid, 0.0, np.inf, float(np.nextafter(mid, np.inf))]
    gi, tp = ops_views.match_scores(res.err, row_offs, c.gt_offs, thresholds)
    wi, wt = M.match_scores(want["err"], row_offs, c.gt_offs, thresholds)
    assert M.same(gi.cpu().numpy(), wi) and M.same(tp.cpu().numpy(), wt)
    assert not wt[1].any() and wt[2].sum() > 0 and wi[0][0] == -1 and wi[3][0] == best
    r, p = ops_views.recall_precision(tp, row_offs, c.gt_offs)
    wr, wp = M.recall_precision(wt, row_offs, c.gt_offs)
    assert r.device == tp.device and np.allclose(r.cpu().numpy(), wr, rtol=1e-15) \
        and np.allclose(p.cpu().numpy(), wp, rtol=1e-15)


# --------------------------------------------------------------- graphs ----
def test_score_op_captures_into_a_graph(cuda):
    """One kernel node and no edge; the replay gives the eager bytes."""
    c = case(257, 5, 5, 5, 2)
    eager = run_score(c, cuda)
    args = c.device(cuda)
    out = {k: torch.full((c.n, c.Gmax), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=cuda)
           for k, dt in OUTS}
    torch.cuda.synchronize(cuda)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        torch.ops.mvmatch_views.score_poses_out(*args, 0, c.Gmax, 0, c.n, *(out[k] for k, _ in OUTS))
    assert all((v == (SENT_I if v.dtype == torch.int32 else SENT_F)).all() for v in out.values())   # captured, not run
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)             # hipGraphNodeTypeKernel == 0
    g.replay()
    torch.cuda.synchronize(cuda)
    for k, v in out.items():
        assert M.same(v.cpu().numpy(), eager[k]), k


def test_match_op_captures_into_a_graph(cuda):
    c = MatchCase(5, 65)
    thresholds = [0.5, 1.0, np.inf]
    eager = run_match(c, cuda, thresholds)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    args = (t(c.err), t(c.row_offs), t(c.gt_offs))
    gi = torch.full((3, c.n), SENT_I, dtype=torch.int32, device=cuda)
    tp = torch.full((3, c.S), SENT_I, dtype=torch.int32, device=cuda)
    torch.cuda.synchronize(cuda)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        torch.ops.mvmatch_views.match_scores_out(*args, thresholds, gi, tp)
    assert (gi == SENT_I).all() and (tp == SENT_I).all()
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)
    g.replay()
    torch.cuda.synchronize(cuda)
    assert M.same(gi.cpu().numpy(), eager[0]) and M.same(tp.cpu().numpy(), eager[1])


# ------------------------------------------------------------- wrappers ----
def test_the_wrappers(cuda):
    c = case(257, 5, 5, 5, 2)
    pose, scene, gt_pose, gt_offs, verts, syms = c.device(cuda)
    want = c.expected()
    for res in (ops_views.score_poses(pose, scene, c.gt_pose, c.gt_offs, c.verts, c.syms),          # host arrays
                ops_views.score_poses(pose, scene, gt_pose, gt_offs, verts, syms),                  # device tensors
                ops_views.score_poses(pose, scene, gt_pose, list(c.gt_offs), verts, c.syms)):
        assert res.gt_index is None and res.tp is None and res.err.shape == (c.n, c.Gmax)
        for k in M.KEYS:
            assert M.same(getattr(res, k).cpu().numpy(), want[k]), k
    res = ops_views.score_poses(pose, scene, gt_pose, gt_offs, verts, rows=(5, 9))                  # no symmetry given
    part = M.score_poses(c.pose, c.scene, c.gt_pose, c.gt_offs, c.verts, rows=(5, 9))
    for k in M.KEYS:
        assert M.same(getattr(res, k).cpu().numpy(), part[k]), k
    res = ops_views.score_poses(pose, scene, gt_pose[:0], np.zeros(6, np.int64), verts)             # no object at all
    assert res.err.shape == (c.n, 1) and torch.isinf(res.err).all() and (res.sym < 0).all()
    res = ops_views.score_poses(pose, scene, gt_pose, gt_offs, verts, rows=(2, 2))
    assert res.err.shape == (0, c.Gmax)


def test_argument_errors(cuda):
    c = case(257, 5, 5, 5, 2)
    pose, scene, gt_pose, gt_offs, verts, syms = c.device(cuda)
    f = ops_views.score_poses
    for bad in (dict(rows=(0, c.n + 1)), dict(rows=(3, 2)), dict(rows=(-1, 2)), dict(rows=5), dict(rows=(1, 2, 3))):
        with pytest.raises(ValueError, match="rows"):
            f(pose, scene, gt_pose, gt_offs, verts, syms, **bad)
    for bad_verts in (np.zeros((0, 3)), np.zeros((4, 2)), np.array([[0.0, np.nan, 0]]), np.array([[np.inf, 0, 0]]),
                      np.array([[0.0, 0, BIG]])):
        with pytest.raises(ValueError, match="verts"):
            f(pose, scene, gt_pose, gt_offs, bad_verts, syms)
    f(pose[:9], scene[:9], gt_pose, gt_offs, np.array([[0.0, 0, BELOW]]), syms)
    for bad_syms in (np.zeros((0, 4, 4)), np.zeros((65, 4, 4)), np.zeros((2, 3, 4)), np.full((1, 4, 4), np.nan),
                     np.full((1, 4, 4), -BIG)):
        with pytest.raises(ValueError, match="syms"):
            f(pose, scene, gt_pose, gt_offs, verts, bad_syms)
    for bad_offs in ([0, 3, 2, 5], [], [-1, 2], [0, gt_pose.shape[0] + 1]):
        with pytest.raises(ValueError, match="gt_offs"):
            f(pose, scene, gt_pose, bad_offs, verts, syms)
    with pytest.raises(ValueError, match="gt_pose"):
        f(pose, scene, gt_pose[:, :3], gt_offs, verts, syms)
    with pytest.raises(ValueError, match="gt_pose"):
        f(pose, scene, gt_pose.float(), gt_offs, verts, syms)
    with pytest.raises(ValueError, match="pose"):
        f(pose.float(), scene, gt_pose, gt_offs, verts, syms)
    with pytest.raises(ValueError, match="pose"):
        f(pose.cpu(), scene, gt_pose, gt_offs, verts, syms)
    with pytest.raises(ValueError, match="pose"):
        f(pose[:-1], scene, gt_pose, gt_offs, verts, syms)
    with pytest.raises(ValueError, match="pose"):
        f(pose[:, :3], scene, gt_pose, gt_offs, verts, syms)
    with pytest.raises(ValueError, match="scene"):
        f(pose, scene.to(torch.int64), gt_pose, gt_offs, verts, syms)
    with pytest.raises(ValueError, match="verts"):
        f(pose, scene, gt_pose, gt_offs, verts.float(), syms)
    with pytest.raises(ValueError, match="verts"):
        f(pose, scene, gt_pose, gt_offs, verts[:, :2], syms)
    with pytest.raises(ValueError, match="syms"):
        f(pose, scene, gt_pose, gt_offs, verts, syms.cpu())
    with pytest.raises(ValueError, match="syms"):
        f(pose, scene, gt_pose, gt_offs, verts, torch.zeros((65, 4, 4), dtype=torch.float64, device=cuda))
    # the op's own rows: the outputs, the width and the range
    op = torch.ops.mvmatch_views.score_poses_out
    e = lambda dt=torch.float64: torch.empty((2, c.Gmax), dtype=dt, device=cuda)
    good = dict(err=e(), sym=e(torch.int32), t_err=e(), rot_cos=e())
    call = lambda g_max=c.Gmax, row0=0, **kw: op(pose, scene, gt_pose, gt_offs, verts, syms, 0, g_max, row0, 2,
                                                 *(dict(good, **kw)[k] for k, _ in OUTS))
    call()
    for name in good:
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name][:1]})
    with pytest.raises(ValueError, match="sym"):
        call(sym=good["sym"].to(torch.int64))
    with pytest.raises(ValueError, match="g_max"):
        call(g_max=0)
    with pytest.raises(ValueError, match="err"):
        call(g_max=c.Gmax + 1)
    with pytest.raises(ValueError, match="pose"):
        call(row0=c.n - 1)                                            # rows past the table
    with pytest.raises(ValueError, match="gt_pose"):
        op(pose, scene, gt_pose[:0], gt_offs, verts, syms, 0, c.Gmax, 0, 2, *(good[k] for k, _ in OUTS))

    m = MatchCase(5, 4)
    err = torch.from_numpy(m.err).to(cuda)
    g = ops_views.match_scores
    g(err, m.row_offs, m.gt_offs, [1.0])
    for bad in ([], [1.0] * 17, [np.nan], 3.0):
        with pytest.raises(ValueError, match="thresholds"):
            g(err, m.row_offs, m.gt_offs, bad)
    with pytest.raises(ValueError, match="row_offs"):
        g(err, m.row_offs[::-1].copy(), m.gt_offs, [1.0])
    with pytest.raises(ValueError, match="row_offs"):
        g(err, m.row_offs + 5, m.gt_offs, [1.0])                      # past err's rows
    with pytest.raises(ValueError, match="gt_offs"):
        g(err, m.row_offs, m.gt_offs[:-1], [1.0])
    with pytest.raises(ValueError, match="err"):
        g(err[0], m.row_offs, m.gt_offs, [1.0])
    with pytest.raises(ValueError, match="err"):
        g(err.float(), m.row_offs, m.gt_offs, [1.0])
    with pytest.raises(ValueError, match="err"):
        g(err.cpu(), m.row_offs, m.gt_offs, [1.0])
    with pytest.raises(ValueError, match="g_max"):                    # 1025 columns
        g(torch.zeros((m.n, 1025), dtype=torch.float64, device=cuda), m.row_offs, m.gt_offs, [1.0])
    mop = torch.ops.mvmatch_views.match_scores_out
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    ro, go = t(m.row_offs), t(m.gt_offs)
    gi, tp = torch.empty((2, m.n), dtype=torch.int32, device=cuda), torch.empty((2, 5), dtype=torch.int32, device=cuda)
    mop(err, ro, go, [1.0, 2.0], gi, tp)
    with pytest.raises(ValueError, match="gt_index"):
        mop(err, ro, go, [1.0, 2.0], gi[:1], tp)
    with pytest.raises(ValueError, match="tp"):
        mop(err, ro, go, [1.0, 2.0], gi, tp[:1])
    with pytest.raises(ValueError, match="tp"):
        mop(err, ro, go, [1.0, 2.0], gi, tp.to(torch.int64))
    with pytest.raises(ValueError, match="gt_offs"):
        mop(err, ro, go[:-1], [1.0, 2.0], gi, tp)
    with pytest.raises(ValueError, match="row_offs"):
        mop(err, ro.to(torch.int32), go, [1.0, 2.0], gi, tp)
    with pytest.raises(ValueError, match="thresholds"):
        mop(err, ro, go, [], gi[:0], tp[:0])
