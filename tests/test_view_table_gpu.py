"""The dense match table of a C-camera batch (mvm_compact_matches_views;
MatchBatch.table(reproj=True), the table of n_cams > 3) against a numpy
restatement of include/mvmatch.h.  Every copied value is compared as
array_equal on integer views; the reprojection residual is a fixed sequence
of single IEEE operations, restated elementwise (no ``@``: a BLAS may fuse),
so it is compared bit for bit too -- no tolerance anywhere."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
I32_MIN = np.iinfo(np.int32).min
NAMES = ("dense_offs", "scene", "views", "n_views", "cost", "ext_cost", "X", "boxes", "centroids",
         "reproj")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _residual(P, X, cent):
    """The header's reprojection residual, elementwise: P [..., 3, 4],
    X [..., 3], cent [..., 2] -> [...]."""
    with np.errstate(all="ignore"):
        h = [((P[..., q, 0] * X[..., 0] + P[..., q, 1] * X[..., 1]) + P[..., q, 2] * X[..., 2])
             + P[..., q, 3] for q in range(3)]
        u = h[0] / h[2]
        v = h[1] / h[2]
        du = u - cent[..., 0]
        dv = v - cent[..., 1]
        return np.sqrt(du * du + dv * dv)


def _restate(views, cost, ext, X, count, seg, pts, boxes, cam, proj, base):
    """mvm_compact_matches_views in numpy (include/mvmatch.h)."""
    S, C = count.size, views.shape[1]
    dense = np.zeros(S + 1, np.int64)
    np.cumsum(count, out=dense[1:])
    s_of = np.repeat(np.arange(S), count)
    src = seg[s_of] + np.arange(dense[-1]) - dense[s_of]
    v = views[src]
    keep = v >= 0
    det = cam[C * s_of[:, None] + np.arange(C)] + np.where(keep, v, 0)
    det = np.where(keep, det, 0)
    bx = np.where(keep[..., None], boxes[det], np.int32(-1)).astype(np.int32)
    ct = np.where(keep[..., None], pts[det], np.nan)
    rp = np.where(keep, _residual(proj[s_of], X[src][:, None, :], ct), np.nan)
    return (dense, (base + s_of).astype(np.int32), v, keep.sum(axis=1).astype(np.int32), cost[src],
            ext[src], X[src], bx, ct, rp)


def _inputs(C, counts, caps, nviews, rng, extra="mixed"):
    """Hand-built select / extend / packer outputs: capture s has ``counts[s]``
    matches in a segment of ``caps[s]`` rows and views of ``nviews[s]``
    detections.  ``extra``: the extra view slots of a match all -1 ("none"),
    all kept where the view has a detection ("all"), or either ("mixed").
    Unused rows hold sentinels (views INT32_MIN, cost / ext_cost / X NaN);
    pts / boxes carry two rows beyond the last view (NaN, -1)."""
    counts, caps = np.asarray(counts, np.int32), np.asarray(caps, np.int64)
    nviews = np.asarray(nviews, np.int64).reshape(-1, C)
    S = counts.size
    seg = np.zeros(S + 1, np.int64)
    np.cumsum(caps, out=seg[1:])
    cam = np.zeros(C * S + 1, np.int64)
    np.cumsum(nviews.reshape(-1), out=cam[1:])
    cap, n = int(seg[-1]), int(cam[-1])
    views = np.full((cap, C), I32_MIN, np.int32)
    cost = np.full(cap, np.nan, np.float32)
    ext = np.full((cap, C - 3), np.nan, np.float32)
    X = np.full((cap, 3), np.nan, np.float64)
    for s in range(S):
        k = int(counts[s])
        assert k <= caps[s] and (k == 0 or nviews[s, :3].min() > 0)
        rows = slice(seg[s], seg[s] + k)
        v = rng.integers(0, np.maximum(nviews[s], 1), (k, C))
        drop = {"none": np.ones((k, C), bool), "all": np.zeros((k, C), bool),
                "mixed": rng.random((k, C)) < 0.5}[extra]
        drop |= nviews[s][None, :] == 0
        drop[:, :3] = False
        views[rows] = np.where(drop, -1, v)
        cost[rows] = rng.uniform(0, 30, k)
        ext[rows] = np.where(drop[:, 3:], np.inf, rng.uniform(0, 30, (k, C - 3)))
        X[rows] = rng.normal(size=(k, 3))
    pts = np.full((n + 2, 2), np.nan, np.float64)
    boxes = np.full((n + 2, 4), -1, np.int32)
    pts[:n] = rng.integers(0, 4000, (n, 2)) * 0.5
    boxes[:n] = rng.integers(0, 2000, (n, 4))
    # P of a camera looking down +z from a few units away: h_2 stays off 0
    proj = rng.normal(size=(S, C, 3, 4)) * np.array([1500.0, 1500.0, 1.0])[:, None]
    proj[:, :, 2, 3] += 8.0
    return views, cost, ext, X, counts, seg, pts, boxes, cam, proj


def _sentinels(cuda, S, cap, C):
    f = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=cuda)
    return [f((S + 1,), -7, torch.int64), f((cap,), I32_MIN, torch.int32), f((cap, C), I32_MIN, torch.int32),
            f((cap,), I32_MIN, torch.int32), f((cap,), np.nan, torch.float32),
            f((cap, C - 3), np.nan, torch.float32), f((cap, 3), np.nan, torch.float64),
            f((cap, C, 4), I32_MIN, torch.int32), f((cap, C, 2), np.nan, torch.float64),
            f((cap, C), np.nan, torch.float64)]


def _compare(name, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, name
    if got.dtype.kind != "f":
        assert np.array_equal(got, ref), name
        return
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), name          # NaN exactly where the restatement is
    assert np.array_equal(_bits(got)[~nan], _bits(ref)[~nan]), name


def _check_out(outs, ref, sentinel_tail=True):
    n = int(ref[0][-1])
    assert np.array_equal(outs[0], ref[0]), "dense_offs"
    for name, o, r in zip(NAMES[1:], outs[1:], ref[1:]):
        _compare(name, o[:n], r)
        if sentinel_tail:
            tail = o[n:]
            assert np.isnan(tail).all() if tail.dtype.kind == "f" else (tail == I32_MIN).all(), name


def _check(cuda, arrays, base=0):
    """The op on outputs pre-filled with sentinels equals the restatement
    below n = count.sum() and writes no row at or beyond n; the allocating
    wrapper gives the same rows."""
    from bpc_baseline_amd import ops
    dev = [torch.from_numpy(a).to(cuda) for a in arrays]
    ref = _restate(*arrays, base)
    S, (cap, C) = arrays[4].size, arrays[0].shape
    outs = _sentinels(cuda, S, cap, C)
    torch.ops.mvmatch.compact_matches_views_out(*dev, base, *outs)
    _check_out([t.cpu().numpy() for t in outs], ref)
    got = [t.cpu().numpy() for t in ops.compact_matches_views(*dev, scene_base=base)]
    assert all(g.shape[0] == cap for g in got[1:])
    _check_out(got, ref, sentinel_tail=False)
    return ref


# per-capture counts at the wave's edges, and count == capacity (captures 1, 3 and 6)
COUNTS = [0, 1, 63, 64, 65, 257, 7]
CAPS = [5, 1, 64, 64, 70, 300, 7]


@pytest.mark.parametrize("extra", ["none", "all", "mixed"])
@pytest.mark.parametrize("C", [3, 4, 5, 8])
def test_counts_and_view_slots(cuda, C, extra):
    rng = np.random.default_rng(10 * C + len(extra))
    ref = _check(cuda, _inputs(C, COUNTS, CAPS, [(40,) * C] * len(COUNTS), rng, extra), base=3)
    kept = ref[2][:, 3:] >= 0
    if C > 3:
        assert {"none": not kept.any(), "all": kept.all(), "mixed": kept.any() and not kept.all()}[extra]
    if C > 4 and extra == "mixed":           # a row that kept some of its extra views and not others
        assert (kept.any(axis=1) & ~kept.all(axis=1)).any()
    assert np.array_equal(ref[3], 3 + kept.sum(axis=1))


@pytest.mark.parametrize("S,base", [(1, 0), (4, 7), (5, 1 << 20), (1025, 9)])
@pytest.mark.parametrize("C", [3, 4, 8])
def test_capture_counts_at_workgroup_edges(cuda, C, S, base):
    """Four captures per workgroup: a part of one, exactly one, one more, and
    several workgroups with a tail; scene ids start at ``base``."""
    rng = np.random.default_rng(S + C)
    nv = [tuple(2 + (c + s) % 3 for c in range(C)) for s in range(S)]
    ref = _check(cuda, _inputs(C, rng.integers(1 if S < 8 else 0, 4, S), [3] * S, nv, rng), base)
    n = int(ref[0][-1])
    assert n > S // 2 and ref[1][0] >= base and ref[1][n - 1] <= base + S - 1


@pytest.mark.parametrize("C", [4, 5, 8])
def test_empty_views_and_captures(cuda, C):
    """An extra view without a detection (cam_offs repeated) in a capture
    that has matches: its slot is -1 in every row; captures without a match,
    without capacity, and with an empty first view between the others."""
    rng = np.random.default_rng(C)
    full = (6,) * C
    hole = (5, 4, 6) + (0,) + (3,) * (C - 4)          # camera 3 saw nothing
    last = (5, 4, 6) + (3,) * (C - 4) + (0,)          # camera C-1 saw nothing
    blind = (0,) + (4,) * (C - 1)                      # no match possible
    arrays = _inputs(C, [3, 0, 70, 0, 5, 2], [4, 0, 70, 6, 5, 3], [full, full, hole, blind, last, full],
                     rng, "all")
    ref = _check(cuda, arrays)
    s_of = ref[1]
    assert (ref[2][s_of == 2, 3] == -1).all() and (ref[2][s_of == 4, C - 1] == -1).all()
    assert np.isnan(ref[9][s_of == 2, 3]).all() and (ref[7][s_of == 2, 3] == -1).all()
    assert (ref[2][s_of == 0] >= 0).all()
    # no capacity at all: nothing is launched, the offsets stay 0
    from bpc_baseline_amd import ops
    none = _inputs(C, [0], [0], [blind], rng)
    got = ops.compact_matches_views(*[torch.from_numpy(a).to(cuda) for a in none])
    assert got[0].tolist() == [0, 0] and got[1].numel() == 0 and tuple(got[7].shape) == (0, C, 4)


@pytest.mark.parametrize("C", [3, 5])
def test_rows_off_16_byte_alignment(cuda, C):
    """pts / boxes and the row outputs one element into their allocations:
    the copy without the 16-byte accesses gives the same table."""
    rng = np.random.default_rng(30 + C)
    arrays = _inputs(C, [5, 0, 70], [8, 2, 70], [(7,) * C, (1,) * C, (20,) * C], rng)
    ref = _restate(*arrays, 0)
    dev = [torch.from_numpy(a).to(cuda) for a in arrays]
    S, cap = 3, arrays[0].shape[0]

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=cuda)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    dev[6], dev[7] = shifted(dev[6]), shifted(dev[7])
    outs = [shifted(t) if k >= 7 else t for k, t in enumerate(_sentinels(cuda, S, cap, C))]
    assert dev[6].data_ptr() % 16 == 8 and dev[7].data_ptr() % 16 == 4
    assert outs[7].data_ptr() % 16 == 4 and outs[8].data_ptr() % 16 == 8
    torch.ops.mvmatch.compact_matches_views_out(*dev, 0, *outs)
    _check_out([t.cpu().numpy() for t in outs], ref)


@pytest.mark.parametrize("C", [3, 4])
def test_zero_third_row_of_P(cuda, C):
    """h_2 exactly 0 (a P whose third row is zero, with either sign of the
    products): the division gives inf, or NaN where h_0 or h_1 is 0 too, as
    IEEE does and as the restatement does."""
    rng = np.random.default_rng(50 + C)
    arrays = _inputs(C, [6, 4], [6, 4], [(5,) * C] * 2, rng, "all")
    proj = arrays[9]
    proj[0, 1, 2, :] = 0.0
    proj[1, C - 1, 2, :] = 0.0
    proj[1, C - 1, 0, :] = 0.0                          # h_0 == 0 as well: 0 / 0
    ref = _check(cuda, arrays)
    rp, s_of = ref[9], ref[1]
    assert np.isinf(rp[s_of == 0, 1]).all() and np.isnan(rp[s_of == 1, C - 1]).all()
    assert np.isfinite(rp[s_of == 0, 0]).all()


def test_three_cameras_equal_compact_matches(cuda):
    """C = 3 through the new op (views = match): the six fields it shares with
    ops.compact_matches are equal bit for bit, and n_views is 3."""
    from bpc_baseline_amd import ops
    rng = np.random.default_rng(8)
    arrays = _inputs(3, [5, 0, 70, 64], [8, 2, 70, 64], [(7, 9, 8), (1, 1, 1), (20, 20, 20), (9, 9, 9)], rng)
    views, cost, ext, X, count, seg, pts, boxes, cam, proj = [torch.from_numpy(a).to(cuda) for a in arrays]
    new = ops.compact_matches_views(views, cost, None, X, count, seg, pts, boxes, cam, proj, scene_base=4)
    old = ops.compact_matches(views, cost, X, count, seg, pts, boxes, cam, scene_base=4)
    n = int(old[0][-1])
    assert n == 139 and torch.equal(new[0], old[0])
    for k_new, k_old in ((1, 1), (2, 2), (4, 3), (6, 4), (7, 5), (8, 6)):
        a, b = new[k_new][:n].cpu().numpy(), old[k_old][:n].cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), NAMES[k_new]
    assert (new[3][:n] == 3).all() and tuple(new[5].shape) == (views.shape[0], 0)


def test_op_validates(cuda):
    rng = np.random.default_rng(2)
    arrays = _inputs(4, [2], [3], [(4,) * 4], rng)
    dev = [torch.from_numpy(a).to(cuda) for a in arrays]
    outs = _sentinels(cuda, 1, 3, 4)
    for k, bad in ((0, dev[0][:, :2].contiguous()), (9, dev[9][:, :3].contiguous()), (3, dev[3].float())):
        args = list(dev)
        args[k] = bad
        with pytest.raises(ValueError):
            torch.ops.mvmatch.compact_matches_views_out(*args, 0, *outs)
    with pytest.raises(ValueError):
        torch.ops.mvmatch.compact_matches_views_out(*dev, 0, *outs[:-1], outs[-1][:2])


# ----------------------------------------------------------- end to end ----
def _end_to_end(cuda, C, rig):
    import test_extend_gpu as TE
    from bpc_baseline_amd.inference.batch_match import match_captures
    f = TE.fixture(C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return f, match_captures(t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs, rig=rig, n_cams=C)


@pytest.mark.parametrize("rig", ("host", "device"))
@pytest.mark.parametrize("C", (4, 5))
def test_table_of_a_c_camera_batch(cuda, C, rig):
    """8 make_capture captures (clutter added to / detections dropped from the
    extra views, an empty extra view, a capture without a match):
    table(reproj=True).predictions(s) is MatchBatch.predictions(s) element for element,
    cams included, and reprojection(s) the restatement on the batch's own X
    and proj."""
    f, res = _end_to_end(cuda, C, rig)
    S = f.S
    assert res.proj is not None and tuple(res.proj.shape) == (S, C, 3, 4)
    tab = res.table(reproj=True)
    n = int(res.count.sum())
    assert tab.n_cams == C and tab.fields() == tab.FIELDS + ("views", "n_views", "ext_cost", "reproj")
    for k, tail in (("scene", ()), ("match", (3,)), ("cost", ()), ("X", (3,)), ("boxes", (C, 4)),
                    ("centroids", (C, 2)), ("views", (C,)), ("n_views", ()), ("ext_cost", (C - 3,)),
                    ("reproj", (C,))):
        assert tuple(getattr(tab, k).shape) == (n,) + tail, k
    assert np.array_equal(np.diff(tab.offs), res.count) and tab.offs[0] == 0
    assert np.array_equal(tab.scene.cpu().numpy(), np.repeat(np.arange(S), res.count).astype(np.int32))
    assert torch.equal(tab.match, tab.views[:, :3])
    assert (res.count == 0).any() and (f.counts[res.count > 0, 3:] == 0).any()
    proj, h = res.proj.cpu().numpy(), res.host()
    kept_extra = 0
    for s in range(S):
        got, ref, rep = tab.predictions(s), res.predictions(s), tab.reprojection(s)
        assert len(got) == len(ref) == len(rep) == res.count[s]
        o = int(res.offs[s])
        for w, (g, r) in enumerate(zip(got, ref)):
            assert len(g) == len(r) == 4
            for a, b in zip(g, r):
                assert a.dtype == b.dtype and a.shape == b.shape
                assert np.array_equal(_bits(a), _bits(b))
            cams = r[3]
            want = _residual(proj[s, cams], h["X"][o + w][None, :], r[1])
            assert rep[w].dtype == np.float64 and np.array_equal(_bits(rep[w]), _bits(want))
            assert np.isfinite(want).all()
            kept_extra += len(cams) > 3
        rows = slice(int(tab.offs[s]), int(tab.offs[s + 1]))
        sl = slice(o, o + int(res.count[s]))
        assert torch.equal(tab.views[rows], res.views[sl])
        assert np.array_equal(_bits(tab.ext_cost[rows].cpu().numpy()), _bits(res.ext_cost[sl].cpu().numpy()))
        assert torch.equal(tab.n_views[rows], (res.views[sl] >= 0).sum(dim=1).to(torch.int32))
    # rows that kept an extra view and rows that kept none both occur
    assert 0 < kept_extra < n
    # a batch built without the device copies uploads them; scene ids from scene_base
    bare = dataclasses.replace(res, offs_dev=None, count_dev=None, cam_offs_dev=None)
    other = bare.table(scene_base=9, reproj=True)
    assert torch.equal(other.views, tab.views) and int(other.scene[0]) == 9
    assert np.array_equal(_bits(other.reproj.cpu().numpy()), _bits(tab.reproj.cpu().numpy()))
    with pytest.raises(ValueError):
        dataclasses.replace(res, proj=None).table(reproj=True)


def test_three_camera_table_with_reproj(cuda):
    """table(reproj=True) of a three-camera batch: the six fields of table()
    bit for bit, n_views == 3, and the residuals of the restatement."""
    import test_extend_gpu as TE
    from bpc_baseline_amd.inference.batch_match import MatchTable, match_captures
    b3 = TE.three_cam_inputs(TE.fixture(4))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    res = match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5])
    plain, tab = res.table(), res.table(reproj=True)
    n = int(res.count.sum())
    assert n > 8 and plain.fields() == MatchTable.FIELDS and plain.reproj is None and plain.n_cams == 3
    assert res.table(reproj=False).fields() == MatchTable.FIELDS
    for k in MatchTable.FIELDS:
        a, b = getattr(tab, k).cpu().numpy(), getattr(plain, k).cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k
    assert np.array_equal(tab.offs, plain.offs)
    assert (tab.n_views == 3).all() and torch.equal(tab.views, tab.match)
    assert tuple(tab.ext_cost.shape) == (n, 0) and tuple(tab.reproj.shape) == (n, 3)
    proj = res.proj.cpu().numpy()
    for s in range(len(res.count)):
        pred, rep = tab.predictions(s), tab.reprojection(s)
        assert len(pred) == len(rep) == res.count[s]
        for (_, cent, X), r in zip(pred, rep):
            assert np.array_equal(_bits(r), _bits(_residual(proj[s], X[None, :], cent)))
    with pytest.raises(ValueError):
        dataclasses.replace(res, proj=None).table(reproj=True)
    assert dataclasses.replace(res, proj=None).table().fields() == MatchTable.FIELDS
    with pytest.raises(ValueError):
        plain.reprojection(0)


def test_empty_c_camera_batches(cuda):
    """Captures without a match: an empty table of the C-camera shapes."""
    f, res = _end_to_end(cuda, 4, "host")
    none = dataclasses.replace(res, count=np.zeros_like(res.count), count_dev=None)
    tab = none.table(reproj=True)
    assert tab.offs.tolist() == [0] * (f.S + 1) and tab.n_cams == 4
    assert tuple(tab.boxes.shape) == (0, 4, 4) and tuple(tab.reproj.shape) == (0, 4)
    assert tab.host()["views"].shape == (0, 4) and tab.predictions(0) == [] and tab.reprojection(0) == []
