"""The dense match table (mvm_compact_matches, ABI 8; MatchBatch.table): every
row is a copy of what the select kernels and the packer wrote, so every
comparison is array_equal on integer views -- no tolerances."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
I32_MIN = np.iinfo(np.int32).min
NAMES = ("dense_offs", "scene", "match", "cost", "X", "boxes", "centroids")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _restate(match, cost, X, count, seg, pts, boxes, cam, base):
    """mvm_compact_matches in numpy (include/mvmatch.h)."""
    S = count.size
    dense = np.zeros(S + 1, np.int64)
    np.cumsum(count, out=dense[1:])
    s_of = np.repeat(np.arange(S), count)
    src = seg[s_of] + np.arange(dense[-1]) - dense[s_of]
    m = match[src]
    det = cam[3 * s_of[:, None] + np.arange(3)] + m
    return dense, (base + s_of).astype(np.int32), m, cost[src], X[src], boxes[det], pts[det]


def _inputs(counts, caps, views, rng):
    """Hand-built select / packer outputs: scene s has ``counts[s]`` matches in
    a segment of ``caps[s]`` rows and views of ``views[s]`` detections.
    Unused rows hold sentinels (match INT32_MIN, cost / X NaN); pts / boxes
    carry two rows beyond the last view (NaN, -1)."""
    counts, caps = np.asarray(counts, np.int32), np.asarray(caps, np.int64)
    views = np.asarray(views, np.int64).reshape(-1, 3)
    S = counts.size
    seg = np.zeros(S + 1, np.int64)
    np.cumsum(caps, out=seg[1:])
    cam = np.zeros(3 * S + 1, np.int64)
    np.cumsum(views.reshape(-1), out=cam[1:])
    cap, n = int(seg[-1]), int(cam[-1])
    match = np.full((cap, 3), I32_MIN, np.int32)
    cost = np.full(cap, np.nan, np.float32)
    X = np.full((cap, 3), np.nan, np.float64)
    for s in range(S):
        k = int(counts[s])
        assert k <= caps[s] and (k == 0 or views[s].min() > 0)
        rows = slice(seg[s], seg[s] + k)
        match[rows] = rng.integers(0, np.maximum(views[s], 1), (k, 3))
        cost[rows] = rng.uniform(0, 30, k)
        X[rows] = rng.normal(size=(k, 3))
    pts = np.full((n + 2, 2), np.nan, np.float64)
    boxes = np.full((n + 2, 4), -1, np.int32)
    pts[:n] = rng.integers(0, 4000, (n, 2)) * 0.5
    boxes[:n] = rng.integers(0, 2000, (n, 4))
    return match, cost, X, counts, seg, pts, boxes, cam


def _check(cuda, arrays, base=0):
    """ops.compact_matches equals the restatement below n = count.sum(); the op
    on outputs pre-filled with sentinels writes no row at or beyond n."""
    from bpc_baseline_amd import ops
    dev = [torch.from_numpy(a).to(cuda) for a in arrays]
    ref = _restate(*arrays, base)
    n = int(ref[0][-1])
    got = [t.cpu().numpy() for t in ops.compact_matches(*dev, scene_base=base)]
    assert np.array_equal(got[0], ref[0]), "dense_offs"
    for name, g, r in zip(NAMES[1:], got[1:], ref[1:]):
        assert g.shape[0] == arrays[0].shape[0] and g.shape[1:] == r.shape[1:], name
        assert g.dtype == r.dtype and np.array_equal(_bits(g[:n]), _bits(r)), name
        # no sentinel reached a row below n
        assert not np.isnan(g[:n]).any() if g.dtype.kind == "f" else (g[:n] >= 0).all(), name
    cap = arrays[0].shape[0]
    if cap == 0 or arrays[5].size == 0:
        return got
    S = arrays[3].size
    outs = [torch.full((S + 1,), -7, dtype=torch.int64, device=cuda),
            torch.full((cap,), I32_MIN, dtype=torch.int32, device=cuda),
            torch.full((cap, 3), I32_MIN, dtype=torch.int32, device=cuda),
            torch.full((cap,), np.nan, dtype=torch.float32, device=cuda),
            torch.full((cap, 3), np.nan, dtype=torch.float64, device=cuda),
            torch.full((cap, 3, 4), I32_MIN, dtype=torch.int32, device=cuda),
            torch.full((cap, 3, 2), np.nan, dtype=torch.float64, device=cuda)]
    torch.ops.mvmatch.compact_matches_out(*dev, base, *outs)
    outs = [t.cpu().numpy() for t in outs]
    assert np.array_equal(outs[0], ref[0])
    for name, o, r in zip(NAMES[1:], outs[1:], ref[1:]):
        assert np.array_equal(_bits(o[:n]), _bits(r)), name
        tail = o[n:]
        assert np.isnan(tail).all() if tail.dtype.kind == "f" else (tail == I32_MIN).all(), name
    return got


@pytest.mark.parametrize("count,cap", [(0, 5), (7, 7), (64, 64), (1, 1)])
def test_single_scene_extremes(cuda, count, cap):
    rng = np.random.default_rng(count)
    _check(cuda, _inputs([count], [cap], [(9, 4, 6)], rng))


@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257, 1024])
def test_counts_at_wave_and_workgroup_edges(cuda, count):
    rng = np.random.default_rng(count)
    _check(cuda, _inputs([count], [1024], [(32, 32, 32)], rng))


def test_empty_scenes(cuda):
    rng = np.random.default_rng(1)
    _check(cuda, _inputs([0, 3, 0, 0, 2], [4, 3, 0, 6, 5], [(5, 5, 5)] * 5, rng))
    # a scene with an empty view (cam_offs repeated) and no match, between two others
    _check(cuda, _inputs([2, 0, 3], [2, 0, 4], [(3, 4, 5), (6, 0, 7), (4, 4, 4)], rng))
    _check(cuda, _inputs([0], [0], [(0, 3, 3)], rng))        # no capacity at all: nothing launched


@pytest.mark.parametrize("S,base", [(1023, 0), (1024, 5), (1025, 0), (2049, 1 << 20)])
def test_many_scenes(cuda, S, base):
    """The scan's per-thread ranges (1, 2 and 3 counts per thread) and the
    four-scenes-per-workgroup tail; scene ids start at ``base``."""
    rng = np.random.default_rng(S)
    got = _check(cuda, _inputs(rng.integers(0, 3, S), [2] * S, [(2, 1, 3)] * S, rng), base)
    n = int(got[0][-1])
    assert n > S // 2 and got[1][0] >= base and got[1][n - 1] <= base + S - 1


def test_rows_off_16_byte_alignment(cuda):
    """boxes / pts one element into their allocations: the copy without the
    16-byte accesses gives the same table."""
    from bpc_baseline_amd import ops
    rng = np.random.default_rng(3)
    arrays = _inputs([5, 0, 70], [8, 2, 70], [(7, 9, 8), (1, 1, 1), (20, 20, 20)], rng)
    dev = [torch.from_numpy(a).to(cuda) for a in arrays]
    pts, boxes = arrays[5], arrays[6]
    p = torch.zeros(pts.size + 1, dtype=torch.float64, device=cuda)
    b = torch.zeros(boxes.size + 1, dtype=torch.int32, device=cuda)
    p[1:] = dev[5].reshape(-1)
    b[1:] = dev[6].reshape(-1)
    dev[5], dev[6] = p[1:].view(-1, 2), b[1:].view(-1, 4)
    assert dev[5].data_ptr() % 16 == 8 and dev[6].data_ptr() % 16 == 4
    ref = _restate(*arrays, 0)
    n = int(ref[0][-1])
    got = [t.cpu().numpy() for t in ops.compact_matches(*dev)]
    assert np.array_equal(got[0], ref[0])
    for name, g, r in zip(NAMES[1:], got[1:], ref[1:]):
        assert np.array_equal(_bits(g[:n]), _bits(r)), name


@pytest.mark.parametrize("keep_cube", [False, True])
def test_table_equals_batch_predictions(cuda, keep_cube):
    """A mixed match_captures batch (8, 24 and 64 detections per view: without
    the cube it goes through the split chain; one capture with its first view
    emptied): table().predictions(s) is MatchBatch.predictions(s) element for
    element, and scene / offs agree with count."""
    from bpc_baseline_amd.inference.batch_match import match_captures
    from sharded_match_worker import CONF_THRESH, MATCH_THRESH, NO_MATCHES, SIZES, mixed_captures, to_device
    res = match_captures(*to_device(mixed_captures(), cuda), conf_thresh=CONF_THRESH,
                         matching_threshold=MATCH_THRESH, keep_cube=keep_cube)
    S = len(SIZES)
    assert res.count[NO_MATCHES] == 0 and res.count.sum() > 2 * S
    assert res.offs_dev is not None and np.array_equal(res.offs_dev.cpu().numpy(), res.offs)
    tab = res.table()
    n = int(res.count.sum())
    assert np.array_equal(np.diff(tab.offs), res.count) and tab.offs[0] == 0
    assert np.array_equal(tab.scene.cpu().numpy(), np.repeat(np.arange(S), res.count).astype(np.int32))
    for k, tail in (("scene", ()), ("match", (3,)), ("cost", ()), ("X", (3,)), ("boxes", (3, 4)),
                    ("centroids", (3, 2))):
        assert tuple(getattr(tab, k).shape) == (n,) + tail, k
    for s in range(S):
        got, ref = tab.predictions(s), res.predictions(s)
        assert len(got) == len(ref) == res.count[s]
        for g, r in zip(got, ref):
            for a, b in zip(g, r):
                assert a.dtype == b.dtype and a.shape == b.shape
                assert np.array_equal(_bits(a), _bits(b))
        o = int(res.offs[s])
        rows = slice(int(tab.offs[s]), int(tab.offs[s + 1]))
        assert torch.equal(tab.match[rows], res.match[o:o + int(res.count[s])])
        assert np.array_equal(_bits(tab.cost[rows].cpu().numpy()),
                              _bits(res.cost[o:o + int(res.count[s])].cpu().numpy()))
    # a batch built without the device copies (the fields default to None) uploads them
    import dataclasses
    bare = dataclasses.replace(res, offs_dev=None, count_dev=None, cam_offs_dev=None)
    assert torch.equal(bare.table(scene_base=9).match, tab.match)
    assert int(bare.table(scene_base=9).scene[0]) == 9


def test_empty_batches_launch_nothing(cuda):
    """No captures, and captures without a match: an empty table."""
    import dataclasses
    from bpc_baseline_amd.inference.batch_match import match_captures
    from sharded_match_worker import capture_range, mixed_captures, to_device, NO_MATCHES
    one = match_captures(*to_device(capture_range(mixed_captures(), NO_MATCHES, NO_MATCHES + 1), cuda))
    assert one.count.tolist() == [0]
    none = dataclasses.replace(one, match=one.match[:0], cost=one.cost[:0], X=one.X[:0],
                               count=one.count[:0], offs=one.offs[:1], cam_offs=one.cam_offs[:1],
                               offs_dev=None, count_dev=None, cam_offs_dev=None)
    for S, batch in ((1, one), (0, none)):
        tab = batch.table()
        assert tab.offs.tolist() == [0] * (S + 1)
        assert tab.scene.numel() == 0 and tuple(tab.boxes.shape) == (0, 3, 4)
        assert tab.host()["X"].shape == (0, 3)
