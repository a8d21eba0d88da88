"""mvm_mark_used, mvm_leftover_counts and mvm_leftover_gather on the GPU
(ops_views.mark_used / leftover_counts / leftover_gather) against
the numpy restatement of tests/seed_pass_model.py, exactly: every output is
pre-filled with a sentinel and compared whole."""
import functools

import numpy as np
import pytest
import torch

import seed_pass_model as M
from bpc_baseline_amd import ops_views       # registers torch.ops.mvmatch_views.*

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 257, 1025)
PATTERNS = ("nothing", "everything", "every other", "last")
SENT = 7                       # what ``used`` holds where nothing is marked
FILL = M.I32_MIN + 11          # what the other outputs hold before the ops
SLACK = 2                      # rows behind every capture's matches
TAIL = 5                       # rows behind the gathered sub-batch


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(C, S, pattern, small=False):
    """S captures of C views whose sizes walk SIZES (``small``: 0..5, for many
    captures) and match rows that use ``pattern`` of every view.  Entries that
    use nothing are -1, INT32_MIN, the view's size or (everything / every
    other) a duplicate of the row above; SLACK rows with valid indices follow
    every capture's count and must be ignored."""
    rng = np.random.default_rng(100 * C + S + len(pattern))
    c = Case()
    c.C, c.S = C, S
    sizes = np.array([[(SIZES[(s * C + k) % len(SIZES)] if not small or s < 3 else int(rng.integers(0, 6)))
                       for k in range(C)] for s in range(S)], np.int64)
    c.sizes = sizes
    c.cam_offs = np.zeros(S * C + 1, np.int64)
    np.cumsum(sizes.reshape(-1), out=c.cam_offs[1:])
    n = int(c.cam_offs[-1])
    c.pts = rng.integers(0, 4800, (n, 2)).astype(np.float64) / 2
    c.boxes = rng.integers(-50, 2500, (n, 4)).astype(np.int32)
    rows = []
    for s in range(S):
        mx = int(sizes[s].max())
        n_rows = {"nothing": 3, "everything": mx, "every other": (mx + 1) // 2, "last": 1}[pattern]
        v = np.zeros((n_rows + SLACK, C), np.int64)
        for k in range(C):
            sz = int(sizes[s, k])
            junk = [-1, M.I32_MIN, sz]
            for w in range(n_rows):
                l = {"nothing": -1, "everything": w, "every other": 2 * w, "last": sz - 1}[pattern]
                if pattern == "nothing" or not 0 <= l < sz:
                    l = junk[(w + k) % 3]
                    if pattern in ("everything", "every other") and w % 4 == 3 and w:
                        l = int(v[w - 1, k])                    # a duplicate (or the junk above again)
                v[w, k] = l
            v[n_rows:, k] = 0 if sz else -1                     # beyond count: valid, ignored
        rows.append((n_rows, v))
    c.count = np.array([r[0] for r in rows], np.int32)
    c.match_offs = np.zeros(S + 1, np.int64)
    np.cumsum(c.count + SLACK, out=c.match_offs[1:])
    c.views = np.concatenate([r[1] for r in rows]).astype(np.int32).reshape(-1, C)
    return c


def _marked(c, dev, order=None, seed=(0, 1, 2), sub_offs=None, orig=None, views=None, fill=SENT):
    """(the op's ``used``, the restatement's) on a ``fill``-filled array."""
    n = int(c.cam_offs[-1])
    views = c.views if views is None else views
    used = torch.full((n,), fill, dtype=torch.int32, device=dev)
    ops_views.mark_used(_t(views, dev), _t(c.match_offs, dev), _t(c.count, dev), _t(c.cam_offs, dev), used,
                        c.C, seed, None if sub_offs is None else _t(sub_offs, dev),
                        None if orig is None else _t(orig, dev))
    want = M.mark_used(np.full(n, fill, np.int32), views, c.match_offs, c.count, c.cam_offs, c.C, order,
                       sub_offs, orig)
    return used, want


def _check_leftovers(c, used_host, seed, dev):
    """leftover_counts and leftover_gather of ``used_host`` against the restatement."""
    C = c.C
    order = M.seed_order(seed, C)
    assert ops_views.seed_order(seed, C) == order
    used = _t(used_host, dev)
    counts = torch.full((c.S * C,), FILL, dtype=torch.int32, device=dev)
    ops_views.leftover_counts(used, _t(c.cam_offs, dev), C, seed, out=counts)
    w_pts, w_boxes, w_orig, sub_offs = M.leftover_gather(used_host, c.pts, c.boxes, c.cam_offs, C, order)
    assert np.array_equal(counts.cpu().numpy(), np.diff(sub_offs).astype(np.int32))
    m = int(sub_offs[-1])
    pts = torch.full((m + TAIL, 2), -1.25, dtype=torch.float64, device=dev)
    boxes = torch.full((m + TAIL, 4), FILL, dtype=torch.int32, device=dev)
    orig = torch.full((m + TAIL,), FILL, dtype=torch.int32, device=dev)
    torch.ops.mvmatch_views.leftover_gather_out(used, _t(c.pts, dev), _t(c.boxes, dev), _t(c.cam_offs, dev),
                                                _t(sub_offs, dev), C, list(seed), pts, boxes, orig)
    tail = lambda a, v: np.concatenate([a, np.full((TAIL,) + a.shape[1:], v, a.dtype)])
    assert np.array_equal(pts.cpu().numpy().view(np.int64), tail(w_pts, -1.25).view(np.int64))
    assert np.array_equal(boxes.cpu().numpy(), tail(w_boxes, FILL))
    assert np.array_equal(orig.cpu().numpy(), tail(w_orig, FILL))
    return w_orig, sub_offs


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("C,seed", ((4, (1, 0, 3)), (5, (2, 3, 4)), (8, (3, 4, 5)), (8, (7, 0, 3))))
def test_view_sizes_at_the_chunk_edges(cuda, C, seed, pattern):
    """Views of 0, 1, 63, 64, 65, 127, 128, 129, 257 and 1025 detections in
    every slot over 5 captures; entries that are no index, duplicates and the
    rows at and beyond count mark nothing."""
    c = case(C, 5, pattern)
    used, want = _marked(c, cuda)
    assert np.array_equal(used.cpu().numpy(), want)
    n_marked = int((want == 1).sum())
    n = int(c.cam_offs[-1])
    assert {"nothing": n_marked == 0, "everything": n_marked == n, "last": n_marked == (c.sizes > 0).sum(),
            "every other": n_marked == ((c.sizes + 1) // 2).sum()}[pattern]
    _check_leftovers(c, (want == 1).astype(np.int32), seed, cuda)


@pytest.mark.parametrize("S", (1, 4, 5, 1025))
@pytest.mark.parametrize("C,seed", ((4, (1, 0, 3)), (8, (7, 0, 3))))
def test_capture_counts_at_workgroup_edges(cuda, C, seed, S):
    """Four (capture, slot) waves per workgroup: a part of one, whole ones,
    and a thousand captures with a tail."""
    c = case(C, S, "every other", small=S > 5)
    used, want = _marked(c, cuda)
    assert np.array_equal(used.cpu().numpy(), want)
    _check_leftovers(c, (want == 1).astype(np.int32), seed, cuda)


@pytest.mark.parametrize("C,seed", ((5, (2, 3, 4)), (8, (7, 0, 3))))
def test_marking_the_matches_of_a_later_pass(cuda, C, seed):
    """A pass's views index its own sub-batch: they mark through its
    sub_cam_offs / orig and camera order, on top of what is marked already."""
    c = case(C, 5, "every other")
    used0 = (M.mark_used(np.zeros(int(c.cam_offs[-1]), np.int32), c.views, c.match_offs, c.count, c.cam_offs,
                         C) == 1).astype(np.int32)
    orig, sub_offs = _check_leftovers(c, used0, seed, cuda)
    order = M.seed_order(seed, C)
    # the pass "matches" the first, the last and a few more leftovers of every
    # view, with junk entries beside them
    sub = np.diff(sub_offs).reshape(c.S, C)
    views = np.full_like(c.views, -1)
    for s in range(c.S):
        for w in range(int(c.count[s]) + SLACK):
            for q in range(C):
                sz = int(sub[s, q])
                views[c.match_offs[s] + w, q] = [0, sz - 1, sz, M.I32_MIN, 5 * w][w % 5] if sz else w - 1
    used = _t(used0, cuda)
    ops_views.mark_used(_t(views, cuda), _t(c.match_offs, cuda), _t(c.count, cuda), _t(c.cam_offs, cuda),
                        used, C, seed, _t(sub_offs, cuda), _t(orig, cuda))
    want = M.mark_used(used0.copy(), views, c.match_offs, c.count, c.cam_offs, C, order, sub_offs, orig)
    assert np.array_equal(used.cpu().numpy(), want) and want.sum() > used0.sum()
    _check_leftovers(c, want, seed, cuda)


def test_rows_off_16_byte_alignment(cuda):
    """pts / boxes, and separately pts_out / boxes_out, one element into their
    allocations (test_view_table_gpu's construction): the gather without the
    16-byte accesses writes the aligned run's bytes and leaves the rows behind
    them alone.  Views of 0, 1, 63, 64 and 65 detections, half of them used."""
    C, S, seed = 4, 2, (1, 0, 3)
    rng = np.random.default_rng(41)
    sizes = np.array([[0, 1, 63, 64], [65, 64, 1, 63]], np.int64)
    cam_offs = np.zeros(S * C + 1, np.int64)
    np.cumsum(sizes.reshape(-1), out=cam_offs[1:])
    n = int(cam_offs[-1])
    pts_h = rng.integers(0, 4800, (n, 2)).astype(np.float64) / 2
    boxes_h = rng.integers(-50, 2500, (n, 4)).astype(np.int32)
    used_h = (rng.random(n) < 0.5).astype(np.int32)
    w_pts, w_boxes, w_orig, sub_offs = M.leftover_gather(used_h, pts_h, boxes_h, cam_offs, C,
                                                        M.seed_order(seed, C))
    m = int(sub_offs[-1])
    assert n // 3 < m < 2 * n // 3

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=cuda)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    def run(shift_in, shift_out):
        pts, boxes = _t(pts_h, cuda), _t(boxes_h, cuda)
        outs = [torch.full((m + TAIL, 2), -1.25, dtype=torch.float64, device=cuda),
                torch.full((m + TAIL, 4), FILL, dtype=torch.int32, device=cuda),
                torch.full((m + TAIL,), FILL, dtype=torch.int32, device=cuda)]
        if shift_in:
            pts, boxes = shifted(pts), shifted(boxes)
        if shift_out:
            outs[:2] = [shifted(t) for t in outs[:2]]
        assert (pts.data_ptr() % 16, boxes.data_ptr() % 16) == ((8, 4) if shift_in else (0, 0))
        assert (outs[0].data_ptr() % 16, outs[1].data_ptr() % 16) == ((8, 4) if shift_out else (0, 0))
        torch.ops.mvmatch_views.leftover_gather_out(_t(used_h, cuda), pts, boxes, _t(cam_offs, cuda),
                                                    _t(sub_offs, cuda), C, list(seed), *outs)
        return [t.cpu().numpy() for t in outs]

    aligned = run(False, False)
    tail = lambda a, v: np.concatenate([a, np.full((TAIL,) + a.shape[1:], v, a.dtype)])
    assert np.array_equal(aligned[0].view(np.int64), tail(w_pts, -1.25).view(np.int64))
    assert np.array_equal(aligned[1], tail(w_boxes, FILL)) and np.array_equal(aligned[2], tail(w_orig, FILL))
    for shift in ((True, False), (False, True)):
        got = run(*shift)
        assert np.array_equal(got[0].view(np.int64), aligned[0].view(np.int64)), shift
        assert np.array_equal(got[1], aligned[1]) and np.array_equal(got[2], aligned[2]), shift


def test_wrappers_validate(cuda):
    c = case(5, 4, "last")
    a = dict(views=_t(c.views, cuda), match_offs=_t(c.match_offs, cuda), count=_t(c.count, cuda),
             cam_offs=_t(c.cam_offs, cuda))
    used = torch.zeros(int(c.cam_offs[-1]), dtype=torch.int32, device=cuda)
    for seed in ((0, 1, 1), (0, 1, 5), (0, 1), (-1, 2, 3)):
        with pytest.raises(ValueError, match="seed"):
            ops_views.mark_used(a["views"], a["match_offs"], a["count"], a["cam_offs"], used, 5, seed)
        with pytest.raises(ValueError, match="seed"):
            ops_views.leftover_counts(used, a["cam_offs"], 5, seed)
    for n_cams in (3, 9):
        with pytest.raises(ValueError, match="n_cams"):
            ops_views.leftover_counts(used, a["cam_offs"], n_cams, (0, 1, 2))
    for k, bad in (("views", a["views"].long()), ("match_offs", a["match_offs"][:-1]),
                   ("count", a["count"].long()), ("cam_offs", a["cam_offs"].cpu())):
        args = dict(a, **{k: bad.contiguous()})
        with pytest.raises(ValueError):
            ops_views.mark_used(args["views"], args["match_offs"], args["count"], args["cam_offs"], used, 5)
    with pytest.raises(ValueError, match="go together"):
        ops_views.mark_used(a["views"], a["match_offs"], a["count"], a["cam_offs"], used, 5, (2, 3, 4),
                            a["cam_offs"], None)
    with pytest.raises(ValueError, match="counts"):
        ops_views.leftover_counts(used, a["cam_offs"], 5, (2, 3, 4),
                                  out=torch.zeros(3, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError, match="pts"):
        ops_views.leftover_gather(used, torch.zeros((3, 2), dtype=torch.float64, device=cuda),
                                  torch.zeros((int(used.numel()), 4), dtype=torch.int32, device=cuda),
                                  a["cam_offs"], a["cam_offs"], 5, (2, 3, 4), 4)
    assert not used.any()                                            # nothing was launched


def test_ops_capture_into_a_graph(cuda):
    """Each launch function enqueues one kernel and nothing else (no
    allocation, copy or sync): it captures into a graph of one kernel node
    and no edge, and the replay gives the eager bytes."""
    from test_view_prune_gpu import _graph_shape
    c = case(5, 5, "every other")
    seed, C = (2, 3, 4), 5
    eager_used, want = _marked(c, cuda, fill=0)
    assert np.array_equal(eager_used.cpu().numpy(), want)
    order = M.seed_order(seed, C)
    w_pts, w_boxes, w_orig, sub_offs = M.leftover_gather(want, c.pts, c.boxes, c.cam_offs, C, order)
    m = int(sub_offs[-1])
    dev = cuda
    a = [_t(x, dev) for x in (c.views, c.match_offs, c.count, c.cam_offs, c.pts, c.boxes, sub_offs)]
    views, match_offs, count, cam_offs, pts, boxes, sub = a
    used = torch.zeros(int(c.cam_offs[-1]), dtype=torch.int32, device=dev)
    counts = torch.full((c.S * C,), FILL, dtype=torch.int32, device=dev)
    outs = (torch.full((m, 2), -1.25, dtype=torch.float64, device=dev),
            torch.full((m, 4), FILL, dtype=torch.int32, device=dev),
            torch.full((m,), FILL, dtype=torch.int32, device=dev))
    calls = (lambda: torch.ops.mvmatch_views.mark_used_out(views, match_offs, count, C, [0, 1, 2], None,
                                                           None, cam_offs, used),
             lambda: torch.ops.mvmatch_views.leftover_counts_out(used, cam_offs, C, list(seed), counts),
             lambda: torch.ops.mvmatch_views.leftover_gather_out(used, pts, boxes, cam_offs, sub, C,
                                                                 list(seed), *outs))
    checks = (lambda: np.array_equal(used.cpu().numpy(), want),
              lambda: np.array_equal(counts.cpu().numpy(), np.diff(sub_offs).astype(np.int32)),
              lambda: (np.array_equal(outs[0].cpu().numpy().view(np.int64), w_pts.view(np.int64))
                       and np.array_equal(outs[1].cpu().numpy(), w_boxes)
                       and np.array_equal(outs[2].cpu().numpy(), w_orig)))
    for call, check in zip(calls, checks):
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            call()
        assert not check()                                           # captured, not run
        assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)         # one kernel node, no edge
        g.replay()
        torch.cuda.synchronize(dev)
        assert check()
