"""Pruning of extra views by reprojection residual on the GPU
(mvm_prune_views_triangulate, ops_views.prune_views,
match_captures(reproj_gate=G)) against the numpy restatement of
tests/view_prune_model.py.

The op is called directly on the builders' inputs with ``pruned`` pre-filled
with a sentinel.  ``views``, ``ext_cost`` and ``pruned`` are compared exactly
(tests/test_view_prune_model.py proves on the CPU that no decision of these
inputs is closer than the two DLTs can differ, so no row is left out), ``X``
bit for bit on rows that dropped nothing and within §3.8's rtol 1e-10 / atol
1e-9 of the restatement elsewhere."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import view_prune_model as M
from bpc_baseline_amd import ops_views       # registers torch.ops.mvmatch_views.*

pytestmark = pytest.mark.gpu
SENT = M.I32_MIN + 5             # what ``pruned`` holds before the op


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _device_args(c, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in c.args()]


def _run(c, gate, dev):
    """The op on a copy of the case's arrays -> (views, ext_cost, X, pruned) on the host."""
    a = _device_args(c, dev)
    pruned = torch.full((c.views.shape[0],), SENT, dtype=torch.int32, device=dev)
    torch.ops.mvmatch_views.prune_views_out(*a, float(gate), c.C, pruned)
    return [t.cpu().numpy() for t in (a[0], a[1], a[2], pruned)]


def _check(name, C, gate, dev):
    c = M.case(name, C)
    views, ext, X, pruned = _run(c, gate, dev)
    w_views, w_ext, w_X, w_pruned, touched, _ = M.expected(name, C, gate)
    # whole arrays: the rows at and beyond every capture's count keep their sentinels
    assert np.array_equal(views, w_views)
    assert np.array_equal(_bits(ext), _bits(w_ext))
    assert np.array_equal(pruned, np.where(touched, w_pruned, SENT))
    same = w_pruned == 0
    assert np.array_equal(_bits(X[same]), _bits(c.X[same]))          # not written: the input's bits
    np.testing.assert_allclose(X[~same], w_X[~same], rtol=M.RTOL, atol=M.ATOL)
    return c, w_pruned, touched


@pytest.mark.parametrize("gate", M.GATES)
@pytest.mark.parametrize("C", (4, 5, 8))
def test_counts_at_the_waves_edges(cuda, C, gate):
    """Captures of 0, 1, 63, 64, 65, 257 matches and count = capacity; an empty
    extra view (capture 4); two rows with a seed index out of range and one
    with an extra-view index that is no detection of its view: untouched."""
    c, pruned, touched = _check("counts", C, gate, cuda)
    skip = c.kind == "skip"
    assert skip.sum() == 3 and (pruned[skip] == 0).all()
    if 0 < gate < np.inf:
        assert (pruned[touched] != 0).any() and (pruned[touched] == 0).any()
    if gate == np.inf:
        assert (pruned == 0).all()


@pytest.mark.parametrize("gate", (1.0, 5.0))
@pytest.mark.parametrize("S", (1, 4, 5, 1025))
@pytest.mark.parametrize("C", (4, 8))
def test_capture_counts_at_workgroup_edges(cuda, C, S, gate):
    """Four captures per workgroup: a part of one, exactly one, one more, and
    several workgroups with a tail."""
    c, pruned, touched = _check(f"captures{S}", C, gate, cuda)
    assert touched.sum() == c.count.sum() and (S < 1025 or (pruned != 0).sum() > 100)


@pytest.mark.parametrize("gate", M.GATES)
@pytest.mark.parametrize("C", (4, 5))
def test_nan_and_inf_residuals(cuda, C, gate):
    """A P with a zero third row in camera C-1: with its first row zero as
    well the residual is NaN (capture 0) -- a candidate at every gate, +inf
    included, and dropped first; alone, inf (capture 1)."""
    c, pruned, _ = _check("nan", C, gate, cuda)
    o = int(c.match_offs[0])
    assert ((pruned[o:o + 12] >> (C - 1)) & 1).all()


@pytest.mark.parametrize("gate", (1.0, 5.0, 20.0))
@pytest.mark.parametrize("C", (5, 8))
def test_exact_tie_between_two_extra_views(cuda, C, gate):
    """Camera 4 is camera 3 again, shifted detection included, so the two
    residuals have equal bits and the kernel must cope with the tie: its final
    state equals the restatement's.  Which of the two leaves first is NOT
    observable here: with exact duplicates the survivor's residual only rises
    once its twin is gone, every tied row ends with both dropped, and views,
    ext_cost, pruned and X are the same either way.  The lowest-camera rule is
    pinned on the restatement alone (tests/test_view_prune_model.py)."""
    c, pruned, _ = _check("tie", C, gate, cuda)
    tied = [t for t in M.expected("tie", C, gate)[5] if t["r"].get(3) == t["r"].get(4) and t["dropped"] == 3]
    assert gate > M.MAIN_GATE or len(tied) >= 3                      # the inputs do hold ties


@pytest.mark.parametrize("C", (4, 5, 8))
def test_infinite_gate_changes_no_byte(cuda, C):
    c = M.case("counts", C)
    views, ext, X, pruned = _run(c, float("inf"), cuda)
    assert np.array_equal(views, c.views) and np.array_equal(_bits(ext), _bits(c.ext_cost))
    assert np.array_equal(_bits(X), _bits(c.X))
    touched = M.expected("counts", C, float("inf"))[4]
    assert np.array_equal(pruned, np.where(touched, 0, SENT))


def test_wrapper_allocates_and_validates(cuda):
    c = M.case("captures5", 8)
    a = _device_args(c, cuda)
    pruned = ops_views.prune_views(*a, M.MAIN_GATE, 8)
    want = M.expected("captures5", 8, M.MAIN_GATE)
    assert pruned.dtype == torch.int32 and np.array_equal(pruned.cpu().numpy(), want[3])
    assert np.array_equal(a[0].cpu().numpy(), want[0])
    a = _device_args(c, cuda)
    out = torch.zeros(c.views.shape[0], dtype=torch.int32, device=cuda)
    for gate in (float("nan"), -1.0):
        with pytest.raises(ValueError, match="gate"):
            ops_views.prune_views(*a, gate, 8, out=out)
    with pytest.raises(ValueError, match="n_cams"):
        ops_views.prune_views(*a, 3.0, 9, out=out)
    with pytest.raises(ValueError, match="views must be"):
        ops_views.prune_views(*a, 3.0, 5, out=out)
    for k, bad in ((0, a[0].long()), (1, a[1][:-1]), (2, a[2].float()), (3, a[3][:-1]), (4, a[4].long()),
                   (6, a[6][:-1]), (7, a[7][:-1]), (5, a[5].cpu())):
        args = list(a)
        args[k] = bad.contiguous()
        with pytest.raises(ValueError):
            ops_views.prune_views(*args, 3.0, 8, out=out)
    with pytest.raises(ValueError, match="pruned"):
        ops_views.prune_views(*a, 3.0, 8, out=out[:-1])
    assert np.array_equal(a[0].cpu().numpy(), c.views) and (out == 0).all()      # nothing was launched


def _hip_runtime():
    """The HIP runtime this process has loaded (the one torch captured the
    graph with), for the graph queries torch does not wrap."""
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


def _graph_shape(graph):
    """(nodes, edges, type of the first node) of a hipGraph_t handle."""
    hip = _hip_runtime()
    handle = ctypes.c_void_p(graph)
    n_nodes, n_edges = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(n_nodes)) == 0
    assert hip.hipGraphGetEdges(handle, None, None, ctypes.byref(n_edges)) == 0
    kind = ctypes.c_int(-1)
    if n_nodes.value:
        nodes = (ctypes.c_void_p * n_nodes.value)()
        assert hip.hipGraphGetNodes(handle, nodes, ctypes.byref(n_nodes)) == 0
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[0]), ctypes.byref(kind)) == 0
    return n_nodes.value, n_edges.value, kind.value


def test_op_captures_into_a_graph(cuda):
    """The launch function enqueues one kernel and nothing else (no
    allocation, copy or sync), so the op captures into a hipGraph: the graph
    holds one node, a kernel, and no edge -- so no parallel branches --, and
    its replay gives the eager bytes."""
    c = M.case("counts", 5)
    eager = _run(c, M.MAIN_GATE, cuda)
    a = _device_args(c, cuda)
    pruned = torch.full((c.views.shape[0],), SENT, dtype=torch.int32, device=cuda)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        torch.ops.mvmatch_views.prune_views_out(*a, M.MAIN_GATE, c.C, pruned)
    assert np.array_equal(a[0].cpu().numpy(), c.views)               # captured, not run
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)             # hipGraphNodeTypeKernel == 0
    g.replay()
    torch.cuda.synchronize(cuda)
    for got, want in zip((a[0], a[1], a[2], pruned), eager):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))


# ----------------------------------------------------------- end to end ----
GATE = 3.0


def shifted_fixture(C):
    """tests/test_extend_gpu.py's eight captures with 40% of the extra views'
    detections moved by 6-12 px: still under the 30 px extension threshold,
    above the gate."""
    import test_extend_gpu as TE
    f = copy.copy(TE.fixture(C))
    f.boxes = M.shift_extra_boxes(f, seed=900 + C)
    return f


def _match(f, dev, **kw):
    from bpc_baseline_amd.inference.batch_match import match_captures
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return match_captures(t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs, n_cams=f.C, **kw)


@pytest.mark.parametrize("rig", ("host", "device"))
@pytest.mark.parametrize("C", (4, 5))
def test_match_captures_with_a_gate(cuda, C, rig):
    f = shifted_fixture(C)
    plain = _match(f, cuda, rig=rig)
    again = _match(f, cuda, rig=rig, reproj_gate=None)
    gated = _match(f, cuda, rig=rig, reproj_gate=GATE)
    assert plain.pruned is None and again.pruned is None and "pruned" not in plain.host()
    h0 = {k: getattr(plain, k).cpu().numpy() for k in ("match", "cost", "X", "views", "ext_cost", "proj")}
    h1 = {k: getattr(gated, k).cpu().numpy() for k in ("match", "cost", "X", "views", "ext_cost", "pruned")}
    want = M.prune(h0["views"], h0["ext_cost"], h0["X"], plain.offs, plain.count, plain.pts.cpu().numpy(),
                   plain.cam_offs, h0["proj"], GATE)
    w_views, w_ext, w_X, w_pruned, touched, trace = want
    # the restatement decides nothing within the margin of the gate on these inputs
    for t in trace:
        assert all(abs(q - GATE) > M.MARGIN for q in t["r"].values())
    # reproj_gate=None is the ungated run, byte for byte; the seeds, costs, order and counts never change
    for k in ("count", "offs", "cam_offs"):
        assert np.array_equal(getattr(plain, k), getattr(again, k)) and np.array_equal(getattr(plain, k),
                                                                                       getattr(gated, k))
    for k in ("match", "cost", "X", "views", "ext_cost"):
        assert np.array_equal(_bits(h0[k][touched]), _bits(getattr(again, k).cpu().numpy()[touched])), k
    assert np.array_equal(h1["match"][touched], h0["match"][touched])
    assert np.array_equal(_bits(h1["cost"][touched]), _bits(h0["cost"][touched]))
    assert np.array_equal(h1["views"][touched][:, :3], h0["views"][touched][:, :3])
    # the gated run is the restatement applied to the ungated one
    assert np.array_equal(h1["views"][touched], w_views[touched])
    assert np.array_equal(_bits(h1["ext_cost"][touched]), _bits(w_ext[touched]))
    assert np.array_equal(h1["pruned"], w_pruned) and gated.host()["pruned"] is not None
    same = touched & (w_pruned == 0)
    assert np.array_equal(_bits(h1["X"][same]), _bits(h0["X"][same]))
    np.testing.assert_allclose(h1["X"][touched], w_X[touched], rtol=M.RTOL, atol=M.ATOL)
    # the table of the gated batch holds no extra view above the gate
    tab = gated.table(reproj=True)
    rep, v = tab.reproj.cpu().numpy()[:, 3:], tab.views.cpu().numpy()[:, 3:]
    assert np.array_equal(np.isnan(rep), v < 0) and (rep[v >= 0] <= GATE).all()
    assert (w_pruned[touched] != 0).sum() >= 3 and (v >= 0).any(axis=1).sum() >= 3


def test_three_cameras_accept_the_gate(cuda):
    import test_extend_gpu as TE
    from bpc_baseline_amd.inference.batch_match import match_captures
    b3 = TE.three_cam_inputs(TE.fixture(4))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    a = match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5])
    b = match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5], reproj_gate=GATE)
    assert a.pruned is None and b.pruned.dtype == torch.int32 and b.pruned.shape[0] == b.match.shape[0]
    assert not b.pruned.any() and b.views is None and np.array_equal(a.count, b.count)
    for s in range(len(a.count)):
        sl = slice(int(a.offs[s]), int(a.offs[s]) + int(a.count[s]))
        assert torch.equal(a.match[sl], b.match[sl]) and torch.equal(a.X[sl], b.X[sl])
    for gate in (float("nan"), -1):
        with pytest.raises(ValueError, match="gate"):
            match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5], reproj_gate=gate)


def test_stream_passes_the_gate_through(cuda):
    from bpc_baseline_amd.inference.batch_match import match_capture_stream
    f = shifted_fixture(4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    batch = (t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs)
    one = _match(f, cuda, reproj_gate=GATE)
    got, = list(match_capture_stream([batch], n_cams=4, reproj_gate=GATE))
    assert torch.equal(got.pruned, one.pruned) and bool(got.pruned.any())
