"""Refinement of triangulated points on the GPU (mvm_refine_points,
ops_views.refine_points) against the statement of
tests/refine_model.py, bit for bit.

The op is called directly on the builders' inputs with every output pre-filled
with a sentinel, and the outputs are compared whole: the rows at and beyond
each capture's count, and unused capacity, keep the fill.  The arithmetic is
+ - x / sqrt in a stated order with contraction off, so ``X_out``, ``rms``,
``info`` and ``cov`` must carry the model's bits (a NaN standing for any NaN:
its sign and payload are the hardware's); a differing bit means a contraction
or another order."""
import ctypes

import numpy as np
import pytest
import torch

import refine_model as M
from bpc_baseline_amd import ops_views       # registers torch.ops.mvmatch_views.*

pytestmark = pytest.mark.gpu
SENT_F = -12345.678125           # what the f64 outputs hold before the op
SENT_I = M.I32_MIN + 7           # and info


def _fill(cap):
    return (np.full((cap, 3), SENT_F), np.full((cap, 2), SENT_F), np.full((cap, 2), SENT_I, np.int32),
            np.full((cap, 6), SENT_F))


def _device_args(c, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in c.args()]


def _run(c, max_evals, dev, cov=True, graph=None):
    """The op on the case's arrays -> (X_out, rms, info, cov | None) on the
    host; the inputs are checked to be what they were."""
    a = _device_args(c, dev)
    outs = [torch.from_numpy(f).to(dev) for f in _fill(c.views.shape[0])]
    if not cov:
        outs[3] = None
    call = lambda: torch.ops.mvmatch_views.refine_points_out(*a, c.C, max_evals, *outs)
    if graph is None:
        call()
    else:
        with torch.cuda.graph(graph):
            call()
    return a, outs


def _host(outs):
    return [None if t is None else t.cpu().numpy() for t in outs]


def _differing_rows(g, w):
    eq = M.bits(g) == M.bits(w)
    if g.dtype.kind == "f":
        eq |= np.isnan(g) & np.isnan(w)
    return np.nonzero(~eq.reshape(len(g), -1).all(axis=1))[0][:8].tolist()


def _check(name, C, max_evals, dev, cov=True):
    c = M.case(name, C)
    a, outs = _run(c, max_evals, dev, cov)
    got = _host(outs)
    want = M.refine(*c.args(), max_evals, fill=_fill(c.views.shape[0]))
    for k, g, w in zip(("X_out", "rms", "info", "cov"), got, want):
        if g is not None:
            assert M.same(g, w), (k, _differing_rows(g, w))
    assert M.same(a[0].cpu().numpy(), c.views) and M.same(a[1].cpu().numpy(), c.X)      # the inputs stand
    return c, want


@pytest.mark.parametrize("max_evals", M.MAX_EVALS)
@pytest.mark.parametrize("C", M.CAMS)
def test_counts_at_the_waves_edges(cuda, C, max_evals):
    """Captures of 3, 0, 1, 63, 64, 65, 257 and 7 matches (an empty capture
    between full ones, count = capacity), under every cap of the evaluations."""
    c, want = _check("counts", C, max_evals, cuda)
    rows = c.rows()
    st = want[2][rows, 0]
    assert (st == M.CONVERGED).sum() >= 3 and ((st == M.CAPPED).sum() >= 3) == (max_evals <= 2)
    assert ((want[2][rows, 1] == 0) & (st == M.CONVERGED)).sum() >= 3          # exact projections


@pytest.mark.parametrize("S", (1, 4, 5, 1025))
@pytest.mark.parametrize("C", (3, 8))
def test_capture_counts_at_workgroup_edges(cuda, C, S):
    """Four captures per workgroup: a part of one, exactly one, one more, and
    several workgroups with a tail."""
    c, want = _check(f"captures{S}", C, 10, cuda)
    assert (want[2][c.rows(), 0] <= M.CAPPED).all()


@pytest.mark.parametrize("C", M.CAMS)
def test_every_regime(cuda, C):
    """A P with a zero third row (the cost is not finite), P with zero first
    three columns (A = 0: no pivot), rows with an index outside its view and
    rows of one view (skipped), beside converging rows."""
    c, want = _check("regimes", C, 10, cuda)
    rows = c.rows()
    st, kind = want[2][rows, 0], c.kind[rows]
    assert (st[kind == "zero3"] == M.FAILED).all() and (kind == "zero3").sum() >= 3
    assert (st[kind == "azero"] == M.FAILED).all() and (kind == "azero").sum() >= 3
    assert (st[kind == "skip"] == M.SKIPPED).all() and (kind == "skip").sum() >= 6
    assert (st == M.CONVERGED).sum() >= 3


@pytest.mark.parametrize("C", (3, 5))
def test_without_the_covariance(cuda, C):
    c, want = _check("counts", C, 10, cuda, cov=False)


def test_wrapper_allocates_and_validates(cuda):
    c = M.case("captures5", 8)
    a = _device_args(c, cuda)
    X_out, rms, info, cov = ops_views.refine_points(*a, 8)
    want = M.expected("captures5", 8)
    rows = c.rows()
    for g, w in zip((X_out, rms, info, cov), want):
        assert M.same(g.cpu().numpy()[rows], w[rows])
    other = np.setdiff1d(np.arange(c.views.shape[0]), rows)
    assert np.isnan(X_out.cpu().numpy()[other]).all() and (info.cpu().numpy()[other] == (3, 0)).all()
    assert ops_views.refine_points(*a, 8, max_evals=3, cov=False)[3] is None
    for bad in (0, 65, True, 2.0, "x"):
        with pytest.raises(ValueError, match="max_evals"):
            ops_views.refine_points(*a, 8, max_evals=bad)
    with pytest.raises(ValueError, match="n_cams"):
        ops_views.refine_points(*a, 9)
    with pytest.raises(ValueError, match="views must be"):
        ops_views.refine_points(*a, 5)
    for k, bad in ((0, a[0].long()), (1, a[1][:-1]), (1, a[1].float()), (2, a[2][:-1]), (3, a[3].long()),
                   (5, a[5][:-1]), (6, a[6][:-1]), (4, a[4].cpu())):
        args = list(a)
        args[k] = bad.contiguous()
        with pytest.raises(ValueError):
            ops_views.refine_points(*args, 8)
    outs = [torch.from_numpy(f).to(cuda) for f in _fill(c.views.shape[0])]
    for k, name in enumerate(("X_out", "rms", "info", "cov")):
        short = list(outs)
        short[k] = outs[k][:-1]
        with pytest.raises(ValueError, match=name):
            torch.ops.mvmatch_views.refine_points_out(*a, 8, 10, *short)
    with pytest.raises(ValueError, match="X_out"):
        torch.ops.mvmatch_views.refine_points_out(*a, 8, 10, a[1], *outs[1:])
    assert all(M.same(t.cpu().numpy(), f) for t, f in zip(outs, _fill(c.views.shape[0])))   # nothing launched


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
    allocation, copy or sync), so the op captures into a hipGraph of one node,
    a kernel, and no edge, and its replay gives the eager bytes."""
    c = M.case("counts", 5)
    eager = _host(_run(c, 10, cuda)[1])
    g = torch.cuda.CUDAGraph(keep_graph=True)
    a, outs = _run(c, 10, cuda, graph=g)
    assert all(M.same(t.cpu().numpy(), f) for t, f in zip(outs, _fill(c.views.shape[0])))   # captured, not run
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)             # hipGraphNodeTypeKernel == 0
    g.replay()
    torch.cuda.synchronize(cuda)
    for got, want in zip(_host(outs), eager):
        assert M.same(got, want)
