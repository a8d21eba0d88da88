"""The point refinement on the GPU where its descent rejects, stalls and fails
(DESIGN §3.17): the inputs of tests/refine_edges.py -- far starts, the origin,
camera centres, twin cameras, failing second and third pivots, power-of-two
scaled rigs, and all of them side by side in one wave -- against
tests/refine_model.py bit for bit, with the checks of tests/test_refine_gpu.py:
every output pre-filled with sentinels and compared whole, the inputs
unchanged.  tests/test_refine_edges_model.py pins on the CPU that these inputs
reach the branches they are there for."""
import numpy as np
import pytest
import torch

import refine_edges as E
import refine_model as M
from bpc_baseline_amd import ops_views
from test_refine_gpu import _check, _device_args, _fill, _graph_shape, _host, _run

pytestmark = pytest.mark.gpu
MATCH_GATE = 1e3          # px: keeps every extra view the extension admits, the wrong ones too


@pytest.mark.parametrize("max_evals", M.MAX_EVALS)
@pytest.mark.parametrize("C", M.CAMS)
@pytest.mark.parametrize("name", E.NAMES)
def test_every_edge_input(cuda, name, C, max_evals):
    c, want = _check(name, C, max_evals, cuda)
    assert c.rows().size >= 17 and c.S <= 6 and int(c.count.max()) <= 257


@pytest.mark.parametrize("C", (3, 8))
def test_mixed_without_the_covariance(cuda, C):
    _check("mixed", C, 64, cuda, cov=False)


@pytest.mark.parametrize("C", (4, 8))
def test_mixed_through_the_wrapper(cuda, C):
    c = M.case("mixed", C)
    got = ops_views.refine_points(*_device_args(c, cuda), C, max_evals=64)
    want = M.expected("mixed", C, 64)
    rows = c.rows()
    for k, g, w in zip(("X_out", "rms", "info", "cov"), got, want):
        assert M.same(g.cpu().numpy()[rows], w[rows]), k
    other = np.setdiff1d(np.arange(c.views.shape[0]), rows)
    assert len(other) and (got[2].cpu().numpy()[other] == (3, 0)).all() and np.isnan(got[0].cpu().numpy()[other]).all()


def test_mixed_captures_into_a_graph(cuda):
    """One kernel node and no edge on the long-running input too, and the
    replay gives the model's bits."""
    c = M.case("mixed", 5)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    a, outs = _run(c, 64, cuda, graph=g)
    fill = _fill(c.views.shape[0])
    assert all(M.same(t.cpu().numpy(), f) for t, f in zip(outs, fill))         # captured, not run
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)
    g.replay()
    torch.cuda.synchronize(cuda)
    want = M.refine(*c.args(), 64, fill=fill)
    for k, got, w in zip(("X_out", "rms", "info", "cov"), _host(outs), want):
        assert M.same(got, w), k


def test_match_captures_refines_matches_with_a_wrong_view(cuda):
    """match_captures(refine=64) behind a gate that keeps wrong extra views:
    some rows then start far from their minimum (checked on the model's trace:
    more than 10 evaluations, or three rejections in a row), and ``X``,
    ``refine_rms``, ``refine_info`` and ``cov`` are the model on the same
    views, bit for bit."""
    from bpc_baseline_amd.inference.batch_match import match_captures
    from test_refine_match_gpu import _inputs, _np, _rows
    args, kw = _inputs(5, cuda)
    ref = match_captures(*args, refine=64, reproj_gate=MATCH_GATE, **kw)
    rows = _rows(ref)
    S, C = ref.count.size, ref.n_cams
    traces = {}
    want = M.refine(_np(ref.views), _np(ref.X_dlt), ref.offs, ref.count, _np(ref.pts), ref.cam_offs,
                    _np(ref.proj).reshape(S, C, 3, 4), 64, traces=traces)
    hard = sum(1 for t in traces.values() if t["evals"] > 10 or t["longest_run"] >= 3)
    print(f"{rows.size} matches, {hard} with more than 10 evaluations or three rejections in a row")
    assert hard >= 3
    for k, w in zip(("X", "refine_rms", "refine_info", "cov"), want):
        assert M.same(_np(getattr(ref, k))[rows], w[rows]), k
