"""The box fit on the GPU (mvm_fit_boxes, ops_views.fit_boxes)
against the statement of tests/box_fit_model.py, bit for bit.

The op is called directly on the builders' inputs with every output pre-filled
with a sentinel and a guard row before and behind the rows it may write; the
outputs are compared whole, guards included.  The arithmetic is + - x / sqrt in
a stated order with contraction off, and the only cross-lane operations are
minima, so every output must carry the model's bits (a NaN standing for any
NaN); a differing bit means a contraction, another order or a wrong tie-break.
No comparison here has a tolerance."""
import numpy as np
import pytest
import torch

import box_fit_inputs as I
import box_fit_model as M
from bpc_baseline_amd import ops_views       # registers torch.ops.mvmatch_views.*
from test_crop_gpu import _graph_shape

pytestmark = pytest.mark.gpu
SENT_F = -12345.678125           # what the f64 outputs hold before the op
SENT_I = M.I32_MIN + 7           # and info
KEYS = ("pose", "rms", "info", "cov", "resid")


def _fill(n, C):
    return dict(pose=np.full((n, 4, 4), SENT_F), rms=np.full((n, 2), SENT_F),
                info=np.full((n, 2), SENT_I, np.int32), cov=np.full((n, 6), SENT_F),
                resid=np.full((n, C, 4), SENT_F))


def _run(c, max_evals, dev, cov=True, resid=True, graph=None, scene_base=0):
    """The op on the case's arrays, writing rows 1 .. n of outputs of n + 2
    rows -> (device inputs, guarded device outputs)."""
    n = len(c.scene)
    a = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in c.args()]
    outs = {k: torch.from_numpy(v).to(dev) for k, v in _fill(n + 2, c.C).items()}
    inner = {k: (v[1:n + 1] if (k != "cov" or cov) and (k != "resid" or resid) else None) for k, v in outs.items()}
    call = lambda: torch.ops.mvmatch_views.fit_boxes_out(*a, c.C, scene_base, max_evals, *(inner[k] for k in KEYS))
    if graph is None:
        call()
    else:
        with torch.cuda.graph(graph):
            call()
    return a, outs


def _differing_rows(g, w):
    eq = M.bits(g) == M.bits(w)
    if g.dtype.kind == "f":
        eq |= np.isnan(g) & np.isnan(w)
    return np.nonzero(~eq.reshape(len(g), -1).all(axis=1))[0][:8].tolist()


def _want(c, max_evals, cov=True, resid=True, scene_base=0):
    n = len(c.scene)
    want = _fill(n + 2, c.C)
    inner = M.fit_boxes(*c.args(), max_evals, scene_base=scene_base)
    for k in KEYS:
        if (k != "cov" or cov) and (k != "resid" or resid):
            want[k][1:n + 1] = inner[k]
    return want


def _check(c, max_evals, dev, **kw):
    a, outs = _run(c, max_evals, dev, **kw)
    want = _want(c, max_evals, **kw)
    for k in KEYS:
        g = outs[k].cpu().numpy()
        assert M.same(g, want[k]), (k, _differing_rows(g, want[k]))
    for t, x in zip(a, c.args()):                     # the inputs stand
        assert M.same(t.cpu().numpy(), np.ascontiguousarray(x))
    return want


@pytest.mark.parametrize("V", I.VERTS)
@pytest.mark.parametrize("C", I.CAMS)
def test_vertex_counts_at_the_lanes_edges(cuda, C, V):
    """One vertex, two, a lane short of the wave, the wave, one more, two
    strides and one more, sixteen strides: idle lanes and lane striding."""
    want = _check(I.case(f"verts{V}", C), 10, cuda)
    assert (want["info"][1:-1, 0] <= M.CAPPED).all()


@pytest.mark.parametrize("n", I.ROWS)
@pytest.mark.parametrize("C", (3, 8))
def test_row_counts_at_the_workgroups_edge(cuda, C, n):
    """Four rows per workgroup: a part of one, exactly one, one more, many with a tail."""
    _check(I.case(f"rows{n}", C), 10, cuda)


@pytest.mark.parametrize("max_evals", I.MAX_EVALS)
@pytest.mark.parametrize("C", I.CAMS)
def test_every_regime(cuda, C, max_evals):
    """Vertices behind a camera at the start and at a trial point only, a
    failed pivot, rows without a view or a capture, capped rows and restarts
    (tests/test_box_fit_model.py counts each), under every cap."""
    c = I.case("regimes", C)
    want = _check(c, max_evals, cuda)
    st = want["info"][1:-1, 0]
    assert {M.CONVERGED if max_evals > 2 else M.CAPPED, M.FAILED, M.SKIPPED} <= set(st.tolist())
    _check(I.case("restart", C), max_evals, cuda)


@pytest.mark.parametrize("swap", (False, True))
def test_tie_keeps_the_lowest_vertex(cuda, swap):
    _check(I.tie_case(swap), 10, cuda)


@pytest.mark.parametrize("name", ("last64", "last65", "last129", "stride2"))
def test_extremes_on_the_last_vertex_and_in_a_second_stride(cuda, name):
    _check(I.case(name, 3 if name.startswith("last") else 4), 10, cuda)


@pytest.mark.parametrize("cov, resid", ((False, True), (True, False), (False, False)))
def test_without_the_optional_outputs(cuda, cov, resid):
    _check(I.case("regimes", 4), 10, cuda, cov=cov, resid=resid)


def test_scene_base(cuda):
    c = I.case("rows5", 3)
    want = _check(c, 10, cuda, scene_base=1)          # capture 0's rows fall below the first capture
    assert (want["info"][1:-1, 0] == M.SKIPPED).sum() == (c.scene == 0).sum() > 0


def test_wrapper_allocates_and_validates(cuda):
    c = I.case("regimes", 4)
    n = len(c.scene)
    a = [torch.from_numpy(np.ascontiguousarray(x)).to(cuda) for x in c.args()]
    pose, scene, views, boxes, proj, verts = a
    want = I.expected("regimes", 4)[0]
    fit = ops_views.fit_boxes(pose, scene, views, boxes, c.proj, 4, c.verts)         # host rig and vertices
    for k in KEYS:
        assert M.same(getattr(fit, k).cpu().numpy(), want[k]), k
    part = ops_views.fit_boxes(pose[3:n - 2].contiguous(), scene, views, boxes, proj, 4, verts, rows=(3, n - 2),
                               max_evals=2, cov=False, resid=False)
    w2 = I.expected("regimes", 4, 2)[0]
    assert part.cov is None and part.resid is None
    for k in ("pose", "rms", "info"):
        assert M.same(getattr(part, k).cpu().numpy(), w2[k][3:n - 2]), k
    empty = ops_views.fit_boxes(pose[:0], scene, views, boxes, proj, 4, verts, rows=(2, 2))
    assert empty.pose.shape == (0, 4, 4) and empty.resid.shape == (0, 4, 4)
    for bad in (0, 65, True, 2.0, "x"):
        with pytest.raises(ValueError, match="max_evals"):
            ops_views.fit_boxes(pose, scene, views, boxes, proj, 4, verts, max_evals=bad)
    for kw in (dict(rows=(0, n + 1)), dict(rows=(2, 1)), dict(rows=3)):
        with pytest.raises(ValueError, match="rows"):
            ops_views.fit_boxes(pose, scene, views, boxes, proj, 4, verts, **kw)
    with pytest.raises(ValueError, match="pose must be"):
        ops_views.fit_boxes(pose[:-1], scene, views, boxes, proj, 4, verts)
    with pytest.raises(ValueError, match="views must be"):
        ops_views.fit_boxes(pose, scene, views, boxes, proj, 5, verts)
    for bad_cams in (2, 9):
        with pytest.raises(ValueError, match="n_cams"):
            torch.ops.mvmatch_views.fit_boxes_out(*a, bad_cams, 0, 10,
                                                  *(torch.from_numpy(v).to(cuda) for v in _fill(n, 4).values()))
    with pytest.raises(ValueError, match="boxes must be"):
        ops_views.fit_boxes(pose, scene, views, boxes[:, :, :3], proj, 4, verts)
    with pytest.raises(ValueError, match="proj"):
        ops_views.fit_boxes(pose, scene, views, boxes, proj[:, :3], 4, verts)
    with pytest.raises(ValueError, match="proj holds no capture"):
        ops_views.fit_boxes(pose, scene, views, boxes, proj[:0], 4, verts)
    with pytest.raises(ValueError, match="verts"):
        ops_views.fit_boxes(pose, scene, views, boxes, proj, 4, np.zeros((0, 3)))
    for k, badt in ((0, pose.float()), (1, scene.long()), (2, views.long()), (3, boxes.long()), (4, proj.float()),
                    (5, verts.float()), (1, scene.cpu())):
        args = list(a)
        args[k] = badt
        with pytest.raises(ValueError):
            ops_views.fit_boxes(*args[:5], 4, args[5])
    outs = {k: torch.from_numpy(v).to(cuda) for k, v in _fill(n, 4).items()}
    for k in KEYS:
        short = dict(outs)
        short[k] = outs[k][:-1]
        with pytest.raises(ValueError, match="pose_out" if k == "pose" else k):
            torch.ops.mvmatch_views.fit_boxes_out(*a, 4, 0, 10, *(short[q] for q in KEYS))
    with pytest.raises(ValueError, match="pose_out"):
        torch.ops.mvmatch_views.fit_boxes_out(*a, 4, 0, 10, pose, *(outs[q] for q in KEYS[1:]))
    assert all(M.same(outs[k].cpu().numpy(), v) for k, v in _fill(n, 4).items())      # nothing launched
    # the C entry point refuses an overlap that is no identity; back to back is none
    both = torch.cat([pose, torch.full_like(pose, SENT_F)])
    with pytest.raises(Exception, match="overlaps"):
        torch.ops.mvmatch_views.fit_boxes_out(both[:n], *a[1:], 4, 0, 10, both[1:n + 1], *(outs[q] for q in KEYS[1:]))
    torch.ops.mvmatch_views.fit_boxes_out(both[:n], *a[1:], 4, 0, 10, both[n:], *(outs[q] for q in KEYS[1:]))
    assert M.same(both[n:].cpu().numpy(), want["pose"]) and M.same(both[:n].cpu().numpy(), c.pose)


def test_op_captures_into_a_graph(cuda):
    """The launch function enqueues one kernel and nothing else (no
    allocation, copy or sync), so the op captures into a hipGraph of one node,
    a kernel, and no edge, and its replay gives the eager bytes."""
    c = I.case("regimes", 8)
    eager = {k: v.cpu().numpy() for k, v in _run(c, 10, cuda)[1].items()}
    g = torch.cuda.CUDAGraph(keep_graph=True)
    a, outs = _run(c, 10, cuda, graph=g)
    fill = _fill(len(c.scene) + 2, 8)
    assert all(M.same(outs[k].cpu().numpy(), fill[k]) for k in KEYS)                  # captured, not run
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)             # hipGraphNodeTypeKernel == 0
    g.replay()
    torch.cuda.synchronize(cuda)
    for k in KEYS:
        assert M.same(outs[k].cpu().numpy(), eager[k]), k
