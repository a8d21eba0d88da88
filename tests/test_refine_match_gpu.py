"""match_captures(refine=...) end to end on the GPU: the
refinement at the end of every pass, on §3.14's eight captures (extra-view
detections moved as in tests/test_view_prune_gpu.py, so a gate has views to
drop) and on their first three cameras as a three-camera batch.

The run with the keyword is the run without it, byte for byte, in every field
that existed before (``X_dlt`` holding its ``X``), and ``X`` / ``refine_rms`` /
``refine_info`` / ``cov`` are tests/refine_model.py applied to that run, bit
for bit (a NaN standing for any NaN)."""
import numpy as np
import pytest
import torch

import refine_model as M
from test_view_prune_gpu import shifted_fixture

pytestmark = pytest.mark.gpu
OLD_FIELDS = ("match", "cost", "views", "ext_cost", "pruned", "pts", "boxes", "proj", "orig")
NEW_FIELDS = ("X_dlt", "refine_rms", "refine_info", "cov")


def _inputs(C, dev):
    """-> (positional arguments of match_captures, keywords)."""
    import test_extend_gpu as TE
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if C == 3:
        b3 = TE.three_cam_inputs(TE.fixture(4))
        return (t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5]), {}
    f = shifted_fixture(C)
    return (t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs), dict(n_cams=C)


def _rows(b):
    return np.concatenate([np.arange(o, o + n) for o, n in zip(b.offs[:-1], b.count)]
                          + [np.zeros(0, np.int64)]).astype(np.int64)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _check_pass(plain, ref, max_evals=10):
    """One pass of the run with the keyword against the same pass without."""
    rows = _rows(plain)
    for k in ("count", "offs", "cam_offs", "n_cams", "cam_order"):
        assert np.array_equal(getattr(plain, k), getattr(ref, k)), k
    for k in OLD_FIELDS:
        a, b = getattr(plain, k), getattr(ref, k)
        assert (a is None) == (b is None), k
        if a is not None:
            a, b = _np(a), _np(b)
            full = k in ("pts", "boxes", "proj", "orig")
            assert M.same(a if full else a[rows], b if full else b[rows]), k
    assert all(getattr(plain, k) is None for k in NEW_FIELDS)
    X0 = _np(plain.X)
    assert M.same(_np(ref.X_dlt)[rows], X0[rows])
    views = _np(plain.views if plain.n_cams > 3 else plain.match)
    S, C = plain.count.size, plain.n_cams
    want = M.refine(views, X0, plain.offs, plain.count, _np(plain.pts), plain.cam_offs,
                    _np(plain.proj).reshape(S, C, 3, 4), max_evals)
    for k, w in zip(("X", "refine_rms", "refine_info", "cov"), want):
        assert M.same(_np(getattr(ref, k))[rows], w[rows]), k
    h = ref.host()
    assert all(k in h for k in NEW_FIELDS) and not any(k in plain.host() for k in NEW_FIELDS)
    return rows, want


def _check_table(plain, ref, rows, want):
    """table(reproj=True) carries the refined X, and a row's summed squared
    reprojection error did not rise (model values: no tolerance)."""
    t0, t1 = plain.table(reproj=True), ref.table(reproj=True)
    assert M.same(_np(t1.X), want[0][rows]) and M.same(_np(t0.X), _np(plain.X)[rows])
    rms = want[1][rows]
    assert not (rms[:, 1] > rms[:, 0]).any()
    n = _np(t1.n_views).astype(np.float64)
    for tab, col in ((t0, 0), (t1, 1)):
        np.testing.assert_allclose(np.nansum(_np(tab.reproj) ** 2, axis=1), n * rms[:, col] ** 2, rtol=1e-12,
                                   atol=1e-18)


@pytest.mark.parametrize("gate", (None, 3.0))
@pytest.mark.parametrize("rig", ("host", "device"))
@pytest.mark.parametrize("C", (3, 4, 5))
def test_match_captures_refines_every_match(cuda, C, rig, gate):
    from bpc_baseline_amd.inference.batch_match import match_captures
    args, kw = _inputs(C, cuda)
    kw = dict(kw, rig=rig, reproj_gate=gate)
    plain = match_captures(*args, **kw)
    ref = match_captures(*args, refine=True, **kw)
    rows, want = _check_pass(plain, ref)
    _check_table(plain, ref, rows, want)
    st = want[2][rows, 0]
    assert rows.size >= 20 and (st == M.CONVERGED).sum() >= 10 and (want[2][rows, 1] > 0).sum() >= 10
    if C > 3:
        k = (_np(plain.views)[rows] >= 0).sum(axis=1)
        assert (k > 3).sum() >= 3                     # rows refined over more than the seed views
    # refine=None is the call without the keyword, byte for byte
    again = match_captures(*args, refine=None, **kw)
    for k in ("match", "cost", "X") + (("views", "ext_cost") if C > 3 else ()):
        assert M.same(_np(getattr(again, k))[rows], _np(getattr(plain, k))[rows]), k
    assert all(getattr(again, k) is None for k in NEW_FIELDS)


def test_every_seed_pass_is_refined(cuda):
    from bpc_baseline_amd.inference.batch_match import match_captures
    args, kw = _inputs(5, cuda)
    kw = dict(kw, extra_seeds=[(2, 3, 4)], reproj_gate=3.0)
    plain = match_captures(*args, **kw)
    ref = match_captures(*args, refine=4, **kw)
    assert len(plain.passes) == len(ref.passes) == 1
    total = 0
    for p, r in zip((plain,) + plain.passes, (ref,) + ref.passes):
        rows, want = _check_pass(p, r, max_evals=4)
        total += rows.size
        assert rows.size >= 1
    assert int(ref.table_all().X.shape[0]) == total               # the merged table carries every pass


@pytest.mark.parametrize("bad", (0, 65, "x", False, 2.5))
def test_a_bad_keyword_raises(cuda, bad):
    from bpc_baseline_amd.inference.batch_match import match_captures
    args, kw = _inputs(3, cuda)
    with pytest.raises(ValueError, match="refine"):
        match_captures(*args, refine=bad, **kw)


def test_stream_passes_the_keyword_through(cuda):
    from bpc_baseline_amd.inference.batch_match import match_capture_stream, match_captures
    for C in (3, 4):
        args, kw = _inputs(C, cuda)
        one = match_captures(*args, refine=True, **kw)
        got, = list(match_capture_stream([args], refine=True, **kw))
        rows = _rows(one)
        for k in ("X",) + NEW_FIELDS:
            assert M.same(_np(getattr(got, k))[rows], _np(getattr(one, k))[rows]), k
        assert (_np(one.refine_info)[rows, 1] > 0).any()
