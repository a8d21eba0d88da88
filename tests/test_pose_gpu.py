"""From the rotation head's outputs to poses on the GPU (mvm_fuse_rotations,
ops_views.fuse_rotations) against tests/pose_model.py.

The op writes into slices of sentinel-filled outputs with a guard row on either
side; every output is compared whole and bit for bit with the model (NaN equal
to NaN), the guards with the sentinel, and the inputs with what was uploaded."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import pose_model as M
from bpc_baseline_amd import ops_views       # registers torch.ops.mvmatch_views.*
from bpc_baseline_amd.synth import make_rig
from test_crop_gpu import _graph_shape

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -777.0, -12345
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "rot_decode.npz"))
OUTS = (("rot_views", (3, 3), torch.float64, True), ("R", (3, 3), torch.float64, False),
        ("pose", (4, 4), torch.float64, False), ("spread", (), torch.float64, True),
        ("slot_status", (), torch.int32, True), ("row_status", (), torch.int32, False))


def special_raw(mode):
    """The raw vectors every case holds besides the random ones."""
    D = M.MODES[mode][1]
    n_edge = int(GOLDEN[f"{mode}_n_edge"])
    rows = [GOLDEN[f"{mode}_raw"][-n_edge:], np.zeros((1, D), np.float32)]
    for bad in (np.nan, np.inf, -np.inf):
        v = np.ones((D, D), np.float32) * np.float32(0.25)
        v[np.arange(D), np.arange(D)] = bad                      # one bad component at a time
        rows.append(v)
    if mode == "6d":                                              # below the 1e-8 clamp, denormals among them
        tiny = np.array([[1e-39, 2e-40, -3e-41, 1, 2, 3], [1e-9, -2e-9, 3e-9, 1e-41, 1e-39, -1e-40],
                         [1e-45, 0, 0, 0, 1e-45, 0], [3e-9, 1e-9, 2e-9, 3e-9, 1e-9, 2.5e-9],
                         [1, 2, 3, 1e-40, 2e-40, 3e-40]], np.float32)
        rows.append(tiny)
    if mode == "quat":
        rows.append(np.array([[1e-39, 2e-40, 0, 1e-41], [1e-30, 1e-30, 1e-30, 1e-30]], np.float32))
    return np.concatenate(rows).astype(np.float32)


class Case:
    """A hand-built table of n rows over S captures of C cameras with random
    raw vectors for every (row, camera); the special vectors go through the
    slots in order.  Some views are -1, row ``bad[0]`` has a scene id past the
    rig's captures, ``bad[1]`` one below ``scene_base``, ``bad[2]`` no view."""

    def __init__(self, n, C, mode, S=3, scene_base=0, seed=0):
        rng = np.random.default_rng(100 * n + 10 * C + M.MODES[mode][0] + seed)
        self.n, self.C, self.S, self.mode, self.scene_base = n, C, S, mode, scene_base
        D = M.MODES[mode][1]
        self.raw = M.random_raw(rng, n * C, mode).reshape(n, C, D)
        sp = special_raw(mode)
        flat = self.raw.reshape(n * C, D)
        at = np.arange(len(sp)) * 2 % (n * C)                     # every other slot, wrapping in a small table
        flat[at] = sp
        if mode == "euler":
            finite = np.isfinite(flat).all(axis=1)
            assert M.euler_filter(flat[finite]).all()
        self.views = rng.integers(0, 40, (n, C)).astype(np.int32)
        self.views[rng.random((n, C)) < 0.2] = -1
        self.views[0] = 0                                         # the first row keeps every view
        self.scene = (np.arange(n) % S + scene_base).astype(np.int32)
        self.bad = ()
        if n >= 5:
            self.bad = (n - 3, n - 1, n - 2)
            self.scene[n - 3], self.scene[n - 1] = S + scene_base, scene_base - 1
            self.views[n - 2] = -1
        self.X = rng.uniform(-300, 300, (n, 3))
        self.RTs = np.stack([np.stack(make_rig(rng, C)[1]) for _ in range(S)]).astype(np.float64)

    def device(self, dev):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t(self.scene), t(self.views), t(self.X), t(self.RTs)


@lru_cache(maxsize=None)
def case(*a, **kw):
    return Case(*a, **kw)


def run_op(c, dev, rows, cams, fuse, cam=2, omit=()):
    """The op on a fresh upload -> dict of the outputs on the host, after
    checking the guards and that no input changed."""
    b, e = rows
    m, K = e - b, len(cams)
    raw = torch.from_numpy(np.ascontiguousarray(c.raw[b:e][:, list(cams)])).to(dev)
    args = c.device(dev)
    keep = [a.clone() for a in (raw,) + args]
    bufs = {}
    for name, tail, dt, per_slot in OUTS:
        shape = (m + 2,) + ((K,) if per_slot else ()) + tail
        bufs[name] = torch.full(shape, SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=dev)
    out = {k: (None if k in omit else v[1:m + 1]) for k, v in bufs.items()}
    torch.ops.mvmatch_views.fuse_rotations_out(raw, *args, c.C, c.scene_base, b, m, list(cams), c.mode, fuse, cam,
                                               out["rot_views"], out["R"], out["pose"], out["spread"],
                                               out["slot_status"], out["row_status"])
    torch.cuda.synchronize(dev)
    for got, was in zip((raw,) + args, keep):
        assert bool(((got == was) | ((got != got) & (was != was))).all())     # NaN stays NaN
    for name, _, dt, _ in OUTS:
        sent = SENT_I if dt == torch.int32 else SENT_F
        assert (bufs[name][0] == sent).all() and (bufs[name][-1] == sent).all(), name
        if name in omit:
            assert (bufs[name] == sent).all(), name
    return {k: v[1:m + 1].cpu().numpy() for k, v in bufs.items() if k not in omit}


def expected(c, rows, cams, fuse, cam=2):
    b, e = rows
    return M.fuse_rotations(c.raw[b:e][:, list(cams)], c.scene, c.views, c.X, c.RTs, c.mode, rows=rows,
                            cams=list(cams), fuse=fuse, cam=cam, scene_base=c.scene_base)


def check(c, dev, rows, cams, fuse, cam=2, omit=()):
    got, want = run_op(c, dev, rows, cams, fuse, cam, omit), expected(c, rows, cams, fuse, cam)
    for k, v in got.items():
        assert M.same(v, want[k]), (k, np.argwhere(~((v == want[k]) | ((v != v) & (want[k] != want[k]))))[:5])
    M.invariants(got)
    return want


@pytest.mark.parametrize("fuse", ("cam", "mean"))
@pytest.mark.parametrize("mode", ("euler", "quat", "6d"))
@pytest.mark.parametrize("C", (3, 4, 8))
@pytest.mark.parametrize("n", (1, 5, 257, 513))
def test_rows_cameras_modes_and_fusions(cuda, n, C, mode, fuse):
    c = case(n, C, mode)
    want = check(c, cuda, (0, n), range(C), fuse)
    if n >= 257:
        assert {0, M.NO_VIEW, M.NO_CAPTURE, M.DEGENERATE} == set(want["slot_status"].reshape(-1))
        assert {0, M.NO_ROTATION} <= set(want["row_status"])
        assert np.isfinite(want["R"]).all(axis=(1, 2)).sum() > n // 2


def test_scene_base(cuda):
    c = case(257, 4, "quat", scene_base=7)
    want = check(c, cuda, (0, c.n), range(4), "mean")
    for r in c.bad[:2]:
        assert (want["slot_status"][r] == M.NO_CAPTURE).all() and want["row_status"][r] == M.NO_ROTATION
    assert (want["slot_status"][c.bad[2]] == M.NO_VIEW).all()


@pytest.mark.parametrize("fuse", ("cam", "mean"))
@pytest.mark.parametrize("cams", ((2,), (0, 2), (3, 0, 2, 1), (2, 1, 1, 2)))
def test_camera_subsets(cuda, cams, fuse):
    for mode in M.MODES:
        check(case(257, 4, mode), cuda, (1, 200), cams, fuse)


@pytest.mark.parametrize("rows", ((0, 0), (0, 1), (4, 9), (-1, None)))
def test_row_ranges(cuda, rows):
    c = case(257, 4, "6d")
    rows = (c.n - 1, c.n) if rows[1] is None else rows
    check(c, cuda, rows, range(4), "mean")
    check(c, cuda, rows, (2, 0), "cam")


@pytest.mark.parametrize("omit", (("rot_views",), ("spread",), ("rot_views", "spread")))
def test_optional_outputs(cuda, omit):
    check(case(257, 4, "euler"), cuda, (0, 257), range(4), "mean", omit=omit)
    check(case(257, 4, "quat"), cuda, (3, 40), (1, 2), "cam", omit=omit)


def test_another_fuse_camera(cuda):
    c = case(257, 8, "quat")
    check(c, cuda, (0, c.n), (7, 3, 5), "cam", cam=5)


@pytest.mark.parametrize("mode", ("euler", "quat", "6d"))
def test_golden_rows(cuda, mode):
    """Every golden raw vector (the edge rows among them) as a one-camera row
    of a three-camera table over the golden rig: the model's bits, and within
    the model's measured distance of the reference's own results."""
    raw, cam = GOLDEN[f"{mode}_raw"], GOLDEN[f"{mode}_cam"]
    if mode == "euler":
        assert M.euler_filter(raw).all()
    n = len(raw)
    c = Case.__new__(Case)
    c.n, c.C, c.S, c.mode, c.scene_base = n, 3, 1, mode, 0
    c.raw = np.repeat(raw[:, None], 3, axis=1)
    c.views = np.where(np.arange(3)[None, :] == cam[:, None], 0, -1).astype(np.int32)
    c.scene = np.zeros(n, np.int32)
    c.X = np.random.default_rng(5).uniform(-300, 300, (n, 3))
    c.RTs = GOLDEN["rts"][None]
    want = check(c, cuda, (0, n), range(3), "mean")
    ok = np.isfinite(GOLDEN[f"{mode}_rot"]).all(axis=(1, 2))
    assert ((want["slot_status"][np.arange(n), cam] == 0) == ok).all()
    got_w = want["rot_views"][np.arange(n), cam]
    bound = {"quat": 2.0 ** -51, "euler": 2.0 ** -22, "6d": 2.0 ** -17}[mode]
    assert np.abs(got_w[ok] - GOLDEN[f"{mode}_world"][ok]).max() <= bound


def test_op_captures_into_a_graph(cuda):
    """One kernel node and no edge; the replay gives the eager bytes."""
    c = case(257, 4, "6d")
    eager = run_op(c, cuda, (0, c.n), (0, 2, 3), "mean")
    raw = torch.from_numpy(np.ascontiguousarray(c.raw[:, [0, 2, 3]])).to(cuda)
    args = c.device(cuda)
    out = {}
    for name, tail, dt, per_slot in OUTS:
        shape = (c.n,) + ((3,) if per_slot else ()) + tail
        out[name] = torch.full(shape, SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=cuda)
    torch.cuda.synchronize(cuda)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        torch.ops.mvmatch_views.fuse_rotations_out(raw, *args, 4, 0, 0, c.n, [0, 2, 3], "6d", "mean", 2,
                                                   *(out[k] for k, *_ in OUTS))
    assert all((v == (SENT_I if v.dtype == torch.int32 else SENT_F)).all() for v in out.values())   # captured, not run
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)             # hipGraphNodeTypeKernel == 0
    g.replay()
    torch.cuda.synchronize(cuda)
    for k, v in out.items():
        assert M.same(v.cpu().numpy(), eager[k]), k


def test_the_wrapper(cuda):
    """ops_views.fuse_rotations: defaults, shapes, host and device RTs."""
    c = case(257, 4, "quat")
    scene, views, X, RTs = c.device(cuda)
    raw = torch.from_numpy(c.raw).to(cuda)
    res = ops_views.fuse_rotations(raw, scene, views, X, c.RTs, 4, "quat")          # host RTs, fuse="cam", cam=2
    want = expected(c, (0, c.n), range(4), "cam")
    for k in ("R", "pose", "rot_views", "spread", "slot_status", "row_status"):
        assert M.same(getattr(res, k).cpu().numpy(), want[k]), k
    assert res.pose.shape == (c.n, 4, 4) and res.rot_views.shape == (c.n, 4, 3, 3)
    res = ops_views.fuse_rotations(raw[5:9, [3, 1]].contiguous(), scene, views, X, RTs, 4, "quat", rows=(5, 9),
                                   cams=(3, 1), fuse="mean")
    want = expected(c, (5, 9), (3, 1), "mean")
    for k in ("R", "pose", "rot_views", "spread", "slot_status", "row_status"):
        assert M.same(getattr(res, k).cpu().numpy(), want[k]), k
    res = ops_views.fuse_rotations(raw[:0], scene, views, X, RTs, 4, "quat", rows=(2, 2))
    assert res.pose.shape == (0, 4, 4) and res.spread.shape == (0, 4)


def test_argument_errors(cuda):
    c = case(257, 4, "quat")
    scene, views, X, RTs = c.device(cuda)
    raw = torch.from_numpy(c.raw).to(cuda)
    f = ops_views.fuse_rotations
    for bad in (dict(rows=(0, c.n + 1)), dict(rows=(3, 2)), dict(rows=(-1, 2)), dict(rows=5), dict(rows=(1, 2, 3)),
                dict(cams=()), dict(cams=(4,)), dict(cams=(-1,)), dict(cams=(0, 1, 2, 3, 0)),
                dict(cams=(0, 1)),                                    # fuse="cam" and camera 2 not selected
                dict(cam=5), dict(cam=1.0), dict(cam=True), dict(fuse="median"), dict(fuse=None),
                dict(rows=(0, 5))):                                   # raw holds every row
        with pytest.raises(ValueError):
            f(raw, scene, views, X, RTs, 4, "quat", **bad)
    for mode in ("euler", "6d", "matrix", None):                      # not raw's width, or no mode
        with pytest.raises(ValueError):
            f(raw, scene, views, X, RTs, 4, mode)
    for n_cams in (2, 9, 3, 5):                                       # outside the range, or not the table's
        with pytest.raises(ValueError):
            f(raw, scene, views, X, RTs, n_cams, "quat")
    with pytest.raises(ValueError, match="raw"):
        f(raw.double(), scene, views, X, RTs, 4, "quat")
    with pytest.raises(ValueError, match="raw"):
        f(raw.cpu(), scene, views, X, RTs, 4, "quat")
    with pytest.raises(ValueError, match="raw"):
        f(raw.transpose(0, 1).contiguous().transpose(0, 1), scene, views, X, RTs, 4, "quat")   # not contiguous
    with pytest.raises(ValueError, match="scene"):
        f(raw, scene.to(torch.int64), views, X, RTs, 4, "quat")
    with pytest.raises(ValueError, match="views"):
        f(raw, scene, views[:-1], X, RTs, 4, "quat")
    with pytest.raises(ValueError, match="X"):
        f(raw, scene, views, X.float(), RTs, 4, "quat")
    with pytest.raises(ValueError, match="X"):
        f(raw, scene, views, X[:-1], RTs, 4, "quat")
    with pytest.raises(ValueError, match="RTs"):
        f(raw, scene, views, X, RTs.float(), 4, "quat")
    with pytest.raises(ValueError, match="RTs"):
        f(raw, scene, views, X, RTs[:, :3], 4, "quat")
    with pytest.raises(ValueError, match="RTs"):
        f(raw, scene, views, X, RTs[:0], 4, "quat")                   # no capture
    with pytest.raises(ValueError, match="RTs"):
        f(raw, scene, views, X, RTs.cpu(), 4, "quat")
    # the op's own rows: the outputs
    op = torch.ops.mvmatch_views.fuse_rotations_out
    e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=cuda)
    good = dict(rot_views=e((2, 4, 3, 3)), R=e((2, 3, 3)), pose=e((2, 4, 4)), spread=e((2, 4)),
                slot_status=e((2, 4), torch.int32), row_status=e(2, torch.int32))
    call = lambda **kw: op(raw[:2].contiguous(), scene, views, X, RTs, 4, 0, 0, 2, [0, 1, 2, 3], "quat", "mean", 2,
                           *(dict(good, **kw)[k] for k, *_ in OUTS))
    call()
    for name in good:
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name][:1]})
    with pytest.raises(ValueError, match="slot_status"):
        call(slot_status=good["slot_status"].to(torch.int64))
    with pytest.raises(ValueError, match="scene"):
        op(raw[:2].contiguous(), scene, views, X, RTs, 4, 0, c.n - 1, 2, [0, 1, 2, 3], "quat", "mean", 2,
           *(good[k] for k, *_ in OUTS))                              # rows past the table
