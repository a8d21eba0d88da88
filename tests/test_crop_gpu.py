"""The pose head's input crops on the GPU (mvm_crop_views,
ops_views.crop_views) against tests/crop_model.py.

The op writes into a slice of sentinel-filled ``out`` / ``geom`` buffers with
a guard row on either side; both are compared whole and bit for bit with the
model, the guards with the sentinel, and the images and tables with what was
uploaded."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import crop_model as M
from bpc_baseline_amd import ops_views       # registers torch.ops.mvmatch_views.*

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -777.0, -12345              # what out / geom hold before the op
NP_OF = {torch.float32: np.float32, torch.float16: np.float16}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])


def special_boxes(T, H, W):
    """The boxes every table here holds: each is (x1, y1, x2, y2)."""
    N = 11
    out = [(5, 5, 6, 6), (5, 5, 6, 5 + N), (5, 5, 5 + N, 6)]                     # 1 x 1, 1 x N, N x 1
    for s in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
        if s >= 1:
            out += [(3, 2, 3 + s, 2 + s), (1, 1, 1 + s, 1 + min(s, 5)), (2, 0, 2 + min(s, 7), s)]
    for short in (1, 3, 5):                                                       # scale 1/2: x.5 sizes
        out += [(1, 0, 1 + short, 2 * T), (0, 1, 2 * T, 1 + short)]
    out += [(-5, -7, 10, 12), (W - 14, H - 8, W + 6, H + 12), (-3, 4, W + 3, 9),  # clipped
            (30, 10, 20, 20), (10, 30, 20, 20), (7, 7, 7, 12),                    # x2 < x1, y2 < y1, no width
            (W + 6, H + 2, W + 26, H + 12), (-9, -9, -1, -1), (W, 0, W + 5, 5),   # wholly outside
            (0, 0, W, H), (-1000, -1000, 10000, 10000),                           # the image, and beyond it
            (5, 5, 6, 6), (0, 0, W, H)]                                           # duplicates
    return out


class Case:
    """A hand-built table over random images: S captures of C cameras; slot
    (r, c) holds box (r C + c) mod len(boxes), so the boxes are gone through
    twice: the first time every slot has a view and a capture, the second
    time some views are -1, one row (``bad[0]``) has a scene id beyond the
    images and one (``bad[1]``) a scene id below ``scene_base``."""

    def __init__(self, H, W, C, T, S=2, n=None, scene_base=0, seed=0):
        rng = np.random.default_rng(1000 * H + 10 * C + T + seed)
        self.H, self.W, self.C, self.S, self.scene_base = H, W, C, S, scene_base
        self.images = rng.integers(0, 256, (S, C, H, W, 3), dtype=np.uint8)
        bx = special_boxes(T, H, W)
        once = -(-len(bx) // C)
        self.n = n = 2 * once if n is None else n
        assert n >= 2 * once
        self.boxes = np.array([bx[i % len(bx)] for i in range(n * C)], np.int32).reshape(n, C, 4)
        self.views = rng.integers(0, 40, (n, C)).astype(np.int32)
        self.views[once:][rng.random((n - once, C)) < 0.15] = -1
        self.scene = (np.arange(n) % S + scene_base).astype(np.int32)
        self.bad = (n - 3, n - 1)
        self.scene[n - 3] = S + scene_base
        self.scene[n - 1] = scene_base - 1

    def device(self, dev):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t(self.images), t(self.scene), t(self.views), t(self.boxes)


@lru_cache(maxsize=None)
def case(*a, **kw):
    return Case(*a, **kw)


def run_op(c, dev, rows, cams, T, fill=255, dtype=torch.float32, lut=None, want_geom=True):
    """The op on a fresh upload -> (out, geom) of the rows on the host, after
    checking the guards and that no input changed."""
    b, e = rows
    if lut is None:
        lut = ops_views.norm_lut(dtype=dtype)
    args = c.device(dev)
    keep = [a.clone() for a in args]
    out = torch.full((e - b + 2, len(cams), 3, T, T), SENT_F, dtype=dtype, device=dev)
    geom = torch.full((e - b + 2, len(cams), 8), SENT_I, dtype=torch.int32, device=dev)
    torch.ops.mvmatch_views.crop_views_out(*args, c.C, c.scene_base, b, e - b, list(cams), T, fill,
                                           lut.to(dev), out[1:e - b + 1],
                                           geom[1:e - b + 1] if want_geom else None)
    torch.cuda.synchronize(dev)
    for got, was in zip(args, keep):
        assert torch.equal(got, was)
    assert (out[0] == SENT_F).all() and (out[-1] == SENT_F).all()
    assert (geom[0] == SENT_I).all() and (geom[-1] == SENT_I).all()
    if not want_geom:
        assert (geom == SENT_I).all()
    return out[1:e - b + 1].cpu().numpy(), geom[1:e - b + 1].cpu().numpy()


def check(c, dev, rows, cams, T, fill=255, dtype=torch.float32, lut=None):
    out, geom = run_op(c, dev, rows, cams, T, fill, dtype, lut)
    lut_h = (ops_views.norm_lut(dtype=dtype) if lut is None else lut).numpy()
    w_out, w_geom = M.crop_views(c.images, c.scene, c.views, c.boxes, rows, list(cams), T, fill, lut_h,
                                 c.scene_base)
    assert out.dtype == NP_OF[dtype] and out.shape == w_out.shape
    assert np.array_equal(geom, w_geom)
    assert np.array_equal(_bits(out), _bits(w_out))
    return geom


@pytest.mark.parametrize("T", (8, 16, 31))
@pytest.mark.parametrize("C", (3, 4, 8))
@pytest.mark.parametrize("H, W", ((48, 64), (300, 280)))
def test_every_box_kind(cuda, H, W, C, T):
    c = case(H, W, C, T)
    geom = check(c, cuda, (0, c.n), range(C), T)
    assert set(geom[..., 0].reshape(-1)) == {0, 1, 2, 3, 4}          # every status occurs


def test_the_default_canvas(cuda):
    c = case(300, 280, 4, 256)
    check(c, cuda, (0, c.n), (2, 0), 256)


@pytest.mark.parametrize("rows", ((0, 0), (0, 1), (4, 9), (-1, None)))
def test_row_ranges(cuda, rows):
    c = case(48, 64, 4, 16)
    rows = (c.n - 1, c.n) if rows[1] is None else rows
    check(c, cuda, rows, range(4), 16)


@pytest.mark.parametrize("cams", ((2,), (0, 2), (3, 0, 2, 1), (1, 1)))
def test_camera_subsets(cuda, cams):
    check(case(48, 64, 4, 8), cuda, (1, 8), cams, 8)


def test_scene_base(cuda):
    c = case(48, 64, 3, 16, scene_base=7)
    geom = check(c, cuda, (0, c.n), range(3), 16)
    for r in c.bad:
        assert (geom[r, :, 0] == 4).all() and (geom[r, :, 7] == -1).all()


@pytest.mark.parametrize("T", (16, 31))
def test_float16(cuda, T):
    c = case(300, 280, 3, T)
    check(c, cuda, (0, c.n), (2, 1), T, dtype=torch.float16)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16))
def test_another_fill_and_table(cuda, dtype):
    lut = ops_views.norm_lut((0.1, 0.5, 0.9), (0.3, 1.0, 0.07), dtype)
    lut[1] = torch.arange(256).to(dtype) - 3          # no plane is a shift of another
    c = case(48, 64, 4, 31)
    check(c, cuda, (0, c.n), range(4), 31, fill=7, dtype=dtype, lut=lut)
    check(c, cuda, (0, 4), (1,), 31, fill=0, dtype=dtype, lut=lut)


def test_geom_is_optional(cuda):
    c = case(48, 64, 4, 16)
    out, _ = run_op(c, cuda, (0, c.n), (0, 3), 16, want_geom=False)
    w_out, _ = M.crop_views(c.images, c.scene, c.views, c.boxes, (0, c.n), [0, 3], 16, 255, M.norm_lut())
    assert np.array_equal(_bits(out), _bits(w_out))


def test_an_unaligned_output(cuda):
    """An even canvas in a buffer that starts off a 16-byte boundary: the element-store path."""
    c = case(48, 64, 4, 16)
    args = c.device(cuda)
    n_el = 2 * 4 * 3 * 16 * 16
    buf = torch.full((n_el + 2,), SENT_F, dtype=torch.float32, device=cuda)
    out = buf[1:n_el + 1].view(2, 4, 3, 16, 16)
    torch.ops.mvmatch_views.crop_views_out(*args, 4, 0, 0, 2, [0, 1, 2, 3], 16, 255,
                                           ops_views.norm_lut().to(cuda), out, None)
    w_out, _ = M.crop_views(c.images, c.scene, c.views, c.boxes, (0, 2), [0, 1, 2, 3], 16, 255, M.norm_lut())
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(w_out))
    assert buf[0] == SENT_F and buf[-1] == SENT_F


def test_sums_beyond_32_bits(cuda):
    """One slot at T = 16: a 4100 x 4100 box of a 4200 x 4200 image, 2 * 255 * w * h >= 2^32."""
    rng = np.random.default_rng(6)
    one = rng.integers(0, 256, (4200, 4200, 3), dtype=np.uint8)
    c = Case.__new__(Case)
    c.H = c.W = 4200
    c.C, c.S, c.scene_base, c.n = 3, 1, 0, 1
    c.images = np.broadcast_to(one, (1, 3, 4200, 4200, 3))     # the cameras share the pixels
    c.boxes = np.array([[(0, 0, 9, 9), (1, 1, 4, 4), (50, 60, 4150, 4160)]], np.int32)
    c.views = np.zeros((1, 3), np.int32)
    c.scene = np.zeros(1, np.int32)
    geom = check(c, cuda, (0, 1), (2,), 16)
    assert tuple(geom[0, 0]) == (0, 50, 60, 4100, 4100, 16, 16, 2)


@pytest.mark.parametrize("slots", (1, 5, 1025))
def test_slot_counts(cuda, slots):
    if slots == 1:
        c, rows, cams = case(48, 64, 3, 8), (2, 3), (2,)
    elif slots == 5:
        c, rows, cams = case(48, 64, 8, 8), (1, 2), (7, 0, 3, 2, 5)
    else:
        c, rows, cams = case(48, 64, 8, 8, n=205), (0, 205), (7, 0, 3, 2, 5)
    assert (rows[1] - rows[0]) * len(cams) == slots
    check(c, cuda, rows, cams, 8)


def test_the_wrapper(cuda):
    """ops_views.crop_views: defaults, shapes and the keywords."""
    c = case(48, 64, 4, 16)
    images, scene, views, boxes = c.device(cuda)
    crops, geom = ops_views.crop_views(images, scene, views, boxes, 4, rows=(0, 3), cams=(2,), size=16)
    assert crops.shape == (3, 1, 3, 16, 16) and crops.dtype == torch.float32 and geom.shape == (3, 1, 8)
    w_out, w_geom = M.crop_views(c.images, c.scene, c.views, c.boxes, (0, 3), [2], 16, 255, M.norm_lut())
    assert np.array_equal(_bits(crops.cpu().numpy()), _bits(w_out)) and np.array_equal(geom.cpu().numpy(), w_geom)
    crops, geom = ops_views.crop_views(images, scene, views, boxes, 4, size=8, mean=(0.1, 0.5, 0.9),
                                       std=(0.3, 1.0, 0.07), fill=3, dtype=torch.float16)
    lut = M.norm_lut((0.1, 0.5, 0.9), (0.3, 1.0, 0.07), np.float16)
    w_out, w_geom = M.crop_views(c.images, c.scene, c.views, c.boxes, (0, c.n), [0, 1, 2, 3], 8, 3, lut)
    assert np.array_equal(_bits(crops.cpu().numpy()), _bits(w_out)) and np.array_equal(geom.cpu().numpy(), w_geom)
    crops, geom = ops_views.crop_views(images, scene, views, boxes, 4, rows=(2, 2), size=8)
    assert crops.shape == (0, 4, 3, 8, 8) and geom.shape == (0, 4, 8)


def test_argument_errors(cuda):
    c = case(48, 64, 4, 16)
    images, scene, views, boxes = c.device(cuda)
    f = lambda *a, **kw: ops_views.crop_views(*a, **kw)
    ok = dict(size=8)
    for bad in (dict(rows=(0, c.n + 1)), dict(rows=(3, 2)), dict(rows=(-1, 2)), dict(rows=5), dict(rows=(1, 2, 3)),
                dict(cams=()), dict(cams=(4,)), dict(cams=(-1,)), dict(cams=(0, 1, 2, 3, 0)),
                dict(size=0), dict(size=1025), dict(size=8.0), dict(size=True),
                dict(fill=-1), dict(fill=256), dict(fill=1.5),
                dict(dtype=torch.float64), dict(dtype=torch.bfloat16),
                dict(mean=(0.5, 0.5)), dict(std=(1, 1, 1, 1))):
        with pytest.raises(ValueError):
            f(images, scene, views, boxes, 4, **dict(ok, **bad))
    for n_cams in (2, 9, 3, 5):                       # outside the range, or not the images'
        with pytest.raises(ValueError):
            f(images, scene, views, boxes, n_cams, **ok)
    with pytest.raises(ValueError, match="images"):
        f(images.to(torch.int32), scene, views, boxes, 4, **ok)
    with pytest.raises(ValueError, match="images"):
        f(images[..., :2], scene, views, boxes, 4, **ok)
    with pytest.raises(ValueError, match="images"):
        f(images[:, :, :, ::2], scene, views, boxes, 4, **ok)             # not contiguous
    with pytest.raises(ValueError, match="images"):
        f(images.cpu(), scene, views, boxes, 4, **ok)
    with pytest.raises(ValueError, match="scene"):
        f(images, scene.to(torch.int64), views, boxes, 4, **ok)
    with pytest.raises(ValueError, match="views"):
        f(images, scene, views[:-1], boxes, 4, **ok)
    with pytest.raises(ValueError, match="boxes"):
        f(images, scene, views, boxes[:-1], 4, **ok)
    with pytest.raises(ValueError, match="boxes"):
        f(images, scene, views, boxes.cpu(), 4, **ok)
    # the op's own rows: the table and the outputs
    lut = ops_views.norm_lut().to(cuda)
    out = torch.empty((2, 4, 3, 8, 8), device=cuda)
    geom = torch.empty((2, 4, 8), dtype=torch.int32, device=cuda)
    op = torch.ops.mvmatch_views.crop_views_out
    cams = [0, 1, 2, 3]
    with pytest.raises(ValueError, match="lut"):
        op(images, scene, views, boxes, 4, 0, 0, 2, cams, 8, 255, lut.half(), out, geom)
    with pytest.raises(ValueError, match="lut"):
        op(images, scene, views, boxes, 4, 0, 0, 2, cams, 8, 255, lut[:2], out, geom)
    with pytest.raises(ValueError, match="out"):
        op(images, scene, views, boxes, 4, 0, 0, 2, cams, 8, 255, lut, out[:1], geom)
    with pytest.raises(ValueError, match="geom"):
        op(images, scene, views, boxes, 4, 0, 0, 2, cams, 8, 255, lut, out, geom[:1])
    with pytest.raises(ValueError, match="scene"):
        op(images, scene, views, boxes, 4, 0, c.n - 1, 2, cams, 8, 255, lut, out, geom)       # rows past the table
    with pytest.raises(ValueError, match="images"):
        op(images[:0], scene, views, boxes, 4, 0, 0, 2, cams, 8, 255, lut, out, geom)         # no capture


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
    """The launch function enqueues one kernel and nothing else, so the op
    captures into a hipGraph of one kernel node and no edge, and its replay
    gives the eager bytes."""
    c = case(48, 64, 4, 16)
    eager_out, eager_geom = run_op(c, cuda, (0, c.n), (0, 2), 16)
    args = c.device(cuda)
    lut = ops_views.norm_lut().to(cuda)
    out = torch.full((c.n, 2, 3, 16, 16), SENT_F, device=cuda)
    geom = torch.full((c.n, 2, 8), SENT_I, dtype=torch.int32, device=cuda)
    torch.cuda.synchronize(cuda)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        torch.ops.mvmatch_views.crop_views_out(*args, 4, 0, 0, c.n, [0, 2], 16, 255, lut, out, geom)
    assert (out == SENT_F).all() and (geom == SENT_I).all()          # captured, not run
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)             # hipGraphNodeTypeKernel == 0
    g.replay()
    torch.cuda.synchronize(cuda)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(eager_out))
    assert np.array_equal(geom.cpu().numpy(), eager_geom)
