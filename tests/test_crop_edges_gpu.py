"""The crop kernel on the GPU at its rounding, width and tiling edges (DESIGN
§3.18): the inputs of tests/crop_edges.py -- sums whose float32 quotient
estimate is off by one either way and sums on the exact rounding tie in both
accumulator widths, saturated boxes either side of the 32/64-bit switch,
canvases whose last workgroup is partly filled, every alignment of ``out`` in
both element types, INT32 corners, a 1 x 1 image, and a 4.5 GiB image set
whose crops lie beyond byte 2^31 and byte 2^32 -- against tests/crop_model.py
bit for bit, with the checks of tests/test_crop_gpu.py: ``out`` and ``geom``
pre-filled with sentinels between guards and compared whole, the inputs
unchanged.  tests/test_crop_edges_model.py pins on the CPU that these inputs
are where they claim to be."""
import numpy as np
import pytest
import torch

import crop_edges as E
import crop_model as M
from bpc_baseline_amd import ops_views
from test_crop_gpu import NP_OF, SENT_F, SENT_I, _bits, check

pytestmark = pytest.mark.gpu
DTYPES = (torch.float32, torch.float16)


def launch(args, dev, rows, cams, T, fill=255, dtype=torch.float32, offset=0, n_cams=3):
    """The op on device tensors ``args`` (images, scene, views, boxes), writing
    ``out`` and ``geom`` ``offset`` elements into flat sentinel buffers that go
    on for a guard beyond them -> (out, geom) on the host, the guards checked."""
    b, e = rows
    n_out, n_geom, guard = (e - b) * len(cams) * 3 * T * T, (e - b) * len(cams) * 8, 64
    buf = torch.full((offset + n_out + guard,), SENT_F, dtype=dtype, device=dev)
    gbuf = torch.full((offset + n_geom + guard,), SENT_I, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0                       # so the offset alone decides the alignment
    out = buf[offset:offset + n_out].view(e - b, len(cams), 3, T, T)
    geom = gbuf[offset:offset + n_geom].view(e - b, len(cams), 8)
    torch.ops.mvmatch_views.crop_views_out(*args, n_cams, 0, b, e - b, list(cams), T, fill,
                                           ops_views.norm_lut(dtype=dtype).to(dev), out, geom)
    torch.cuda.synchronize(dev)
    assert (buf[:offset] == SENT_F).all() and (buf[offset + n_out:] == SENT_F).all()
    assert (gbuf[:offset] == SENT_I).all() and (gbuf[offset + n_geom:] == SENT_I).all()
    return out.cpu().numpy(), geom.cpu().numpy()


def same(got, want):
    (out, geom), (w_out, w_geom) = got, want
    assert out.dtype == w_out.dtype and out.shape == w_out.shape
    assert np.array_equal(geom, w_geom)
    assert np.array_equal(_bits(out), _bits(w_out))


# ---- family A ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", E.TIE_SHAPES)
def test_the_quotient_estimate_and_the_tie(cuda, name, dtype):
    """Both repair loops of the final division and the exact tie, in 32-bit
    (32-*) and 64-bit (64-*) sums: every level is k or k + 1 by one source pixel."""
    t = E.ties(name)
    geom = check(t, cuda, (0, t.n), range(3), t.tags["T"], dtype=dtype)
    for r, c in t.tags["slots"]:
        assert E.is_wide(*geom[r, c, 3:5].tolist()) == name.startswith("64")


# ---- family B ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_either_side_of_the_switch(cuda, dtype):
    """The largest area with 32-bit sums and the next one, all 255, all 0 and random."""
    t = E.switch()
    geom = check(t, cuda, (0, 2), range(3), E.SWITCH_T, fill=7, dtype=dtype)
    assert [E.is_wide(*g[3:5].tolist()) for g in geom[:, 0]] == [False, True]


# ---- family C ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", E.TILING_T)
def test_partial_last_workgroups(cuda, T, dtype):
    t = E.tiling(T)
    geom = check(t, cuda, (0, t.n), E.TILING_CAMS, T, fill=3, dtype=dtype)
    assert set(geom[..., 0].reshape(-1)) == {M.OK, M.CLIPPED, M.EMPTY, M.NO_VIEW}
    if T >= 1023:
        th = E.thin(T)
        geom = check(th, cuda, (0, th.n), E.TILING_CAMS, T, fill=3, dtype=dtype)
        assert tuple(geom[0, 0, 5:7]) == (T, round(T / 20)) and tuple(geom[0, 1, 5:7]) == (32, T)


# ---- family D ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", (1, 2, 3, 4))
@pytest.mark.parametrize("T", (16, 66))
def test_every_alignment_of_out(cuda, T, offset, dtype):
    """Offsets 1-3 leave a plane off a 4-element boundary in either type
    (float16 at 2 is 4-byte but not 8-byte aligned); 4 is aligned at a base
    that is not the allocation's.  The bytes are the model's either way."""
    t = E.tiling(T)
    args = t.device(cuda)
    keep = [a.clone() for a in args]
    got = launch(args, cuda, (0, t.n), E.TILING_CAMS, T, 3, dtype, offset)
    for a, was in zip(args, keep):
        assert torch.equal(a, was)
    same(got, M.crop_views(t.images, t.scene, t.views, t.boxes, (0, t.n), list(E.TILING_CAMS), T, 3,
                           M.norm_lut(dtype=NP_OF[dtype])))


# ---- family E ----------------------------------------------------------------------------------------------------

def test_int32_corners_and_a_one_pixel_image(cuda):
    t = E.int32_corners()
    check(t, cuda, (0, 2), range(3), 16)                  # extreme corners alone
    check(t, cuda, (0, 4), (2, 0, 1), 16)                 # and among in-range boxes
    t = E.one_pixel_image()
    for T in (1, 16, 31):
        check(t, cuda, (0, 2), range(3), T)


@pytest.fixture(scope="module")
def far(cuda):
    """The 4.5 GiB of images on the device, zero but for the patches; the host
    holds the patches alone.  Freed when the module is done."""
    images = torch.zeros(E.FAR_SHAPE, dtype=torch.uint8, device=cuda)
    for name, patch in E.far_patches().items():
        s, c, y0, x0, ph, pw = E.FAR_PATCHES[name]
        images[s, c, y0:y0 + ph, x0:x0 + pw] = torch.from_numpy(patch).to(cuda)
    torch.cuda.synchronize(cuda)
    yield images
    del images
    torch.cuda.empty_cache()


def _far(images, dev, rows, T, dtype=torch.float32):
    scene, views, boxes = (torch.from_numpy(a).to(dev) for a in E.far_table(rows))
    tables = [a.clone() for a in (scene, views, boxes)]
    words = images.view(-1).view(torch.int64)
    before = int(words.sum())                             # wraps; any changed byte changes it
    got = launch((images, scene, views, boxes), dev, (0, len(rows)), E.FAR_CAMS, T, 255, dtype)
    assert int(words.sum()) == before
    for name, patch in E.far_patches().items():
        s, c, y0, x0, ph, pw = E.FAR_PATCHES[name]
        assert torch.equal(images[s, c, y0:y0 + ph, x0:x0 + pw].cpu(), torch.from_numpy(patch))
    for a, was in zip((scene, views, boxes), tables):
        assert torch.equal(a, was)
    same(got, E.far_expected(rows, T, 255, M.norm_lut(dtype=NP_OF[dtype])))
    return got[1]


def test_crops_beyond_2_31_and_2_32_bytes(cuda, far):
    """Interior, clipped and last-pixel boxes and both 16384-long strips at
    T = 16, where image 2 holds byte 2^31 and image 5 byte 2^32."""
    geom = _far(far, cuda, E.FAR_ROWS, 16)
    assert sorted(set(geom[:, 1, 7])) == [2, 5] and geom[7, 1, 1] == geom[7, 1, 2] == E.FAR_SIDE - 1
    _far(far, cuda, E.FAR_ROWS[5:7], 16, torch.float16)


def test_the_longest_strips_on_the_largest_canvas(cuda, far):
    """16384 x 8 and 8 x 16384 at T = 1024: the largest X w and (i + 1) new_w."""
    geom = _far(far, cuda, E.FAR_STRIP_ROWS, 1024)
    assert tuple(geom[0, 1, 3:7]) == (8, E.FAR_SIDE, 1, 1024) and tuple(geom[1, 1, 3:7]) == (E.FAR_SIDE, 8, 1024, 1)
