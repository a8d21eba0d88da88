"""tests/crop_model.py against itself and against closed forms (DESIGN §3.18;
CPU).  Every condition is exact: the model is integer arithmetic up to the
look-up, and the look-up copies table entries."""
import numpy as np
import pytest
import torch

import crop_model as M
from bpc_baseline_amd import ops_views


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_the_two_statements_of_the_resample_agree():
    """~200 random (w, h, T): the matrix products and the per-pixel loops."""
    rng = np.random.default_rng(18)
    n = 0
    for T in (8, 16, 31, 256):
        for _ in range(50):
            w, h = (int(v) for v in rng.integers(1, 3 * T if T < 256 else 400, 2))
            new_w, new_h, _, _ = M.sizes(w, h, T)
            src = _img(h, w, rng.integers(1 << 30))
            got = M.area_resample(src, new_h, new_w)
            # every pixel of a small result, a sample of a large one
            pix = None
            if new_w * new_h > 400:
                pix = [(int(rng.integers(new_h)), int(rng.integers(new_w))) for _ in range(60)]
                pix += [(0, 0), (new_h - 1, new_w - 1), (0, new_w - 1), (new_h - 1, 0)]
            for (Y, X), lv in M.area_resample_loops(src, new_h, new_w, pix).items():
                assert tuple(int(v) for v in got[Y, X]) == lv, (w, h, T, Y, X)
            n += 1
    assert n == 200


@pytest.mark.parametrize("T", (8, 16, 31))
def test_closed_forms(T):
    src = _img(T, T, 1)
    assert np.array_equal(M.area_resample(src, T, T), src)                       # the same size: unchanged
    big = _img(2 * T, 2 * T, 2)
    mean = big.astype(np.int64).reshape(T, 2, T, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(M.area_resample(big, T, T), (2 * mean + 4) // 8)       # rounded 2 x 2 block means
    if T % 2 == 0:
        small = _img(T // 2, T // 2, 3)
        assert np.array_equal(M.area_resample(small, T, T), small.repeat(2, 0).repeat(2, 1))
    const = np.empty((5, 7, 3), np.uint8)
    const[:] = (3, 140, 255)
    cv, g = M.canvas(np.pad(const, ((2, 2), (2, 2), (0, 0))), (2, 2, 9, 7), T, 9)
    new_w, new_h, dx, dy = M.sizes(7, 5, T)
    assert g == (M.OK, 2, 2, 7, 5, new_w, new_h)
    assert (cv[dy:dy + new_h, dx:dx + new_w] == (3, 140, 255)).all()
    mask = np.ones((T, T), bool)
    mask[dy:dy + new_h, dx:dx + new_w] = False
    assert (cv[mask] == 9).all()
    one = _img(6, 6, 4)
    cv, g = M.canvas(one, (4, 1, 5, 2), T, 0)                                     # 1 x 1 fills the canvas
    assert g == (M.OK, 4, 1, 1, 1, T, T) and (cv == one[1, 4]).all()


def test_half_way_sizes_round_to_even():
    # T = 16, long side 32: scale 0.5
    assert M.sizes(1, 32, 16)[:2] == (1, 16)      # 0.5 -> 0, floored to 1
    assert M.sizes(3, 32, 16)[:2] == (2, 16)      # 1.5 -> 2
    assert M.sizes(5, 32, 16)[:2] == (2, 16)      # 2.5 -> 2
    assert M.sizes(32, 1, 16)[:2] == (16, 1)
    assert M.sizes(5, 32, 16)[2:] == (7, 0)


def test_clip_cases():
    H, W = 48, 64
    assert M.clip_box((0, 0, W, H), H, W) == (M.OK, 0, 0, W, H)                   # the image itself
    assert M.clip_box((-5, -7, 10, 12), H, W) == (M.CLIPPED, 0, 0, 10, 12)       # negative corners
    assert M.clip_box((50, 40, 70, 60), H, W) == (M.CLIPPED, 50, 40, 14, 8)      # beyond W and H
    assert M.clip_box((30, 10, 20, 20), H, W) == (M.EMPTY, 0, 0, 0, 0)           # x2 < x1
    assert M.clip_box((10, 30, 20, 20), H, W) == (M.EMPTY, 0, 0, 0, 0)
    assert M.clip_box((70, 50, 90, 60), H, W) == (M.EMPTY, 0, 0, 0, 0)           # wholly outside
    assert M.clip_box((-9, -9, -1, -1), H, W) == (M.EMPTY, 0, 0, 0, 0)
    assert M.clip_box((5, 5, 5, 9), H, W) == (M.EMPTY, 0, 0, 0, 0)               # zero width
    img = _img(H, W, 5)
    cv, g = M.canvas(img, (70, 50, 90, 60), 8, 200)
    assert g == (M.EMPTY, 0, 0, 0, 0, 0, 0) and (cv == 200).all()
    # a clipped box is the crop of its clipped part
    a, _ = M.canvas(img, (-5, -7, 10, 12), 16, 255)
    b, _ = M.canvas(img, (0, 0, 10, 12), 16, 255)
    assert np.array_equal(a, b)


def test_norm_lut_is_to_tensor_then_normalize():
    v = torch.arange(256, dtype=torch.uint8)
    for mean, std in ((M.MEAN, M.STD), ((0.1, 0.5, 0.9), (0.3, 1.0, 0.07))):
        want = torch.stack([v.float().div(255).sub(mean[c]).div(std[c]) for c in range(3)])
        got = ops_views.norm_lut(mean, std)
        assert got.dtype == torch.float32 and got.shape == (3, 256)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))          # all 768 entries, bit for bit
        half = ops_views.norm_lut(mean, std, torch.float16)
        assert torch.equal(half.view(torch.int16), want.half().view(torch.int16))
        assert np.array_equal(M.norm_lut(mean, std).view(np.int32), got.numpy().view(np.int32))
        assert np.array_equal(M.norm_lut(mean, std, np.float16).view(np.int16), half.numpy().view(np.int16))
    with pytest.raises(ValueError):
        ops_views.norm_lut(dtype=torch.float64)
    with pytest.raises(ValueError):
        ops_views.norm_lut((0.5, 0.5), (1, 1, 1))


def test_look_up_swaps_the_channels():
    cv = np.zeros((2, 2, 3), np.uint8)
    cv[..., 0], cv[..., 1], cv[..., 2] = 10, 20, 30        # B, G, R
    lut = np.arange(768, dtype=np.float32).reshape(3, 256)
    out = M.look_up(cv, lut)
    assert out.shape == (3, 2, 2)
    assert (out[0] == 30).all() and (out[1] == 256 + 20).all() and (out[2] == 512 + 10).all()


def test_a_crop_whose_sums_need_64_bits():
    """4100 x 4100 of a 4200 x 4200 image: 2 * 255 * w * h > 2^32."""
    img = _img(4200, 4200, 6)
    T = 16
    assert 2 * 255 * 4100 * 4100 >= 1 << 32
    cv, g = M.canvas(img, (50, 60, 4150, 4160), T, 255)
    assert g == (M.OK, 50, 60, 4100, 4100, T, T)
    pix = [(0, 0), (15, 15), (7, 9), (3, 12)]
    for (Y, X), lv in M.area_resample_loops(img[60:4160, 50:4150], T, T, pix).items():
        assert tuple(int(v) for v in cv[Y, X]) == lv
