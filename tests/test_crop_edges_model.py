"""The inputs of tests/crop_edges.py are where they claim to be (DESIGN §3.18;
CPU): which sums the float32 quotient estimate gets wrong and which sit on the
rounding tie, what tests/crop_model.py makes of them, either side of the
32/64-bit switch, how many workgroups a canvas takes and how full the last one
is, and where the far patches lie in bytes.  Every condition is exact."""
import numpy as np
import pytest

import crop_edges as E
import crop_model as M


def _census(t):
    """(estimates above the floor, below it, exact ties) over a table's placed values."""
    T, d = t.tags["T"], t.tags["w"] * t.tags["h"]
    fx, fy = t.tags["w"] // T, t.tags["h"] // T
    above = below = tie = 0
    for k, off in t.tags["pairs"].reshape(-1, 2):
        n = E.tie_numerator(int(k), int(off), T, T, fx, fy)
        est = E.estimate(n, d)
        above, below, tie = above + (est > n // d), below + (est < n // d), tie + (n % d == 0)
    return above, below, tie


def test_the_estimate_fails_both_ways_in_both_widths():
    total = {False: np.zeros(3, int), True: np.zeros(3, int)}
    for name in E.TIE_SHAPES:
        t = E.ties(name)
        wide = E.is_wide(t.tags["w"], t.tags["h"])
        assert wide == name.startswith("64")
        counts = _census(t)
        print(name, "estimate above / below the floor, exact ties:", counts)
        total[wide] += counts
    for wide in (False, True):
        assert total[wide][0] >= 4 and total[wide][1] >= 4 and total[wide][2] >= 16
    # the starting shapes' own counts, over every k and offset (all of them are placed)
    assert _census(E.ties("32-T4"))[:2] == (70, 6) and _census(E.ties("64-T8"))[:2] == (83, 19)


def test_the_estimate_is_off_by_one_at_the_most():
    for name, (T, w, h, _) in E.TIE_SHAPES.items():
        for k, off in E.ties(name).tags["pairs"].reshape(-1, 2):
            n = E.tie_numerator(int(k), int(off), T, T, w // T, h // T)
            assert abs(E.estimate(n, w * h) - n // (w * h)) <= 1


@pytest.mark.parametrize("name", E.TIE_SHAPES)
def test_the_model_returns_the_designed_levels(name):
    """A third statement of the resample: a block of k with 1 added to half of
    it, less one, rounds to k; with 1 added to half of it or more, to k + 1."""
    t = E.ties(name)
    T, w, h = t.tags["T"], t.tags["w"], t.tags["h"]
    pairs = t.tags["pairs"]
    want = E.designed_level(pairs[..., 0], pairs[..., 1], (w // T) * (h // T))
    if name == "32-T8":
        assert (want == pairs[..., 0] + (pairs[..., 1] > 0)).all()            # an odd block: no tie
    else:
        assert (want == pairs[..., 0] + (pairs[..., 1] >= 0)).all()
    assert want.min() == 0 and want.max() == 255
    for i, (r, c) in enumerate(t.tags["slots"]):
        cv, g = M.canvas(t.images[r, c], t.boxes[r, c], T, 255)
        assert g == (M.OK, 5, 3, w, h, T, T)                      # whole factors: the canvas is the resample
        assert np.array_equal(cv, want[i])
    # the loops statement on a value of each offset (a footprint is fx fy source pixels)
    for off in E.OFFS:
        i, Y, X, ch = (int(v) for v in np.argwhere(pairs[..., 1] == off)[0])
        r, c = t.tags["slots"][i]
        src = t.images[r, c, 3:3 + h, 5:5 + w]
        lv = M.area_resample_loops(src[:, :, ch:ch + 1].repeat(3, 2), T, T, [(Y, X)])[(Y, X)]
        assert lv[0] == want[i, Y, X, ch]


def test_every_offset_and_level_is_placed():
    for name in E.TIE_SHAPES:
        pairs = E.ties(name).tags["pairs"].reshape(-1, 2)
        assert set(pairs[:, 1]) == set(E.OFFS)
        assert pairs[:, 0].min() == 0 and pairs[:, 0].max() == 254
    for name in ("32-T1", "64-T16"):                                  # all of them
        assert len({tuple(p) for p in E.ties(name).tags["pairs"].reshape(-1, 2)}) == 3 * 255
    # one step below the tie is one unit below it only where every weight is 1
    for name, (T, w, h, _) in E.TIE_SHAPES.items():
        n = E.tie_numerator(7, -1, T, T, w // T, h // T)
        assert ((n + 1) % (w * h) == 0) == (T == 1)


def test_which_sums_leave_32_bits():
    """The switch is taken a factor of two early, so just past it 32-bit sums
    would still be right: of these inputs only 64-T16's numerators reach 2^32
    (nor do those of a 4100 x 4100 box)."""
    assert [E.overflows_32(w, h) for w, h in E.SWITCH_BOXES] == [False, False]
    assert {n: E.overflows_32(w, h) for n, (_, w, h, _) in E.TIE_SHAPES.items()} == {
        "32-T1": False, "32-T4": False, "32-T8": False, "64-T8": False, "64-T16": True}
    assert E.is_wide(4100, 4100) and not E.overflows_32(4100, 4100)


def test_either_side_of_the_switch():
    (w0, h0), (w1, h1) = E.SWITCH_BOXES
    assert not E.is_wide(w0, h0) and E.is_wide(w1, h1)
    assert 510 * w0 * h0 == 4294967040 and w1 * h1 == w0 * h0 + 19
    # no larger area keeps 32-bit sums, and the largest 32-bit numerator fits
    assert E.is_wide(1, w0 * h0 + 1) and 255 * w0 * h0 + w0 * h0 // 2 == 2151694272 < 1 << 32
    t = E.switch()
    out, geom = M.crop_views(t.images, t.scene, t.views, t.boxes, (0, 2), [0, 1, 2], E.SWITCH_T, 7, M.norm_lut())
    lut = M.norm_lut()
    for r, (w, h) in enumerate(E.SWITCH_BOXES):
        for c in range(3):
            assert tuple(geom[r, c]) == (M.OK, 0, 0, w, h, 16, 16, c)
        for p in range(3):
            assert (out[r, 0, p] == lut[p, 255]).all() and (out[r, 1, p] == lut[p, 0]).all()
        assert len(np.unique(out[r, 2])) > 3                      # the random image is no constant


def test_blocks_per_canvas():
    """(workgroups a slot, pixels in the last) as the kernel tiles a canvas."""
    assert E.blocks(33, 1) == (2, 65)
    assert E.blocks(45, 1) == (2, 1001)                           # the walk ends in its fourth step
    assert E.blocks(1023, 1) == (1023, 1)
    assert E.blocks(1, 1) == (1, 1)
    assert E.blocks(2, 4) == (1, 4) and E.blocks(6, 4) == (1, 36)             # one thread; nine
    assert E.blocks(66, 4) == (2, 260)
    assert E.blocks(1024, 4) == (256, 4096)
    assert E.blocks(66, 1) == (5, 260)                            # at an unaligned base


@pytest.mark.parametrize("T", E.TILING_T)
def test_the_tiling_tables_hold_every_kind(T):
    t = E.tiling(T)
    _, geom = M.crop_views(t.images, t.scene, t.views, t.boxes, (0, t.n), list(E.TILING_CAMS), min(T, 8), 255,
                           M.norm_lut())
    assert [int(v) for v in geom[:2, :, 0].reshape(-1)] == [M.OK, M.CLIPPED, M.EMPTY, M.NO_VIEW]
    assert t.n * len(E.TILING_CAMS) <= 4 or T < 1023
    if T >= 1023:
        th = E.thin(T)
        assert all(M.clip_box(th.boxes[r, c], th.H, th.W)[0] == M.OK for r in range(th.n) for c in E.TILING_CAMS)
        assert tuple(th.boxes[0, 0, 2:] - th.boxes[0, 0, :2]) == (60, 3)
        assert tuple(th.boxes[0, 2, 2:] - th.boxes[0, 2, :2]) == (2, 64)
        new_w, new_h, dx, dy = M.sizes(60, 3, T)
        assert new_w == T and dy > T // 2 - 30
        new_w, new_h, dx, dy = M.sizes(2, 64, T)
        assert new_h == T and dx > T // 2 - 20


def test_int32_corners_clip_like_python_integers():
    t = E.int32_corners()
    _, geom = M.crop_views(t.images, t.scene, t.views, t.boxes, (0, 4), [0, 1, 2], 16, 255, M.norm_lut())
    assert [int(v) for v in geom[..., 0].reshape(-1)] == [1, 1, 2, 1, 2, 2, 0, 1, 0, 1, 0, 1]
    assert tuple(geom[0, 0, 1:5]) == (0, 0, 64, 48) and tuple(geom[3, 0, 1:5]) == (63, 47, 1, 1)
    t = E.one_pixel_image()
    _, geom = M.crop_views(t.images, t.scene, t.views, t.boxes, (0, 2), [0, 1, 2], 16, 255, M.norm_lut())
    assert [int(v) for v in geom[..., 0].reshape(-1)] == [0, 1, 2, 1, 2, 1]


def test_the_far_patches_lie_past_the_crossings():
    S, C, H, W, _ = E.FAR_SHAPE
    pitch, image = 3 * W, 3 * W * H
    assert 2 * image < 1 << 31 < 3 * image and 5 * image < 1 << 32 < 6 * image
    first = lambda name: (lambda s, c, y0, x0, ph, pw: (s * C + c) * image + y0 * pitch + 3 * x0)(*E.FAR_PATCHES[name])
    assert first("far2") > 1 << 31 and first("far5") > 1 << 32 and first("row5") > 1 << 32
    assert E.FAR_PATCHES["far5"][2] >= 11000 and first("near0") == 0
    # the strip down image 2 starts before byte 2^31 and ends after it
    assert first("col2") < 1 << 31 < first("col2") + (H - 1) * pitch
    # no two patches of one image overlap, and every box keeps inside its patch
    for a in E.FAR_PATCHES:
        for b in E.FAR_PATCHES:
            (s, c, y, x, h, w), (s2, c2, y2, x2, h2, w2) = E.FAR_PATCHES[a], E.FAR_PATCHES[b]
            if a < b and (s, c) == (s2, c2):
                assert y + h <= y2 or y2 + h2 <= y or x + w <= x2 or x2 + w2 <= x, (a, b)
    out, geom = E.far_expected(E.FAR_ROWS, 16, 255, M.norm_lut())
    assert [int(v) for v in geom[:, 1, 0]] == [0, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert tuple(geom[6, 1]) == (M.CLIPPED, W - 300, H - 200, 300, 200, 16, 11, 5)
    assert tuple(geom[7, 1]) == (M.OK, W - 1, H - 1, 1, 1, 16, 16, 5)
    assert tuple(geom[4, 1, 3:7]) == (8, H, 1, 16) and tuple(geom[9, 1, 3:7]) == (W, 8, 16, 1)
    scene, views, boxes = E.far_table(E.FAR_ROWS)
    assert list(scene) == [0] * 5 + [1] * 5 and (views[:, 1] == -1).all()
