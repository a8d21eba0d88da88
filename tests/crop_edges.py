"""Hand-built inputs at the edges of the crop kernel: sums whose
float32 quotient estimate is off by one in either direction and sums on the
exact rounding tie, in both accumulator widths; saturated boxes either side of
the 32/64-bit switch; canvases whose last workgroup is partly filled; boxes
with INT32 corners and a 1 x 1 image; patches of a 2 x 3 x 16384 x 16384 image
set beyond byte 2^31 and byte 2^32.  A helper, not a test:
tests/test_crop_edges_model.py proves on the CPU which regime every input is
in, tests/test_crop_edges_gpu.py demands the model's bits of the device.

Every builder returns a ``Table`` with the fields tests/test_crop_gpu.py's
``Case`` carries, so its ``run_op`` and ``check`` take it.
"""
from functools import lru_cache

import numpy as np

import crop_model as M

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
OFFS = (-1, 0, 1)                    # one step below the rounding tie, on it, one step above


class Table:
    """``images`` uint8 [S, C, H, W, 3], ``scene`` int32 [n], ``views`` int32
    [n, C], ``boxes`` int32 [n, C, 4]; ``tags`` holds what a family knows of
    its slots."""

    def __init__(self, images, scene, views, boxes, scene_base=0, **tags):
        self.images = images
        self.scene = np.ascontiguousarray(scene, np.int32)
        self.views = np.ascontiguousarray(views, np.int32)
        self.boxes = np.ascontiguousarray(boxes, np.int32)
        self.S, self.C, self.H, self.W = images.shape[:4]
        self.n, self.scene_base = len(self.scene), scene_base
        assert images.dtype == np.uint8 and images.shape[4] == 3 and self.C >= 3
        assert self.views.shape == (self.n, self.C) and self.boxes.shape == (self.n, self.C, 4)
        self.tags = tags

    def device(self, dev):
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t(self.images), t(self.scene), t(self.views), t(self.boxes)


def is_wide(w: int, h: int) -> bool:
    """The kernel's switch to 64-bit sums, stated with Python integers."""
    return 2 * 255 * w * h >= 1 << 32


# ---- family A: the quotient estimate, the tie ------------------------------------------------------------------

def estimate(n: int, d: int) -> int:
    """The kernel's first guess at n // d: both operands rounded to IEEE
    float32, one float32 division, truncated."""
    assert n < 1 << 53 and d < 1 << 53                    # exact as doubles: one rounding each
    return int(np.float32(n) / np.float32(d))


def tie_numerator(k: int, off: int, new_w: int, new_h: int, fx: int, fy: int) -> int:
    """s + half of a destination pixel whose fy x fx source block holds ``k``
    with 1 added to its first ff // 2 + off pixels, ff = fx fy: every weight is
    new_w new_h, the block's sum is k ff + ff // 2 + off.  With an even ff,
    off = 0 is the exact tie; an odd ff (259 x 259) has none, its off = 0 is
    half a pixel below and its off = +1 half a pixel above."""
    ff = fx * fy
    return new_w * new_h * (k * ff + ff // 2 + off) + (fx * new_w * fy * new_h) // 2


def designed_level(k, off, ff):
    """(2 S + ff) // (2 ff) of S = k ff + ff // 2 + off, |off| <= 1, by hand:
    k + 1 once the added ones are half the block, else k."""
    return k + (2 * (ff // 2 + off) >= ff)


# T, w, h, slots; 32-*: 32-bit sums.  At T = 1 every weight is 1, so one step
# below the tie is one unit of the sum below it (at T > 1 it is T^2 units: a
# rounding constant that is off by one would go unseen); its 255 slots hold
# every (k, off).  Of the 64-bit shapes only 64-T16 has numerators of 2^32 and
# more (``overflows_32``): 64-T8's would still fit.
TIE_SHAPES = {"32-T1": (1, 30, 20, 255), "32-T4": (4, 1528, 1532, 3), "32-T8": (8, 2072, 2072, 3),
              "64-T8": (8, 3464, 3472, 3), "64-T16": (16, 4128, 4128, 1)}


def overflows_32(w: int, h: int) -> bool:
    """Whether the largest s + half of a w x h box needs more than 32 bits."""
    return 255 * w * h + w * h // 2 >= 1 << 32


def tie_pairs(T, w, h, capacity):
    """-> int [capacity, 2] of (k, off): every pair whose estimate misses the
    floor first, then a spread of k from 0 to 254 at the three offsets."""
    new_w, new_h, _, _ = M.sizes(w, h, T)
    fx, fy = w // new_w, h // new_h
    assert fx * new_w == w and fy * new_h == h
    missed, rest = [], []
    for k in range(255):
        for off in OFFS:
            n = tie_numerator(k, off, new_w, new_h, fx, fy)
            (missed if estimate(n, w * h) != n // (w * h) else rest).append((k, off))
    assert len(missed) <= capacity
    room = capacity - len(missed)
    if room <= len(rest):
        spread = [rest[i] for i in np.linspace(0, len(rest) - 1, room).round().astype(int)]
    else:
        spread = rest + [missed[i % len(missed)] for i in range(room - len(rest))]
    return np.array(missed + spread, np.int64).reshape(capacity, 2)


@lru_cache(maxsize=None)
def ties(name):
    """One row a capture, three cameras; slot i is row i // 3, camera i % 3, its
    box w x h at (5, 3) of an image 9 wider and 7 taller whose margin is random.
    tags: ``T``, ``slots`` [(row, cam)], ``pairs`` int [slots, T, T, 3, 2] (the
    (k, off) of destination pixel (Y, X), source channel c), ``w``, ``h``."""
    T, w, h, n_slots = TIE_SHAPES[name]
    new_w, new_h, dx, dy = M.sizes(w, h, T)
    assert (new_w, new_h, dx, dy) == (T, T, 0, 0)
    fx, fy = w // T, h // T
    rng = np.random.default_rng(T * w + h)
    pairs = tie_pairs(T, w, h, n_slots * T * T * 3)
    pairs = pairs[rng.permutation(len(pairs))].reshape(n_slots, T, T, 3, 2)
    n, xa, ya = -(-n_slots // 3), 5, 3
    images = rng.integers(0, 256, (n, 3, h + 7, w + 9, 3), dtype=np.uint8)
    views = np.full((n, 3), -1, np.int32)
    boxes = np.zeros((n, 3, 4), np.int32)
    idx = (np.arange(fy)[:, None] * fx + np.arange(fx)[None, :])[None, :, None, :, None]       # [1, fy, 1, fx, 1]
    slots = []
    for i in range(n_slots):
        r, c = divmod(i, 3)
        k, off = (pairs[i, :, None, :, None, :, j] for j in (0, 1))                           # [T, 1, T, 1, 3]
        block = k.astype(np.uint8) + (idx.astype(np.int32) < (fx * fy // 2 + off).astype(np.int32))
        images[r, c, ya:ya + h, xa:xa + w] = block.reshape(h, w, 3)
        views[r, c], boxes[r, c] = 7, (xa, ya, xa + w, ya + h)
        slots.append((r, c))
    return Table(images, np.arange(n), views, boxes, T=T, slots=slots, pairs=pairs, w=w, h=h)


# ---- family B: either side of the switch, saturated -------------------------------------------------------------

SWITCH_BOXES = ((2892, 2912), (2893, 2911))               # w, h: the largest 32-bit area, and one above it
SWITCH_T = 16


@lru_cache(maxsize=None)
def switch():
    """Row i holds SWITCH_BOXES[i] at (0, 0) in the three cameras: all 255, all
    0, random."""
    rng = np.random.default_rng(2892)
    images = np.zeros((1, 3, 2912, 2893, 3), np.uint8)
    images[0, 0] = 255
    images[0, 2] = rng.integers(0, 256, images.shape[2:], dtype=np.uint8)
    boxes = np.array([[(0, 0, w, h)] * 3 for w, h in SWITCH_BOXES], np.int32)
    return Table(images, [0, 0], np.zeros((2, 3), np.int32), boxes)


# ---- family C: partial last workgroups, extreme canvases ----------------------------------------------------------

TILING_T = (1, 2, 6, 33, 45, 66, 1023, 1024)
TILING_CAMS = (0, 2)
BLOCK_THREADS, BLOCK_STEPS = 256, 4                       # the kernel's workgroup: a block owns 4 * 256 * PIX pixels


def blocks(T, pix):
    """-> (workgroups a slot, pixels in the last one) of the PIX instance."""
    per = BLOCK_STEPS * BLOCK_THREADS * pix
    n = -(-T * T // per)
    return n, T * T - (n - 1) * per


def _small_images(seed, S=2, H=70, W=90):
    return np.random.default_rng(seed).integers(0, 256, (S, 3, H, W, 3), dtype=np.uint8)


@lru_cache(maxsize=None)
def tiling(T):
    """Over TILING_CAMS the slots are: made, clipped; empty, no view; and below
    T = 1023 a third row: a 1 x 1 box, a tall one.  Source boxes of at most 44
    px a side: the kernel enlarges at the large T."""
    n = 2 if T >= 1023 else 3
    views = np.full((n, 3), 5, np.int32)
    boxes = np.zeros((n, 3, 4), np.int32)
    boxes[0] = (10, 8, 50, 41), (1, 1, 9, 9), (-6, 40, 38, 75)
    boxes[1] = (30, 10, 20, 20), (2, 2, 30, 30), (12, 12, 40, 30)
    views[1, 2] = -1
    if n == 3:
        boxes[2] = (5, 5, 6, 6), (0, 0, 90, 70), (60, 2, 67, 45)
    return Table(_small_images(T), np.arange(n) % 2, views, boxes)


@lru_cache(maxsize=None)
def thin(T):
    """Long thin boxes, so that dy or dx is most of the canvas: 60 x 3 and
    2 x 64, then a 1 x 1 box and a 3 x 2 one."""
    boxes = np.zeros((2, 3, 4), np.int32)
    boxes[0] = (2, 30, 62, 33), (0, 0, 1, 1), (40, 3, 42, 67)
    boxes[1] = (88, 68, 89, 69), (0, 0, 1, 1), (50, 50, 53, 52)
    return Table(_small_images(T + 1), [1, 0], np.full((2, 3), 5, np.int32), boxes)


# ---- family E: INT32 corners, a 1 x 1 image, offsets beyond 2^31 and 2^32 bytes ----------------------------------

@lru_cache(maxsize=None)
def int32_corners():
    """Rows 0-1 hold only boxes with an INT32_MIN / INT32_MAX corner, rows 2-3
    mix them with in-range ones."""
    lo, hi = INT32_MIN, INT32_MAX
    boxes = np.array([
        [(lo, lo, hi, hi), (lo, 3, 10, hi), (hi, 0, lo, 5)],             # the image; clipped; x2 < x1
        [(5, lo, hi, 7), (hi, hi, hi, hi), (lo, lo, lo + 1, lo + 1)],    # clipped; outside on either side
        [(4, 4, 20, 30), (lo, lo, 1, 1), (2, 2, 11, 9)],                 # in range; the first pixel; in range
        [(63, 47, hi, hi), (3, 1, 40, 21), (0, lo, 64, 48)],             # the last pixel; in range; clipped
    ], np.int64)
    return Table(_small_images(31, H=48, W=64), [0, 1, 1, 0], np.full((4, 3), 1, np.int32), boxes)


@lru_cache(maxsize=None)
def one_pixel_image():
    boxes = np.array([[(0, 0, 1, 1), (-5, -5, 5, 5), (1, 1, 2, 2)],
                      [(0, 0, 1, 2), (1, 0, 2, 1), (INT32_MIN, 0, INT32_MAX, 1)]], np.int64)
    return Table(_small_images(11, H=1, W=1), [1, 0], np.full((2, 3), 1, np.int32), boxes)


FAR_SHAPE = (2, 3, 16384, 16384, 3)                      # 4.5 GiB: image 2 holds byte 2^31, image 5 byte 2^32
FAR_SIDE = 16384
# (scene, camera, y0, x0, rows, columns): where a host patch goes in the images
FAR_PATCHES = {
    "far2": (0, 2, FAR_SIDE - 320, FAR_SIDE - 330, 320, 330),             # the far corner of image 2
    "far5": (1, 2, FAR_SIDE - 320, FAR_SIDE - 330, 320, 330),             # of image 5: past byte 2^32
    "near0": (0, 0, 0, 0, 300, 310),                                      # the near corner of image 0
    "row5": (1, 2, 12000, 0, 12, FAR_SIDE),                               # a strip across image 5
    "col2": (0, 2, 0, 9000, FAR_SIDE, 12),                                # a strip down image 2
}
_E = FAR_SIDE
# rows of (patch, box) per selected camera (0, 2); None: views = -1
FAR_ROWS = (
    (("near0", (20, 30, 200, 170)), ("far2", (_E - 300, _E - 290, _E - 100, _E - 150))),      # interior boxes
    (("near0", (-7, -9, 120, 100)), ("far2", (_E - 300, _E - 200, _E + 6, _E + 16))),         # clipped
    (None, ("far2", (_E - 1, _E - 1, _E, _E))),                                               # the last pixel
    (None, ("col2", (9002, 7000, 9010, 7400))),
    (None, ("col2", (9002, 0, 9010, _E))),                                                    # 8 x 16384
    (None, ("far5", (_E - 300, _E - 290, _E - 100, _E - 150))),
    (None, ("far5", (_E - 300, _E - 200, _E + 6, _E + 16))),
    (None, ("far5", (_E - 1, _E - 1, _E, _E))),
    (None, ("row5", (5000, 12002, 5300, 12010))),
    (None, ("row5", (0, 12002, _E, 12010))),                                                  # 16384 x 8
)
FAR_STRIP_ROWS = (FAR_ROWS[4], FAR_ROWS[9])
FAR_CAMS = (0, 2)


@lru_cache(maxsize=None)
def far_patches():
    rng = np.random.default_rng(16384)
    return {name: rng.integers(0, 256, (ph, pw, 3), dtype=np.uint8)
            for name, (_, _, _, _, ph, pw) in FAR_PATCHES.items()}


def far_table(rows):
    """-> (scene, views, boxes) of the rows over FAR_SHAPE's three cameras."""
    n = len(rows)
    scene, views, boxes = np.zeros(n, np.int32), np.full((n, 3), -1, np.int32), np.zeros((n, 3, 4), np.int32)
    for r, row in enumerate(rows):
        for cam, entry in zip(FAR_CAMS, row):
            if entry is not None:
                s, c = FAR_PATCHES[entry[0]][:2]
                assert c == cam and (scene[r] == s or views[r].max() < 0)
                scene[r], views[r, cam], boxes[r, cam] = s, 3, entry[1]
    return scene, views, boxes


def far_expected(rows, T, fill, lut):
    """What the op writes for the rows over FAR_CAMS: each crop is the model's
    on the host patch with the box translated into it (the patch holds the
    whole clipped box and shares the image's edges where the box is clipped)."""
    patches = far_patches()
    out = np.empty((len(rows), 2, 3, T, T), lut.dtype)
    geom = np.zeros((len(rows), 2, 8), np.int32)
    blank = M.look_up(np.full((T, T, 3), fill, np.uint8), lut)
    for r, row in enumerate(rows):
        for k, entry in enumerate(row):
            if entry is None:
                out[r, k], geom[r, k, 0] = blank, M.NO_VIEW
                continue
            s, c, y0, x0, ph, pw = FAR_PATCHES[entry[0]]
            x1, y1, x2, y2 = entry[1]
            status, xa, ya, w, h = M.clip_box(entry[1], FAR_SIDE, FAR_SIDE)
            assert status <= M.CLIPPED and x0 <= xa and xa + w <= x0 + pw and y0 <= ya and ya + h <= y0 + ph
            o, g = M.crop(patches[entry[0]], (x1 - x0, y1 - y0, x2 - x0, y2 - y0), T, fill, lut)
            assert g[0] == status and g[3:5] == (w, h)
            out[r, k] = o
            geom[r, k] = (g[0], g[1] + x0, g[2] + y0) + g[3:] + (s * 3 + c,)
    return out, geom
