"""The pose head's input crops (mvm_crop_views): the normative
statement, numpy and integers only up to the look-up.  Not a test module.

One crop is defined by an image ``img`` uint8 [H, W, 3] (B, G, R), a box
(x1, y1, x2, y2), a canvas side ``T``, a fill level and a table ``lut``
float32 or float16 [3, 256]:

1. clip the box to the image (``clip_box``);
2. the resampled size, Python's round() of the double product (``sizes``);
3. the exact area resample (``area_resample``: two int64 matrix products;
   ``area_resample_loops``: the same integral written independently, per
   destination pixel over its footprint with Python integers);
4. the result placed on a T x T canvas of ``fill``;
5. ``out[c][y][x] = lut[c][canvas[y][x][2 - c]]``.

No bit equality with OpenCV's INTER_AREA is claimed: that evaluates the same
integral with float32 weights when shrinking and switches to a linear rule
when enlarging.
"""
import numpy as np

MEAN = (0.485, 0.456, 0.406)     # RGB
STD = (0.229, 0.224, 0.225)

OK, CLIPPED, EMPTY, NO_VIEW, NO_SCENE = 0, 1, 2, 3, 4


def norm_lut(mean=MEAN, std=STD, dtype=np.float32) -> np.ndarray:
    """lut[c][v] = (float32(v) / float32(255) - float32(mean[c])) / float32(std[c]),
    one IEEE float32 operation each; float16: that rounded to nearest-even once."""
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    lut = np.stack([(v - np.float32(mean[c])) / np.float32(std[c]) for c in range(3)])
    assert lut.dtype == np.float32
    return lut.astype(dtype)


def clip_box(box, H: int, W: int):
    """-> (status, xa, ya, w, h); status EMPTY has zeros after it."""
    x1, y1, x2, y2 = (int(v) for v in box)
    xa, xb = min(max(x1, 0), W), min(max(x2, 0), W)
    ya, yb = min(max(y1, 0), H), min(max(y2, 0), H)
    w, h = xb - xa, yb - ya
    if w <= 0 or h <= 0:
        return EMPTY, 0, 0, 0, 0
    moved = (xa, ya, xb, yb) != (x1, y1, x2, y2)
    return (CLIPPED if moved else OK), xa, ya, w, h


def sizes(w: int, h: int, T: int):
    """-> (new_w, new_h, dx, dy)."""
    scale = float(T) / max(h, w)
    new_w = max(1, int(round(w * scale)))
    new_h = max(1, int(round(h * scale)))
    return new_w, new_h, (T - new_w) // 2, (T - new_h) // 2


def overlaps(n_src: int, n_dst: int) -> np.ndarray:
    """int64 [n_dst, n_src]: in units of 1 / n_dst source pixels, the length of
    the overlap of destination cell [X n_src, (X + 1) n_src) with source cell
    [i n_dst, (i + 1) n_dst).  Every row sums to n_src."""
    X = np.arange(n_dst, dtype=np.int64)[:, None]
    i = np.arange(n_src, dtype=np.int64)[None, :]
    lo = np.maximum(X * n_src, i * n_dst)
    hi = np.minimum((X + 1) * n_src, (i + 1) * n_dst)
    return np.maximum(hi - lo, 0)


def area_resample(src: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """uint8 [h, w, 3] -> uint8 [new_h, new_w, 3]: the box integral of the
    piecewise-constant image over each destination pixel, rounded half up."""
    h, w = src.shape[:2]
    ox, oy = overlaps(w, new_w), overlaps(h, new_h)
    out = np.empty((new_h, new_w, 3), np.uint8)
    for c in range(3):
        s = oy @ (src[:, :, c].astype(np.int64) @ ox.T)
        out[:, :, c] = (2 * s + w * h) // (2 * w * h)
    return out


def area_resample_loops(src: np.ndarray, new_h: int, new_w: int, pixels=None) -> dict:
    """The second statement of step 3: {(Y, X): (l0, l1, l2)} for the given
    destination pixels (default all), each summed over its own footprint
    with Python integers."""
    h, w = src.shape[:2]
    if pixels is None:
        pixels = [(Y, X) for Y in range(new_h) for X in range(new_w)]
    out = {}
    for Y, X in pixels:
        s = [0, 0, 0]
        j = Y * h // new_h
        while j * new_h < (Y + 1) * h:
            oy = min((Y + 1) * h, (j + 1) * new_h) - max(Y * h, j * new_h)
            i = X * w // new_w
            while i * new_w < (X + 1) * w:
                ox = min((X + 1) * w, (i + 1) * new_w) - max(X * w, i * new_w)
                for c in range(3):
                    s[c] += oy * ox * int(src[j, i, c])
                i += 1
            j += 1
        out[(Y, X)] = tuple((2 * v + w * h) // (2 * w * h) for v in s)
    return out


def canvas(img: np.ndarray, box, T: int, fill: int):
    """Steps 1-4 -> (uint8 [T, T, 3] in the image's channel order,
    (status, xa, ya, w, h, new_w, new_h))."""
    H, W = img.shape[:2]
    cv = np.full((T, T, 3), fill, np.uint8)
    status, xa, ya, w, h = clip_box(box, H, W)
    if status == EMPTY:
        return cv, (EMPTY, 0, 0, 0, 0, 0, 0)
    new_w, new_h, dx, dy = sizes(w, h, T)
    cv[dy:dy + new_h, dx:dx + new_w] = area_resample(img[ya:ya + h, xa:xa + w], new_h, new_w)
    return cv, (status, xa, ya, w, h, new_w, new_h)


def look_up(cv: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """Step 5: [T, T, 3] levels -> [3, T, T] of the table's type; plane 0 is R,
    taken from source channel 2."""
    return np.stack([lut[c][cv[:, :, 2 - c]] for c in range(3)])


def crop(img, box, T: int, fill: int, lut):
    cv, geom = canvas(img, box, T, fill)
    return look_up(cv, lut), geom


def crop_views(images, scene, views, boxes, rows, cams, T: int, fill: int, lut, scene_base: int = 0):
    """What mvm_crop_views writes: images uint8 [S, C, H, W, 3]; scene [n],
    views [n, C] and boxes [n, C, 4] a table's; rows (begin, end); cams the
    selected cameras.  -> (out [rows, cams, 3, T, T], geom int32 [rows, cams, 8]).
    The scene is checked before the view; a slot that is not made is all fill."""
    S, C = images.shape[:2]
    b, e = rows
    out = np.empty((e - b, len(cams), 3, T, T), lut.dtype)
    geom = np.zeros((e - b, len(cams), 8), np.int32)
    blank = look_up(np.full((T, T, 3), fill, np.uint8), lut)
    memo = {}
    for r in range(b, e):
        s = int(scene[r]) - scene_base
        for k, c in enumerate(cams):
            if not 0 <= s < S:
                out[r - b, k], geom[r - b, k, 0], geom[r - b, k, 7] = blank, NO_SCENE, -1
            elif views[r, c] < 0:
                out[r - b, k], geom[r - b, k, 0] = blank, NO_VIEW
            else:
                key = (s, c) + tuple(int(v) for v in boxes[r, c])
                if key not in memo:
                    memo[key] = crop(images[s, c], boxes[r, c], T, fill, lut)
                o, g = memo[key]
                out[r - b, k] = o
                geom[r - b, k, :7] = g
                geom[r - b, k, 7] = s * C + c if g[0] <= CLIPPED else 0
    return out, geom
