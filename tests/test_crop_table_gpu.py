"""MatchTable.crops on the GPU: on the eight captures of
tests/test_extend_gpu.py with random images, the crops of every table a batch
has are tests/crop_model.py applied to ``predictions(s)``'s boxes, row by row
and camera by camera, bit for bit."""
import numpy as np
import pytest
import torch

import crop_model as M
import test_extend_gpu as TE
from bpc_baseline_amd.inference.batch_match import match_captures

pytestmark = pytest.mark.gpu
H, W, T = 1600, 2000, 16          # smaller than the rig's 2400 x 2400: some boxes are clipped, some empty
SEED = (2, 3, 4)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _images(S, C, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(318 + C)
    return torch.randint(0, 256, (S, C, H, W, 3), dtype=torch.uint8, device=dev, generator=g)


def _expected(tab, images_h, cams, lut, fill=255):
    """Per row and selected camera, from predictions(s) alone."""
    C = tab.n_cams
    n = int(tab.offs[-1])
    out = np.empty((n, len(cams), 3, T, T), lut.dtype)
    geom = np.zeros((n, len(cams), 8), np.int32)
    blank = M.look_up(np.full((T, T, 3), fill, np.uint8), lut)
    for s in range(len(tab.offs) - 1):
        for q, pred in enumerate(tab.predictions(s)):
            r = int(tab.offs[s]) + q
            kept = list(pred[3]) if C > 3 else [0, 1, 2]
            for k, c in enumerate(cams):
                if c not in kept:
                    out[r, k], geom[r, k, 0] = blank, M.NO_VIEW
                    continue
                o, g = M.crop(images_h[s, c], pred[0][kept.index(c)], T, fill, lut)
                out[r, k], geom[r, k, :7] = o, g
                geom[r, k, 7] = s * C + c if g[0] <= M.CLIPPED else 0
    return out, geom


def _check_table(tab, images, images_h, cams=None, **kw):
    before = {k: v.copy() for k, v in tab.host().items()}
    crops, geom = tab.crops(images, cams=cams, size=T, **kw)
    sel = list(range(tab.n_cams)) if cams is None else list(cams)
    dtype = kw.get("dtype", torch.float32)
    lut = M.norm_lut(dtype=np.float16 if dtype == torch.float16 else np.float32)
    w_out, w_geom = _expected(tab, images_h, sel, lut, kw.get("fill", 255))
    assert np.array_equal(geom.cpu().numpy(), w_geom)
    assert np.array_equal(_bits(crops.cpu().numpy()), _bits(w_out))
    for k in tab.fields():                                            # the table's fields are untouched
        assert np.array_equal(_bits(getattr(tab, k).cpu().numpy()), _bits(before[k])), k
    return w_geom


@pytest.mark.parametrize("C, seeds", ((3, None), (5, None), (5, [SEED])))
def test_table_crops_are_the_model_on_the_predictions(cuda, C, seeds):
    f = TE.fixture(C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    kw = dict(extra_seeds=seeds) if seeds else {}
    res = match_captures(t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs, n_cams=C, **kw)
    images = _images(f.S, C, cuda)
    images_h = images.cpu().numpy()
    tables = [res.table(reproj=True), res.table_all()] + ([res.table()] if C == 3 else [])
    assert int(tables[0].offs[-1]) >= 20
    if seeds:
        assert int(tables[1].offs[-1]) > int(tables[0].offs[-1])     # the extra pass added rows
    for tab in tables:
        geom = _check_table(tab, images, images_h)
        assert (geom[..., 0] == M.OK).sum() >= geom[..., 0].size // 4
    if C > 3:
        assert (geom[..., 0] == M.NO_VIEW).any()
    assert torch.equal(images, torch.from_numpy(images_h).to(cuda))
    # what the reference's final_rotation uses, a row range, float16 and another fill
    tab = tables[1]
    _check_table(tab, images, images_h, cams=(2,))
    _check_table(tab, images, images_h, cams=(C - 1, 0), dtype=torch.float16, fill=0)
    n = int(tab.offs[-1])
    part, pg = tab.crops(images, rows=(3, n - 2), cams=(2,), size=T)
    whole, wg = tab.crops(images, cams=(2,), size=T)
    assert torch.equal(part, whole[3:n - 2]) and torch.equal(pg, wg[3:n - 2])
