"""MatchTable.fit_boxes on the GPU: captures of known poses go
through match_captures -> table -> poses (the true rotations as the
quaternions a head would give) -> fit_boxes -> score.  The fitted poses are
tests/box_fit_model.py's bits on the table's own arrays, on every table a
batch has, and the translation error of the matched rows falls."""
import numpy as np
import pytest
import torch

import box_fit_inputs as I
import box_fit_model as M
from bpc_baseline_amd.inference.batch_match import match_captures
from bpc_baseline_amd.inference.utils.camera_utils import projection_matrices
from test_score_table_gpu import quat_of

pytestmark = pytest.mark.gpu
KEYS = ("pose", "rms", "info", "cov", "resid")


def _match(f, dev, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return match_captures(t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs, **kw)


def _row_objects(f, h, views):
    out = np.full(len(views), -1, np.int64)
    for r in range(len(views)):
        s = int(h["scene"][r])
        seen = {int(f.ident[s][c][v]) for c, v in enumerate(views[r]) if v >= 0}
        if len(seen) == 1:
            out[r] = seen.pop()
    return out


def _check_table(f, tab, dev):
    """poses -> fit_boxes -> score on one table -> (mean t_err before, after) of the matched rows."""
    h, n, C = tab.host(), int(tab.offs[-1]), f.C
    views = h["views"] if "views" in h else h["match"]
    obj = _row_objects(f, h, views)
    known = np.nonzero(obj >= 0)[0]
    assert len(known) >= f.S * 3
    raw = np.zeros((n, C, 4), np.float32)
    for r in range(n):
        s = int(h["scene"][r])
        for c in range(C):
            raw[r, c] = quat_of(f.RTs[s, c, :3, :3] @ f.R[s, max(obj[r], 0)])
    fused = tab.poses(torch.from_numpy(raw).to(dev), f.RTs, "quat", fuse="mean")
    assert (fused.row_status.cpu().numpy() == 0).all()
    pose = fused.pose.cpu().numpy()
    proj = projection_matrices(f.Ks, f.RTs)
    want = M.fit_boxes(pose, h["scene"], views, h["boxes"], proj, f.verts)
    fit = tab.fit_boxes(fused.pose, f.verts, Ks=f.Ks, RTs=f.RTs)
    for k in KEYS:
        assert M.same(getattr(fit, k).cpu().numpy(), want[k]), k
    by_proj = tab.fit_boxes(fused.pose, f.verts, proj=torch.from_numpy(proj).to(dev), cov=False, resid=False)
    assert M.same(by_proj.pose.cpu().numpy(), want["pose"]) and by_proj.cov is None and by_proj.resid is None
    part = tab.fit_boxes(fused.pose[2:n - 1].contiguous(), f.verts, proj=proj, rows=(2, n - 1), max_evals=2)
    w2 = M.fit_boxes(pose[2:n - 1], h["scene"][2:n - 1], views[2:n - 1], h["boxes"][2:n - 1], proj, f.verts, 2)
    for k in KEYS:
        assert M.same(getattr(part, k).cpu().numpy(), w2[k]), k
    # straight into score: the translation error of the matched rows
    n_obj = f.R.shape[1]
    gt = np.tile(np.eye(4), (f.S, n_obj, 1, 1))
    gt[:, :, :3, :3], gt[:, :, :3, 3] = f.R, f.t
    gt, gt_offs = gt.reshape(-1, 4, 4), np.arange(f.S + 1, dtype=np.int64) * n_obj
    before = tab.score(gt, gt_offs, verts=f.verts, pose=fused.pose).t_err.cpu().numpy()[known, obj[known]]
    after = tab.score(gt, gt_offs, verts=f.verts, pose=fit.pose).t_err.cpu().numpy()[known, obj[known]]
    model_after = np.linalg.norm(want["pose"][known, :3, 3] - f.t[h["scene"][known], obj[known]], axis=1)
    assert np.allclose(after, model_after, rtol=0, atol=1e-9)       # score's own statement of the same distance
    print(C, "rows", n, "matched", len(known), "t_err before", before.mean(), "after", after.mean())
    assert after.mean() < before.mean()
    return fit


def test_three_camera_table(cuda):
    f = I.first_three(I.captures(5))
    tab = _match(f, cuda).table()
    assert tab.views is None
    _check_table(f, tab, cuda)


def test_view_table_and_table_all(cuda):
    f = I.captures(5)
    batch = _match(f, cuda, n_cams=5)
    _check_table(f, batch.table(reproj=True), cuda)
    _check_table(f, _match(f, cuda, n_cams=5, extra_seeds=[(1, 2, 3)]).table_all(), cuda)


def test_rig_arguments(cuda):
    f = I.first_three(I.captures(5))
    tab = _match(f, cuda).table()
    n = int(tab.offs[-1])
    pose = torch.eye(4, dtype=torch.float64, device=cuda).repeat(n, 1, 1)
    proj = projection_matrices(f.Ks, f.RTs)
    for kw in (dict(), dict(proj=proj, Ks=f.Ks, RTs=f.RTs), dict(proj=proj, RTs=f.RTs), dict(Ks=f.Ks),
               dict(RTs=f.RTs)):
        with pytest.raises(ValueError, match="rig"):
            tab.fit_boxes(pose, f.verts, **kw)
    with pytest.raises(ValueError, match="pose must be"):
        tab.fit_boxes(pose[:-1], f.verts, proj=proj)
    with pytest.raises(ValueError, match="rows"):
        tab.fit_boxes(pose, f.verts, proj=proj, rows=(0, n + 1))
