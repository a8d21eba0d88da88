"""MatchTable.poses on the GPU: on the eight captures of
tests/test_extend_gpu.py with random raw rotation vectors, the poses of every
table a batch has are tests/pose_model.py applied to ``predictions(s)``, row
by row, bit for bit."""
import os

import numpy as np
import pytest
import torch

import pose_model as M
import test_extend_gpu as TE
from bpc_baseline_amd.inference.batch_match import match_captures

pytestmark = pytest.mark.gpu
SEED = (2, 3, 4)
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "rot_decode.npz"))
KEYS = ("R", "pose", "rot_views", "spread", "slot_status", "row_status")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _expected(tab, raw, RTs, mode, cams, **kw):
    """Row by row, from predictions(s) alone: the views a prediction kept and its t."""
    C = tab.n_cams
    out = {k: [] for k in KEYS}
    for s in range(len(tab.offs) - 1):
        for q, pred in enumerate(tab.predictions(s)):
            r = int(tab.offs[s]) + q
            kept = list(pred[3]) if C > 3 else [0, 1, 2]
            views = np.array([[0 if c in kept else -1 for c in range(C)]], np.int32)
            one = M.fuse_rotations(raw[r:r + 1], np.array([s], np.int32), views, pred[2][None], RTs, mode,
                                   cams=list(cams), **kw)
            for k in KEYS:
                out[k].append(one[k][0])
    return {k: np.stack(v) for k, v in out.items()}


def _check_table(tab, RTs, mode, rng, cams=None, **kw):
    before = {k: v.copy() for k, v in tab.host().items()}
    n, dev = int(tab.offs[-1]), tab.scene.device
    sel = list(range(tab.n_cams)) if cams is None else list(cams)
    raw = M.random_raw(rng, n * len(sel), mode).reshape(n, len(sel), -1)
    res = tab.poses(torch.from_numpy(raw).to(dev), RTs, mode, cams=cams, **kw)
    want = _expected(tab, raw, RTs, mode, sel, **kw)
    for k in KEYS:
        assert M.same(getattr(res, k).cpu().numpy(), want[k]), k
    for k in tab.fields():                                            # the table's fields are untouched
        assert np.array_equal(_bits(getattr(tab, k).cpu().numpy()), _bits(before[k])), k
    return res, want


@pytest.mark.parametrize("C, seeds", ((3, None), (5, None), (5, [SEED])))
def test_table_poses_are_the_model_on_the_predictions(cuda, C, seeds):
    f = TE.fixture(C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    kw = dict(extra_seeds=seeds) if seeds else {}
    args = (t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs)
    res = match_captures(*args, n_cams=C, **kw)
    RTs = np.asarray(f.RTs, np.float64).reshape(f.S, C, 4, 4)
    rng = np.random.default_rng(319 + C)
    tables = [res.table(reproj=True), res.table_all()] + ([res.table()] if C == 3 else [])
    assert int(tables[0].offs[-1]) >= 20
    if seeds:
        assert int(tables[1].offs[-1]) > int(tables[0].offs[-1])     # the extra pass added rows
    for tab, mode in zip(tables, ("quat", "6d", "euler")):
        _, want = _check_table(tab, RTs, mode, rng, fuse="mean")
        assert (want["row_status"] == 0).sum() >= len(want["row_status"]) // 2
        _check_table(tab, RTs, mode, rng)                              # fuse="cam", cam=2
    if C > 3:
        assert (want["slot_status"] == M.NO_VIEW).any()
    tab = tables[1]
    _check_table(tab, RTs, "euler", rng, cams=(C - 1, 0), fuse="mean")
    _check_table(tab, RTs, "6d", rng, cams=(1, 2), fuse="cam", cam=1)
    # a row range is that part of the whole, and device RTs are the host ones
    n = int(tab.offs[-1])
    raw = torch.from_numpy(M.random_raw(rng, n, "quat").reshape(n, 1, 4)).to(cuda)
    whole = tab.poses(raw, RTs, "quat", cams=(2,))
    part = tab.poses(raw[3:n - 2].contiguous(), t(RTs), "quat", rows=(3, n - 2), cams=(2,))
    for k in KEYS:
        assert M.same(getattr(part, k).cpu().numpy(), getattr(whole, k)[3:n - 2].cpu().numpy()), k

    # refine=True: the pose's last column is the refined X
    ref = match_captures(*args, n_cams=C, refine=True, **kw)
    rtab = ref.table(reproj=True)
    m = int(rtab.offs[-1])
    got = rtab.poses(torch.from_numpy(M.random_raw(rng, m * C, "quat").reshape(m, C, 4)).to(cuda), RTs, "quat",
                     fuse="mean")
    assert torch.equal(got.pose[:, :3, 3], rtab.X) and (got.pose[:, 3] == torch.tensor([0., 0, 0, 1]).to(cuda)).all()
    rows = np.concatenate([np.arange(ref.offs[s], ref.offs[s] + ref.count[s]) for s in range(f.S)])
    assert M.same(rtab.X.cpu().numpy(), ref.X.cpu().numpy()[rows])
    assert not M.same(rtab.X.cpu().numpy(), ref.X_dlt.cpu().numpy()[rows])


def test_the_reference_chain_on_the_three_camera_table(cuda):
    """fuse="cam" with the defaults: camera 2's decoded quaternion under the
    golden rig is the reference's final_rotation, the pose its 4 x 4 layout."""
    f = TE.fixture(3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    tab = match_captures(t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs).table()
    n = int(tab.offs[-1])
    idx = (np.arange(n)[:, None] % (len(GOLDEN["quat_raw"]) // 3)) * 3 + np.arange(3)[None, :]
    assert (GOLDEN["quat_cam"][idx] == np.arange(3)[None, :]).all()
    RTs = np.tile(GOLDEN["rts"][None], (f.S, 1, 1, 1))
    res = tab.poses(t(GOLDEN["quat_raw"][idx]), RTs, "quat")
    ok = np.isfinite(GOLDEN["quat_world"][idx]).all(axis=(2, 3))
    assert ok[:, 2].sum() >= n - 1 and ((res.slot_status.cpu().numpy() == 0) == ok).all()
    pose, X = res.pose.cpu().numpy(), tab.X.cpu().numpy()
    assert np.abs(pose[:, :3, :3] - GOLDEN["quat_world"][idx[:, 2]])[ok[:, 2]].max() <= 2.0 ** -51
    assert np.abs(res.rot_views.cpu().numpy() - GOLDEN["quat_world"][idx])[ok].max() <= 2.0 ** -51
    assert (pose[:, :3, 3] == X).all() and (pose[:, 3] == [0, 0, 0, 1]).all()
    assert (res.row_status.cpu().numpy() == np.where(ok[:, 2], 0, M.NO_ROTATION)).all()
