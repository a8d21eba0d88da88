"""MatchTable.poses(syms=) on the GPU, end to end on the
hand-built captures of tests/seed_pass_model.py, whose objects are known: every
camera answers the object's rotation times a seeded symmetry, the mean under
the symmetries is tests/pose_sym_model.py's bits and scores an MSSD of float32
rounding against the ground truth, and the plain mean of the same answers does
not."""
import numpy as np
import pytest
import torch

import pose_model as P
import pose_sym_model as M
import score_model as SM
import seed_pass_model as SP
import test_extend_gpu as TE
from bpc_baseline_amd.inference.batch_match import match_captures
from test_score_table_gpu import N_OBJ, _match, object_centres, row_objects

pytestmark = pytest.mark.gpu
KEYS = ("R", "pose", "rot_views", "spread", "slot_status", "row_status", "sym_index", "sym_margin", "n_changed")
# what float32 quaternions leave of MSSD beyond the centre distance: 2.93e-6 mm at the most over the four cases
# on an MI355X (|v| <= 52 mm, 2^-24 relative per component); the smallest power of two at least twice that
ROUNDING_MM = 2.0 ** -17
MODELS = {2: (40.0, 25.0, 10.0), 4: (30.0, 30.0, 10.0)}            # box half-sizes with that fold about z


def quaternion(R):
    """Rotations f64 [n, 3, 3] -> unit quaternions (x, y, z, w) f64 [n, 4], by the largest component."""
    t = np.stack([R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2], R[:, 1, 1] - R[:, 0, 0] - R[:, 2, 2],
                  R[:, 2, 2] - R[:, 0, 0] - R[:, 1, 1], R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]], axis=1)
    q = np.empty((len(R), 4))
    for r, big in enumerate(np.argmax(t, axis=1)):
        m = R[r]
        d = 2.0 * np.sqrt(1.0 + t[r, big])
        q[r] = [(d / 4, (m[0, 1] + m[1, 0]) / d, (m[0, 2] + m[2, 0]) / d, (m[2, 1] - m[1, 2]) / d),
                ((m[0, 1] + m[1, 0]) / d, d / 4, (m[1, 2] + m[2, 1]) / d, (m[0, 2] - m[2, 0]) / d),
                ((m[0, 2] + m[2, 0]) / d, (m[1, 2] + m[2, 1]) / d, d / 4, (m[1, 0] - m[0, 1]) / d),
                ((m[2, 1] - m[1, 2]) / d, (m[0, 2] - m[2, 0]) / d, (m[1, 0] - m[0, 1]) / d, d / 4)][big]
    return q


@pytest.mark.parametrize("C, fold", ((3, 2), (3, 4), (5, 2), (5, 4)))
def test_symmetric_answers_fuse_to_the_object(cuda, C, fold):
    f = SP.captures(5)
    centres = object_centres(5)
    if C == 3:                                                        # cameras 0-2 alone: the plain three-camera table
        b3 = TE.three_cam_inputs(f)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        tab = match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5]).table()
        assert tab.views is None
        RTs = np.asarray(b3[5], np.float64).reshape(f.S, 3, 4, 4)
    else:                                                             # the view table of five cameras
        tab = _match(f, cuda, n_cams=5).table(reproj=True)
        RTs = np.asarray(f.RTs, np.float64).reshape(f.S, 5, 4, 4)
    h = tab.host()
    views = h["views"] if "views" in h else h["match"]
    n = len(h["scene"])
    rng = np.random.default_rng(100 * C + fold)
    syms = M.z_fold(fold)
    half = np.array(MODELS[fold])
    verts = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    R_obj = P.random_rotations(rng, f.S * N_OBJ).reshape(f.S, N_OBJ, 3, 3)
    gt = np.tile(np.eye(4), (f.S * N_OBJ, 1, 1))
    gt[:, :3, :3], gt[:, :3, 3] = R_obj.reshape(-1, 3, 3), centres.reshape(-1, 3)
    gt_offs = np.arange(f.S + 1, dtype=np.int64) * N_OBJ
    obj = row_objects(f, tab)
    known = obj >= 0
    assert known.sum() >= 8 * SP.N_ALL
    k = rng.integers(0, fold, (n, C))
    Rw = R_obj[h["scene"], np.maximum(obj, 0)]                        # a row of mixed views answers object 0
    raw = np.stack([quaternion(RTs[h["scene"], c, :3, :3] @ Rw @ syms[k[:, c], :3, :3]) for c in range(C)],
                   axis=1).astype(np.float32)

    fused = tab.poses(torch.from_numpy(raw).to(cuda), RTs, "quat", syms=syms)
    want = M.fuse_rotations_sym(raw, h["scene"], views, h["X"], RTs, "quat", syms)
    for key in KEYS:
        assert M.same(getattr(fused, key).cpu().numpy(), want[key]), key
    M.invariants(want)
    assert (want["row_status"][known] == 0).all() and (want["n_changed"][known] == 0).all()
    usable = want["slot_status"] == 0
    first = np.argmax(usable, axis=1)
    turned = (k - k[np.arange(n), first][:, None]) % fold                # what each view must undo
    assert (((want["sym_index"] + turned) % fold == 0) | ~usable)[known].all()

    score = tab.score(gt, gt_offs, verts=verts, syms=syms, pose=fused.pose)
    model = SM.score_poses(want["pose"], h["scene"], gt, gt_offs, verts, syms)
    for key in SM.KEYS:
        assert SM.same(getattr(score, key).cpu().numpy(), model[key]), key
    # with the rotation right up to a symmetry, what is left of MSSD is the distance of the centres
    at = (np.arange(n), np.maximum(obj, 0))
    err = np.abs(model["err"][at] - model["t_err"][at])
    print(f"C={C} fold={fold}: largest MSSD beyond the centre distance on a known row {err[known].max():.3g} mm")
    assert (err[known] < ROUNDING_MM).all()

    # the same answers through the plain mean
    plain = tab.poses(torch.from_numpy(raw).to(cuda), RTs, "quat", fuse="mean")
    perr = tab.score(gt, gt_offs, verts=verts, syms=syms, pose=plain.pose).err.cpu().numpy()
    perr = perr[np.arange(n), np.maximum(obj, 0)]
    lost = known & ~(perr <= 10.0)                                       # a NaN pose is lost too
    print(f"C={C} fold={fold}: plain mean beyond 10 mm on {lost.sum()} of {known.sum()} known rows")
    if fold == 4:                                                        # under a half turn the majority wins the sum
        assert lost.sum() >= known.sum() // 4
    mixed = np.array([len(set(k[r][usable[r]])) > 1 for r in range(n)])
    assert not (lost & ~mixed).any()

    if fold == 2:
        # an even number of views: two that answer half a turn apart leave the plain sum without a z rotation
        # (ambiguous, or whatever angle float32 rounding decides); under the symmetries they are one answer
        two = torch.from_numpy(np.ascontiguousarray(raw[:, :2])).to(cuda)
        p2 = tab.poses(two, RTs, "quat", cams=(0, 1), fuse="mean")
        s2 = tab.poses(two, RTs, "quat", cams=(0, 1), syms=syms)
        e2 = tab.score(gt, gt_offs, verts=verts, syms=syms, pose=p2.pose).err.cpu().numpy()[at]
        g2 = tab.score(gt, gt_offs, verts=verts, syms=syms, pose=s2.pose)
        both = known & (s2.slot_status.cpu().numpy() == 0).all(axis=1)
        apart = both & (k[:, 0] != k[:, 1])
        lost2 = apart & (((p2.row_status.cpu().numpy() & P.AMBIGUOUS) != 0) | ~(e2 <= 10.0))
        print(f"C={C} fold=2, cameras 0 and 1: plain mean ambiguous or beyond 10 mm on {lost2.sum()} of "
              f"{apart.sum()} rows half a turn apart")
        assert apart.sum() >= 8 and lost2.sum() >= apart.sum() // 2
        left = np.abs(g2.err.cpu().numpy()[at] - g2.t_err.cpu().numpy()[at])
        assert (s2.row_status.cpu().numpy()[both] == 0).all() and (left[both] < ROUNDING_MM).all()

    # the keyword's rules
    with pytest.raises(ValueError, match="fuse"):
        tab.poses(torch.from_numpy(raw).to(cuda), RTs, "quat", syms=syms, fuse="cam")
    with pytest.raises(ValueError, match="cam"):
        tab.poses(torch.from_numpy(raw).to(cuda), RTs, "quat", syms=syms, cam=2)
    again = tab.poses(torch.from_numpy(raw).to(cuda), RTs, "quat", syms=syms, fuse="mean", rounds=1)
    assert M.same(again.R.cpu().numpy(), M.fuse_rotations_sym(raw, h["scene"], views, h["X"], RTs, "quat", syms,
                                                              rounds=1)["R"])
