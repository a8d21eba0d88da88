"""Camera parameters and fundamental matrices (host side).

Mirrors ``bpc/inference/utils/camera_utils.py`` of the reference.  The
fundamental matrix is O(1) per camera pair and stays on the host, as in the
reference: only the O(n^2) residual work goes to the GPU.

Precision follows the reference exactly (camera_utils.py:23-46): K is float32
(load_camera_params :16), R and t arrive as float64 (``calc_pose_matrix`` puts
them in ``np.eye(4)``, data_utils.py:383-387), the skew matrix is cast to
float32 (:31-35), and the product is float64.  Because the bits depend on the
host BLAS, the parity fixtures store F as an *input* of the matcher.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Iterable, Optional, Sequence

import numpy as np

__all__ = [
    "load_camera_params",
    "capture_cameras",
    "compute_fundamental_matrix",
    "calc_pose_matrix",
    "camera_pairs",
    "fundamental_matrices",
    "fundamental_matrices_batched",
    "projection_matrices",
    "pinhole_intrinsics",
    "rig_matrices",
]


def load_camera_params(scene_dir: str, cam_ids: Iterable[str], verbose: bool = True
                       ) -> Dict[str, Dict[str, dict]]:
    """Read BOP ``scene_camera_<cam>.json`` files (camera_utils.py:6-20).

    Returns ``{cam: {'K': {im_id: f32[3,3]}, 'R': {im_id: f32[3,3]}, 't': {im_id: f32[3]}}}``
    and, like the reference, prints the last file read.
    """
    params: Dict[str, Dict[str, dict]] = {}
    cam = None
    for cam in cam_ids:
        path = os.path.join(scene_dir, f"scene_camera_{cam}.json")
        with open(path) as fh:
            records = json.load(fh)
        per_cam = {"K": {}, "R": {}, "t": {}}
        for key, rec in records.items():
            im_id = int(key)
            per_cam["K"][im_id] = np.asarray(rec["cam_K"], dtype=np.float32).reshape(3, 3)
            per_cam["R"][im_id] = np.asarray(rec["cam_R_w2c"], dtype=np.float32).reshape(3, 3)
            per_cam["t"][im_id] = np.asarray(rec["cam_t_w2c"], dtype=np.float32).reshape(-1)
        params[cam] = per_cam
    if verbose:
        print(f"Loading camera parameters from: {os.path.join(scene_dir, f'scene_camera_{cam}.json')}")
    return params


def capture_cameras(scene_dir: str, cam_ids: Sequence[str], image_ids: Sequence[int], *,
                    params: Optional[Dict[str, Dict[str, dict]]] = None, verbose: bool = False):
    """Cameras of many captures of one scene, stacked for ``match_captures``.

    What ``Capture.from_dir`` (bpc/utils/data_utils.py:399-405) builds per
    capture -- ``Ks = [K[cam][image_id]]`` (float32) and ``RTs =
    [calc_pose_matrix(R, t)]`` (float64) -- for every ``image_id`` at once,
    reading each camera's JSON once.  -> (Ks f32 [S, C, 3, 3], RTs f64 [S, C, 4, 4]).
    """
    if params is None:
        params = load_camera_params(scene_dir, cam_ids, verbose=verbose)
    S, C = len(image_ids), len(cam_ids)
    Ks = np.empty((S, C, 3, 3), np.float32)
    RTs = np.zeros((S, C, 4, 4), np.float64)
    RTs[:, :, 3, 3] = 1.0
    for c, cam in enumerate(cam_ids):
        p = params[cam]
        Ks[:, c] = np.stack([p["K"][i] for i in image_ids]) if S else Ks[:, c]
        if S:
            RTs[:, c, :3, :3] = np.stack([p["R"][i] for i in image_ids])
            RTs[:, c, :3, 3] = np.stack([p["t"][i] for i in image_ids])
    return Ks, RTs


def calc_pose_matrix(R_mat: np.ndarray, t: np.ndarray) -> np.ndarray:
    """4x4 float64 [R|t] (data_utils.py:383-387: built on ``np.eye(4)``)."""
    pose = np.eye(4)
    pose[:3, :3] = R_mat
    pose[:3, 3] = t
    return pose


def compute_fundamental_matrix(K1, R1, t1, K2, R2, t2) -> np.ndarray:
    """F mapping camera-1 points to camera-2 epipolar lines (camera_utils.py:23-46).

    ``F = K2^-T [t_rel]_x R_rel K1^-1`` with ``R_rel = R2 R1^T``,
    ``t_rel = t2 - R_rel t1``; normalised by F[2,2] when |F[2,2]| > 1e-8.
    """
    t1 = np.asarray(t1).reshape(-1)
    t2 = np.asarray(t2).reshape(-1)
    R_rel = R2 @ R1.T
    t_rel = t2 - R_rel @ t1
    # the reference builds the skew matrix as float32 (camera_utils.py:31-35)
    skew = np.zeros((3, 3), dtype=np.float32)
    skew[0, 1], skew[0, 2] = -t_rel[2], t_rel[1]
    skew[1, 0], skew[1, 2] = t_rel[2], -t_rel[0]
    skew[2, 0], skew[2, 1] = -t_rel[1], t_rel[0]
    essential = skew @ R_rel
    F = np.linalg.inv(K2).T @ essential @ np.linalg.inv(K1)
    if abs(F[2, 2]) > 1e-8:
        F /= F[2, 2]
    return F


def camera_pairs(n_cams: int) -> np.ndarray:
    """All camera pairs (a, b), a < b, in lexicographic order -> int32 [P, 2].

    For three cameras this is (0,1), (0,2), (1,2): the F12, F13, F23 of
    ``process_pose.py:157-159``.
    """
    out = [(a, b) for a in range(n_cams) for b in range(a + 1, n_cams)]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def fundamental_matrices(Ks: Sequence[np.ndarray], RTs: Sequence[np.ndarray],
                         pairs: np.ndarray) -> np.ndarray:
    """F for every listed pair of one capture -> float64 [P, 9] (row-major)."""
    out = np.empty((len(pairs), 9), dtype=np.float64)
    for p, (a, b) in enumerate(pairs):
        F = compute_fundamental_matrix(Ks[a], RTs[a][:3, :3], RTs[a][:3, 3],
                                       Ks[b], RTs[b][:3, :3], RTs[b][:3, 3])
        out[p] = np.asarray(F, dtype=np.float64).reshape(9)
    return out


def fundamental_matrices_batched(Ks: np.ndarray, RTs: np.ndarray, pairs: np.ndarray) -> np.ndarray:
    """F for every (scene, pair) at once -> float64 [S*P, 9].

    ``Ks`` float32 [S, C, 3, 3], ``RTs`` float64 [S, C, 4, 4].  Same operations,
    dtypes and order as ``compute_fundamental_matrix`` (camera_utils.py:23-46),
    vectorised over scenes and pairs with stacked matmuls; numpy evaluates a
    stacked matmul matrix by matrix, so the bits equal the per-pair function
    (tests/test_host_logic.py checks this on this host's BLAS).
    """
    Ks = np.asarray(Ks)
    RTs = np.asarray(RTs, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    a, b = pairs[:, 0], pairs[:, 1]
    RT1, RT2 = RTs[:, a], RTs[:, b]                            # [S, P, 4, 4]
    R1, R2 = RT1[..., :3, :3], RT2[..., :3, :3]
    t1, t2 = RT1[..., :3, 3], RT2[..., :3, 3]                  # [S, P, 3]
    R_rel = R2 @ np.swapaxes(R1, -1, -2)
    t_rel = t2 - (R_rel @ t1[..., None])[..., 0]
    skew = np.zeros(R_rel.shape, dtype=np.float32)
    skew[..., 0, 1], skew[..., 0, 2] = -t_rel[..., 2], t_rel[..., 1]
    skew[..., 1, 0], skew[..., 1, 2] = t_rel[..., 2], -t_rel[..., 0]
    skew[..., 2, 0], skew[..., 2, 1] = -t_rel[..., 1], t_rel[..., 0]
    essential = skew @ R_rel
    # inverse once per DISTINCT intrinsic matrix (byte-wise: identical bytes give
    # identical inverses), as rigs share K across captures
    flatK = np.ascontiguousarray(Ks, dtype=np.float32).reshape(-1, 9)
    keys = flatK.view(np.dtype((np.void, flatK.dtype.itemsize * 9))).reshape(-1)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    Kinv = np.linalg.inv(flatK[first].reshape(-1, 3, 3))[inverse.reshape(-1)].reshape(Ks.shape)
    K1inv, K2inv = Kinv[:, a], Kinv[:, b]
    F = np.swapaxes(K2inv, -1, -2) @ essential @ K1inv
    f22 = F[..., 2:3, 2:3]
    F = np.where(np.abs(f22) > 1e-8, F / np.where(np.abs(f22) > 1e-8, f22, 1.0), F)
    return np.ascontiguousarray(F.reshape(-1, 9), dtype=np.float64)


def projection_matrices(Ks: np.ndarray, RTs: np.ndarray) -> np.ndarray:
    """P = K @ RT[:3] per camera (process_pose.py:91: float32 K promoted to
    float64 by the product with the float64 RT) -> float64 [S, C, 3, 4]."""
    return np.ascontiguousarray(np.asarray(Ks) @ np.asarray(RTs, dtype=np.float64)[..., :3, :])


def pinhole_intrinsics(Ks: np.ndarray) -> np.ndarray:
    """Per matrix of ``Ks`` [..., 3, 3]: True where it has the form the device
    rig kernel inverts (include/mvmatch.h, mvm_rig_matrices): strict lower
    triangle zero, no skew, ``K[2, 2] == 1``, non-zero focal lengths."""
    K = np.asarray(Ks)
    return ((K[..., 1, 0] == 0) & (K[..., 2, 0] == 0) & (K[..., 2, 1] == 0) & (K[..., 0, 1] == 0)
            & (K[..., 2, 2] == 1) & (K[..., 0, 0] != 0) & (K[..., 1, 1] != 0))


def rig_matrices(Ks: np.ndarray, RTs: np.ndarray):
    """F (f64 [S*3, 9]) and P (f64 [S, 3, 3, 4]) of every capture, computed once
    per DISTINCT rig: captures whose K and RT bytes are identical (a static
    camera rig, as within an IPD scene) share one evaluation, so the values
    are bit-identical to evaluating each capture."""
    S = Ks.shape[0]
    kb = np.ascontiguousarray(Ks).reshape(S, -1).view(np.uint32)
    rb = np.ascontiguousarray(RTs).reshape(S, -1).view(np.uint64)
    if S > 1 and (kb == kb[0]).all() and (rb == rb[0]).all():
        first, inv = np.zeros(1, np.int64), np.zeros(S, np.int64)
    elif S > 1 and len(np.unique(rb[:, 3])) == S:   # camera 0's t_x already tells them apart
        first, inv = None, None
    elif S > 1:
        key = np.ascontiguousarray(np.concatenate([kb.view(np.uint8), rb.view(np.uint8)], axis=1))
        kv = key.view(np.dtype((np.void, key.shape[1]))).reshape(-1)
        _, first, inv = np.unique(kv, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        if len(first) == S:
            first, inv = None, None
    else:
        first, inv = None, None
    if first is None:
        return fundamental_matrices_batched(Ks, RTs, camera_pairs(3)), projection_matrices(Ks, RTs)
    Fu = fundamental_matrices_batched(Ks[first], RTs[first], camera_pairs(3)).reshape(len(first), 3, 9)
    Pu = projection_matrices(Ks[first], RTs[first])
    return np.ascontiguousarray(Fu[inv].reshape(S * 3, 9)), np.ascontiguousarray(Pu[inv])
