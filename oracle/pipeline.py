"""CPU restatement of the steps either side of the matcher.

TEST INFRASTRUCTURE ONLY: the checker for mvm_pack_detections,
mvm_triangulate_dlt and the threshold + sort of mvm_select_triangulate
(bpc_baseline_amd/csrc/mvm_pipeline.hip).  Pinned against
tests/golden/a8_detect.npz and a9_triangulate.npz, which hold the reference's
own outputs (oracle/gen_golden.py), and (select_sort) against
oracle/lsap.match_objects on the a3 and a7 fixtures.
"""
from __future__ import annotations

import numpy as np


def detect_pack(boxes: np.ndarray, conf: np.ndarray, cls: np.ndarray, in_offs: np.ndarray,
                thresh: float, class_id: float = 0.0):
    """PoseEstimator._detect's packing (bpc/inference/process_pose.py:122-140),
    over a CSR batch of images.

    Per image: ``valid = (cls == 0) & (conf >= thresh)`` in float32 (:130; a
    Python float against a float32 array compares in float32), boxes kept in
    order, ``int()`` of each float32 coordinate (:134, toward zero), centre
    ``0.5 * (x1 + x2)`` as float64 (:135-136).
    -> (bbox int64 [k, 4], center f64 [k, 2], out_offs int64 [n_img + 1]).
    """
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    conf = np.asarray(conf, np.float32)
    cls = np.asarray(cls, np.float32)
    in_offs = np.asarray(in_offs, np.int64)
    t32 = np.float32(thresh)
    bbox, center, counts = [], [], []
    for k in range(in_offs.size - 1):
        b, e = int(in_offs[k]), int(in_offs[k + 1])
        valid = (cls[b:e] == np.float32(class_id)) & (conf[b:e] >= t32)
        kept = boxes[b:e][valid]
        q = np.trunc(kept.astype(np.float64)).astype(np.int64)
        bbox.append(q)
        center.append(np.stack([0.5 * (q[:, 0] + q[:, 2]), 0.5 * (q[:, 1] + q[:, 3])], axis=1)
                      .astype(np.float64))
        counts.append(q.shape[0])
    out_offs = np.zeros(len(counts) + 1, np.int64)
    out_offs[1:] = np.cumsum(counts)
    return (np.concatenate(bbox).reshape(-1, 4) if bbox else np.zeros((0, 4), np.int64),
            np.concatenate(center).reshape(-1, 2) if center else np.zeros((0, 2)),
            out_offs)


def select_sort(cube_flat: np.ndarray, M: int, P: int, row_ind: np.ndarray, col_ind: np.ndarray,
                threshold: float):
    """The tail of PoseEstimator._match before triangulation
    (process_pose.py:182-183 with match_objects, epipolar_matching.py:110-115):
    the checker for mvm_select_triangulate's match and cost outputs.

    Assignment m of the flattened (N*M, P) float32 cube is kept iff
    ``float(np.float32(v_m)) < float(threshold)``: an explicit float64 compare,
    the contract of include/mvmatch.h, whatever the installed NumPy would
    promote a float32 scalar against a Python number to.  A pair (r, c) with r
    outside [0, N*M) or c outside [0, P) is dropped first.  Kept entries are
    decoded ``i = r // M, j = r % M, k = c`` and ordered by a stable sort of
    their float32 costs (Python's sorted: ties keep the assignment's order).
    -> (match int32 [k, 3], cost float32 [k]).
    """
    cube_flat = np.asarray(cube_flat, np.float32).reshape(-1)
    r = np.asarray(row_ind, np.int64).reshape(-1)
    c = np.asarray(col_ind, np.int64).reshape(-1)
    # a pair that is no index of the (N*M, P) problem is ignored (a failed
    # assignment's region holds whatever it held before)
    ok = (r >= 0) & (r < cube_flat.size // P) & (c >= 0) & (c < P) if P > 0 else np.zeros(r.size, bool)
    r, c = r[ok], c[ok]
    if r.size == 0:
        return np.zeros((0, 3), np.int32), np.zeros(0, np.float32)
    v = cube_flat[r * P + c]
    keep = v.astype(np.float64) < float(threshold)      # NaN on either side: dropped
    r, c, v = r[keep], c[keep], v[keep]
    order = np.argsort(v, kind="stable")
    r, c = r[order], c[order]
    return np.stack([r // M, r % M, c], axis=1).astype(np.int32).reshape(-1, 3), v[order]


def triangulate(proj: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """triangulate_multi_view (bpc/inference/epipolar_matching.py:118-127) for
    a stack of systems: proj [n, V, 3, 4], pts [n, V, 2] -> X [n, 3].

    A row pair per view ``x * P[2] - P[0]``, ``y * P[2] - P[1]``; X is the last
    row of Vt from numpy's SVD, returned as X[:3] / X[3].
    """
    proj = np.asarray(proj, np.float64)
    pts = np.asarray(pts, np.float64)
    n, V = proj.shape[:2]
    A = np.empty((n, 2 * V, 4))
    A[:, 0::2] = pts[:, :, 0:1] * proj[:, :, 2] - proj[:, :, 0]
    A[:, 1::2] = pts[:, :, 1:2] * proj[:, :, 2] - proj[:, :, 1]
    X = np.empty((n, 3))
    for q in range(n):
        _, _, Vt = np.linalg.svd(A[q])
        X[q] = Vt[-1][:3] / Vt[-1][3]
    return X
