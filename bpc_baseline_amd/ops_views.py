"""The ops on the views of a C-camera batch over the C ABI
(``torch.ops.mvmatch_views.*``).

``bpc_baseline_amd.ops`` keeps its frozen op surface (``mvmatch::*_out``); the
ops that act on the views of a C-camera batch after the fact register here,
under a namespace of their own, with the same boundary layer: spec rows checked
by ``ops._check_args``, the C entry point through ``ops._call``, and the shared
fake that returns None.

  mvmatch_views::prune_views_out       mvm_prune_views_triangulate
  mvmatch_views::mark_used_out         mvm_mark_used               
  mvmatch_views::leftover_counts_out   mvm_leftover_counts
  mvmatch_views::leftover_gather_out   mvm_leftover_gather
  mvmatch_views::refine_points_out     mvm_refine_points           
  mvmatch_views::crop_views_out        mvm_crop_views              
  mvmatch_views::fuse_rotations_out    mvm_fuse_rotations          
  mvmatch_views::score_poses_out       mvm_score_poses             
  mvmatch_views::match_scores_out      mvm_match_scores
  mvmatch_views::fuse_rotations_sym_out  mvm_fuse_rotations_sym    
  mvmatch_views::fit_boxes_out         mvm_fit_boxes               
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _native, ops
from .ops import ANY, AT_LEAST, EXACT, f32, f64, i32, i64, u8

__all__ = ["prune_views", "seed_order", "mark_used", "leftover_counts", "leftover_gather", "refine_points",
           "norm_lut", "crop_views", "fuse_rotations", "FusedRotations", "score_poses", "match_scores",
           "recall_precision", "PoseScores", "fuse_rotations_sym", "SymFusedRotations", "fit_boxes", "BoxFit"]

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)     # RGB
CROP_MAX_SIZE, CROP_MAX_IMAGE = 1024, 16384
_CROP_KINDS = {torch.float32: 0, torch.float16: 1}
ROTATION_MODES = {"euler": (0, 3), "quat": (1, 4), "6d": (2, 6)}     # name -> (code, values per slot)
ROTATION_FUSE = {"cam": 0, "mean": 1}
SLOT_NO_VIEW, SLOT_NO_CAPTURE, SLOT_DEGENERATE = 1, 2, 4              # FusedRotations.slot_status
SLOT_NO_SYM = 8                                                       # SymFusedRotations.slot_status only
SYM_MAX_ROUNDS = 4
ROW_NO_ROTATION, ROW_AMBIGUOUS = 1, 2                                 # FusedRotations.row_status
SYM_PADDING, SYM_NO_CAPTURE, SYM_NOT_FINITE = -1, -2, -3              # PoseScores.sym below 0
SCORE_MAX_SYMS, SCORE_MAX_THRESHOLDS, SCORE_MAX_MATCH_GT = 64, 16, 1024
SCORE_POSE_MAX = 2.0 ** 200


def _check_gate(gate) -> float:
    gate = float(gate)
    if math.isnan(gate) or gate < 0.0:
        raise ValueError(f"gate: expected a number of pixels >= 0 (or +inf), got {gate}")
    return gate


@ops._gpu_op("prune_views_out", ("views", "ext_cost", "X", "pruned"), namespace="mvmatch_views")
def prune_views_out(views: Tensor, ext_cost: Tensor, X: Tensor, match_offs: Tensor, count: Tensor,
                    pts: Tensor, cam_offs: Tensor, proj: Tensor, gate: float, n_cams: int,
                    pruned: Tensor) -> None:
    """Drop the extra views whose reprojection residual exceeds ``gate``, worst
    first and one at a time, and triangulate each affected match again
    (mvm_prune_views_triangulate).  ``views`` / ``ext_cost`` / ``X`` are
    in/out, ``pruned`` out."""
    dev = ops._gpu(views, "views", "view pruning")
    if not 4 <= n_cams <= _native.MVM_MAX_CAMS:
        raise ValueError(f"n_cams: expected 4..{_native.MVM_MAX_CAMS}, got {n_cams}")
    if views.dim() != 2 or views.shape[1] != n_cams:
        raise ValueError(f"views must be [cap, {n_cams}]")
    gate = _check_gate(gate)
    cap, n_scenes = int(views.shape[0]), count.numel()
    ops._check_args(dev, [(views, "views", i32, n_cams * cap, AT_LEAST),
                          (ext_cost, "ext_cost", f32, (n_cams - 3) * cap, AT_LEAST),
                          (X, "X", f64, 3 * cap, AT_LEAST),
                          (match_offs, "match_offs", i64, n_scenes + 1, EXACT),
                          (count, "count", i32, n_scenes, EXACT), (pts, "pts", f64, None, ANY),
                          (cam_offs, "cam_offs", i64, n_cams * n_scenes + 1, EXACT),
                          (proj, "proj", f64, 12 * n_cams * n_scenes, EXACT),
                          (pruned, "pruned", i32, cap, AT_LEAST)])
    if n_scenes == 0 or cap == 0 or pts.numel() == 0:
        return                       # no match a capture could hold: nothing to launch
    ops._call("mvm_prune_views_triangulate", ops._p(match_offs), ops._p(count), n_scenes, n_cams,
              ops._p(pts), ops._p(cam_offs), ops._p(proj), gate, ops._p(views), ops._p(ext_cost),
              ops._p(X), ops._p(pruned), ops._stream(views))


def _check_seed(seed, n_cams: int) -> tuple:
    """A seed triple of ``n_cams`` cameras as three ints, or ValueError."""
    if not 4 <= int(n_cams) <= _native.MVM_MAX_CAMS:
        raise ValueError(f"n_cams: expected 4..{_native.MVM_MAX_CAMS}, got {n_cams}")
    try:
        seed = tuple(int(c) for c in seed)
    except TypeError:
        raise ValueError(f"seed: expected three cameras, got {seed!r}") from None
    if len(seed) != 3 or len(set(seed)) != 3 or not all(0 <= c < n_cams for c in seed):
        raise ValueError(f"seed: expected three distinct cameras < {n_cams}, got {seed}")
    return seed


def seed_order(seed, n_cams: int) -> tuple:
    """The camera order of a seed pass: the triple, then the other cameras ascending."""
    seed = _check_seed(seed, n_cams)
    return seed + tuple(c for c in range(int(n_cams)) if c not in seed)


@ops._gpu_op("mark_used_out", ("used",), namespace="mvmatch_views")
def mark_used_out(views: Tensor, match_offs: Tensor, count: Tensor, n_cams: int, seed: List[int],
                  sub_cam_offs: Optional[Tensor], orig: Optional[Tensor], cam_offs: Tensor,
                  used: Tensor) -> None:
    """used[detection] = 1 for every detection a match row holds (mvm_mark_used)."""
    dev = ops._gpu(views, "views", "leftover marking")
    seed = _check_seed(seed, n_cams)
    if views.dim() != 2 or views.shape[1] != n_cams:
        raise ValueError(f"views must be [cap, {n_cams}]")
    if (sub_cam_offs is None) != (orig is None):
        raise ValueError("sub_cam_offs and orig go together")
    cap, n_scenes = int(views.shape[0]), count.numel()
    rows = [(views, "views", i32, n_cams * cap, EXACT), (match_offs, "match_offs", i64, n_scenes + 1, EXACT),
            (count, "count", i32, n_scenes, EXACT), (cam_offs, "cam_offs", i64, n_cams * n_scenes + 1, EXACT),
            (used, "used", i32, None, ANY)]
    if orig is not None:
        rows += [(sub_cam_offs, "sub_cam_offs", i64, n_cams * n_scenes + 1, EXACT), (orig, "orig", i32, None, ANY)]
    ops._check_args(dev, rows)
    if n_scenes == 0 or cap == 0 or used.numel() == 0 or (orig is not None and orig.numel() == 0):
        return                       # no row, or no detection a row could hold
    ops._call("mvm_mark_used", ops._p(views), ops._p(match_offs), ops._p(count), cap, n_scenes, n_cams,
              *seed, ops._p(sub_cam_offs), ops._p(orig), ops._p(cam_offs), used.numel(), ops._p(used),
              ops._stream(views))


@ops._gpu_op("leftover_counts_out", ("counts",), namespace="mvmatch_views")
def leftover_counts_out(used: Tensor, cam_offs: Tensor, n_cams: int, seed: List[int], counts: Tensor) -> None:
    """The unused detections per (capture, slot) of the seed's camera order
    (mvm_leftover_counts)."""
    dev = ops._gpu(cam_offs, "cam_offs", "leftover count")
    seed = _check_seed(seed, n_cams)
    n_views = cam_offs.numel() - 1
    if n_views < 0 or n_views % n_cams:
        raise ValueError(f"cam_offs must describe {n_cams} views per capture")
    ops._check_args(dev, [(used, "used", i32, None, ANY), (cam_offs, "cam_offs", i64, n_views + 1, EXACT),
                          (counts, "counts", i32, n_views, EXACT)])
    if n_views == 0:
        return
    if used.numel() == 0:            # every view is empty: nothing to read
        counts.zero_()
        return
    ops._call("mvm_leftover_counts", ops._p(used), ops._p(cam_offs), n_views // n_cams, n_cams, *seed,
              ops._p(counts), ops._stream(cam_offs))


@ops._gpu_op("leftover_gather_out", ("pts_out", "boxes_out", "orig_out"), namespace="mvmatch_views")
def leftover_gather_out(used: Tensor, pts: Tensor, boxes: Tensor, cam_offs: Tensor, sub_cam_offs: Tensor,
                        n_cams: int, seed: List[int], pts_out: Tensor, boxes_out: Tensor,
                        orig_out: Tensor) -> None:
    """The unused detections, compacted per view in the seed's camera order
    (mvm_leftover_gather)."""
    dev = ops._gpu(used, "used", "leftover gather")
    seed = _check_seed(seed, n_cams)
    n_views = cam_offs.numel() - 1
    if n_views < 0 or n_views % n_cams:
        raise ValueError(f"cam_offs must describe {n_cams} views per capture")
    n, m = used.numel(), orig_out.numel()
    ops._check_args(dev, [(used, "used", i32, None, ANY), (pts, "pts", f64, 2 * n, EXACT),
                          (boxes, "boxes", i32, 4 * n, EXACT), (cam_offs, "cam_offs", i64, n_views + 1, EXACT),
                          (sub_cam_offs, "sub_cam_offs", i64, n_views + 1, EXACT),
                          (pts_out, "pts_out", f64, 2 * m, EXACT), (boxes_out, "boxes_out", i32, 4 * m, EXACT),
                          (orig_out, "orig_out", i32, None, ANY)])
    if n_views == 0 or n == 0 or m == 0:
        return                       # nothing left over: nothing to launch
    ops._call("mvm_leftover_gather", ops._p(used), ops._p(pts), ops._p(boxes), ops._p(cam_offs),
              ops._p(sub_cam_offs), n_views // n_cams, n_cams, *seed, ops._p(pts_out), ops._p(boxes_out),
              ops._p(orig_out), ops._stream(used))


def _check_max_evals(max_evals) -> int:
    if isinstance(max_evals, bool) or not isinstance(max_evals, int) or not 1 <= max_evals <= 64:
        raise ValueError(f"max_evals: expected an int in 1..64, got {max_evals!r}")
    return max_evals


@ops._gpu_op("refine_points_out", ("X_out", "rms", "info", "cov"), namespace="mvmatch_views")
def refine_points_out(views: Tensor, X: Tensor, match_offs: Tensor, count: Tensor, pts: Tensor,
                      cam_offs: Tensor, proj: Tensor, n_cams: int, max_evals: int, X_out: Tensor,
                      rms: Tensor, info: Tensor, cov: Optional[Tensor]) -> None:
    """Refine every match's point by its reprojection error and give its
    covariance (mvm_refine_points).  ``views`` / ``X`` are read only; ``X_out``
    / ``rms`` / ``info`` / ``cov`` (None: not computed) out."""
    dev = ops._gpu(views, "views", "point refinement")
    if not 3 <= n_cams <= _native.MVM_MAX_CAMS:
        raise ValueError(f"n_cams: expected 3..{_native.MVM_MAX_CAMS}, got {n_cams}")
    if views.dim() != 2 or views.shape[1] != n_cams:
        raise ValueError(f"views must be [cap, {n_cams}]")
    max_evals = _check_max_evals(max_evals)
    cap, n_scenes = int(views.shape[0]), count.numel()
    rows = [(views, "views", i32, n_cams * cap, AT_LEAST), (X, "X", f64, 3 * cap, AT_LEAST),
            (match_offs, "match_offs", i64, n_scenes + 1, EXACT), (count, "count", i32, n_scenes, EXACT),
            (pts, "pts", f64, None, ANY), (cam_offs, "cam_offs", i64, n_cams * n_scenes + 1, EXACT),
            (proj, "proj", f64, 12 * n_cams * n_scenes, EXACT), (X_out, "X_out", f64, 3 * cap, AT_LEAST),
            (rms, "rms", f64, 2 * cap, AT_LEAST), (info, "info", i32, 2 * cap, AT_LEAST)]
    if cov is not None:
        rows.append((cov, "cov", f64, 6 * cap, AT_LEAST))
    ops._check_args(dev, rows)
    if X_out.data_ptr() == X.data_ptr() and cap:
        raise ValueError("X_out must not be X: the input is kept")
    if n_scenes == 0 or cap == 0 or pts.numel() == 0:
        return                       # no match a capture could hold: nothing to launch
    ops._call("mvm_refine_points", ops._p(match_offs), ops._p(count), n_scenes, n_cams, ops._p(pts),
              ops._p(cam_offs), ops._p(proj), ops._p(views), ops._p(X), max_evals, ops._p(X_out),
              ops._p(rms), ops._p(info), ops._p(cov), ops._stream(views))


@ops._gpu_op("crop_views_out", ("out", "geom"), namespace="mvmatch_views")
def crop_views_out(images: Tensor, scene: Tensor, views: Tensor, boxes: Tensor, n_cams: int, scene_base: int,
                   row0: int, n_rows: int, cams: List[int], size: int, fill: int, lut: Tensor, out: Tensor,
                   geom: Optional[Tensor]) -> None:
    """The crops of rows ``row0 : row0 + n_rows`` in the cameras ``cams``
    (mvm_crop_views).  ``images`` / ``scene`` / ``views`` / ``boxes`` / ``lut``
    are read only; ``out`` / ``geom`` (None: not written) out."""
    dev = ops._gpu(images, "images", "crop kernel")
    if not 3 <= n_cams <= _native.MVM_MAX_CAMS:
        raise ValueError(f"n_cams: expected 3..{_native.MVM_MAX_CAMS}, got {n_cams}")
    if images.dim() != 5 or images.shape[1] != n_cams or images.shape[4] != 3:
        raise ValueError(f"images must be [S, {n_cams}, H, W, 3], got {tuple(images.shape)}")
    S, H, W = int(images.shape[0]), int(images.shape[2]), int(images.shape[3])
    if not (1 <= H <= CROP_MAX_IMAGE and 1 <= W <= CROP_MAX_IMAGE):
        raise ValueError(f"images: expected 1..{CROP_MAX_IMAGE} rows and columns, got {H} x {W}")
    if not 1 <= size <= CROP_MAX_SIZE:
        raise ValueError(f"size: expected 1..{CROP_MAX_SIZE}, got {size}")
    if not 0 <= fill <= 255:
        raise ValueError(f"fill: expected 0..255, got {fill}")
    if not 1 <= len(cams) <= n_cams or not all(0 <= c < n_cams for c in cams):
        raise ValueError(f"cams: expected 1..{n_cams} cameras < {n_cams}, got {list(cams)}")
    if row0 < 0 or n_rows < 0:
        raise ValueError(f"rows: expected 0 <= begin <= end, got ({row0}, {row0 + n_rows})")
    if out.dtype not in _CROP_KINDS:
        raise ValueError(f"out: expected torch.float32 or torch.float16, got {out.dtype}")
    n_end, n_slots = row0 + n_rows, n_rows * len(cams)
    rows = [(images, "images", u8, S * n_cams * H * W * 3, EXACT), (scene, "scene", i32, n_end, AT_LEAST),
            (views, "views", i32, n_cams * n_end, AT_LEAST), (boxes, "boxes", i32, 4 * n_cams * n_end, AT_LEAST),
            (lut, "lut", out.dtype, 3 * 256, EXACT), (out, "out", out.dtype, 3 * size * size * n_slots, EXACT)]
    if geom is not None:
        rows.append((geom, "geom", i32, 8 * n_slots, EXACT))
    ops._check_args(dev, rows)
    if n_rows == 0:
        return                       # no row: nothing to launch
    if S == 0:
        raise ValueError("images holds no capture")
    ops._call("mvm_crop_views", ops._p(images), S, n_cams, H, W, ops._p(scene), scene_base, ops._p(views),
              ops._p(boxes), row0, n_rows, (ctypes.c_int32 * len(cams))(*cams), len(cams), size, fill,
              ops._p(lut), _CROP_KINDS[out.dtype], ops._p(out), ops._p(geom), ops._stream(images))


@ops._gpu_op("fuse_rotations_out", ("rot_views", "R", "pose", "spread", "slot_status", "row_status"),
             namespace="mvmatch_views")
def fuse_rotations_out(raw: Tensor, scene: Tensor, views: Tensor, X: Tensor, RTs: Tensor, n_cams: int,
                       scene_base: int, row0: int, n_rows: int, cams: List[int], mode: str, fuse: str,
                       fuse_cam: int, rot_views: Optional[Tensor], R: Tensor, pose: Tensor,
                       spread: Optional[Tensor], slot_status: Tensor, row_status: Tensor) -> None:
    """The rotation head's raw outputs of rows ``row0 : row0 + n_rows`` in the
    cameras ``cams``, decoded, taken to the world and fused into a pose per row
    (mvm_fuse_rotations).  ``raw`` / ``scene`` / ``views`` / ``X`` / ``RTs`` are
    read only; ``rot_views`` / ``spread`` (None: not written) and the others out."""
    dev = ops._gpu(raw, "raw", "rotation kernel")
    if not 3 <= n_cams <= _native.MVM_MAX_CAMS:
        raise ValueError(f"n_cams: expected 3..{_native.MVM_MAX_CAMS}, got {n_cams}")
    if mode not in ROTATION_MODES:
        raise ValueError(f"mode: expected one of {sorted(ROTATION_MODES)}, got {mode!r}")
    if fuse not in ROTATION_FUSE:
        raise ValueError(f"fuse: expected one of {sorted(ROTATION_FUSE)}, got {fuse!r}")
    if not 1 <= len(cams) <= n_cams or not all(0 <= c < n_cams for c in cams):
        raise ValueError(f"cams: expected 1..{n_cams} cameras < {n_cams}, got {list(cams)}")
    if fuse == "cam" and fuse_cam not in cams:
        raise ValueError(f"cam: camera {fuse_cam} is not among the selected cameras {list(cams)}")
    if row0 < 0 or n_rows < 0:
        raise ValueError(f"rows: expected 0 <= begin <= end, got ({row0}, {row0 + n_rows})")
    if RTs.dim() != 4 or tuple(RTs.shape[1:]) != (n_cams, 4, 4):
        raise ValueError(f"RTs must be [S, {n_cams}, 4, 4], got {tuple(RTs.shape)}")
    (code, D), S = ROTATION_MODES[mode], int(RTs.shape[0])
    n_end, n_slots = row0 + n_rows, n_rows * len(cams)
    rows = [(raw, "raw", f32, D * n_slots, EXACT), (scene, "scene", i32, n_end, AT_LEAST),
            (views, "views", i32, n_cams * n_end, AT_LEAST), (X, "X", f64, 3 * n_end, AT_LEAST),
            (RTs, "RTs", f64, 16 * n_cams * S, EXACT), (R, "R", f64, 9 * n_rows, EXACT),
            (pose, "pose", f64, 16 * n_rows, EXACT), (slot_status, "slot_status", i32, n_slots, EXACT),
            (row_status, "row_status", i32, n_rows, EXACT)]
    if rot_views is not None:
        rows.append((rot_views, "rot_views", f64, 9 * n_slots, EXACT))
    if spread is not None:
        rows.append((spread, "spread", f64, n_slots, EXACT))
    ops._check_args(dev, rows)
    if n_rows == 0:
        return                       # no row: nothing to launch
    if S == 0:
        raise ValueError("RTs holds no capture")
    ops._call("mvm_fuse_rotations", ops._p(raw), D, ops._p(scene), scene_base, ops._p(views), ops._p(X),
              ops._p(RTs), S, n_cams, row0, n_rows, (ctypes.c_int32 * len(cams))(*cams), len(cams), code,
              ROTATION_FUSE[fuse], fuse_cam, ops._p(rot_views), ops._p(R), ops._p(pose), ops._p(spread),
              ops._p(slot_status), ops._p(row_status), ops._stream(raw))


@ops._gpu_op("fuse_rotations_sym_out", ("rot_views", "R", "pose", "spread", "slot_status", "row_status", "sym_index",
                                        "sym_margin", "n_changed"), namespace="mvmatch_views")
def fuse_rotations_sym_out(raw: Tensor, scene: Tensor, views: Tensor, X: Tensor, RTs: Tensor, syms: Tensor,
                           n_cams: int, scene_base: int, row0: int, n_rows: int, cams: List[int], mode: str,
                           rounds: int, rot_views: Optional[Tensor], R: Tensor, pose: Tensor,
                           spread: Optional[Tensor], slot_status: Tensor, row_status: Tensor, sym_index: Tensor,
                           sym_margin: Optional[Tensor], n_changed: Optional[Tensor]) -> None:
    """``fuse_rotations_out``'s mean taken under the symmetries ``syms`` f64
    [K, 4, 4], in ``rounds`` rounds (mvm_fuse_rotations_sym).  The inputs are
    read only; ``rot_views`` / ``spread`` / ``sym_margin`` / ``n_changed``
    (None: not written) and the others out."""
    dev = ops._gpu(raw, "raw", "rotation kernel")
    if not 3 <= n_cams <= _native.MVM_MAX_CAMS:
        raise ValueError(f"n_cams: expected 3..{_native.MVM_MAX_CAMS}, got {n_cams}")
    if mode not in ROTATION_MODES:
        raise ValueError(f"mode: expected one of {sorted(ROTATION_MODES)}, got {mode!r}")
    if not 1 <= rounds <= SYM_MAX_ROUNDS:
        raise ValueError(f"rounds: expected 1..{SYM_MAX_ROUNDS}, got {rounds}")
    if not 1 <= len(cams) <= n_cams or not all(0 <= c < n_cams for c in cams):
        raise ValueError(f"cams: expected 1..{n_cams} cameras < {n_cams}, got {list(cams)}")
    if row0 < 0 or n_rows < 0:
        raise ValueError(f"rows: expected 0 <= begin <= end, got ({row0}, {row0 + n_rows})")
    if RTs.dim() != 4 or tuple(RTs.shape[1:]) != (n_cams, 4, 4):
        raise ValueError(f"RTs must be [S, {n_cams}, 4, 4], got {tuple(RTs.shape)}")
    if syms.dim() != 3 or tuple(syms.shape[1:]) != (4, 4) or syms.shape[0] < 1:
        raise ValueError(f"syms must be [K, 4, 4] with K >= 1, got {tuple(syms.shape)}")
    (code, D), S, K = ROTATION_MODES[mode], int(RTs.shape[0]), int(syms.shape[0])
    n_end, n_slots = row0 + n_rows, n_rows * len(cams)
    rows = [(raw, "raw", f32, D * n_slots, EXACT), (scene, "scene", i32, n_end, AT_LEAST),
            (views, "views", i32, n_cams * n_end, AT_LEAST), (X, "X", f64, 3 * n_end, AT_LEAST),
            (RTs, "RTs", f64, 16 * n_cams * S, EXACT), (syms, "syms", f64, 16 * K, EXACT),
            (R, "R", f64, 9 * n_rows, EXACT), (pose, "pose", f64, 16 * n_rows, EXACT),
            (slot_status, "slot_status", i32, n_slots, EXACT), (row_status, "row_status", i32, n_rows, EXACT),
            (sym_index, "sym_index", i32, n_slots, EXACT)]
    for t, name, dt, size in ((rot_views, "rot_views", f64, 9 * n_slots), (spread, "spread", f64, n_slots),
                              (sym_margin, "sym_margin", f64, n_slots), (n_changed, "n_changed", i32, n_rows)):
        if t is not None:
            rows.append((t, name, dt, size, EXACT))
    ops._check_args(dev, rows)
    if n_rows == 0:
        return                       # no row: nothing to launch
    if S == 0:
        raise ValueError("RTs holds no capture")
    ops._call("mvm_fuse_rotations_sym", ops._p(raw), D, ops._p(scene), scene_base, ops._p(views), ops._p(X),
              ops._p(RTs), S, n_cams, row0, n_rows, (ctypes.c_int32 * len(cams))(*cams), len(cams), code,
              ops._p(syms), K, rounds, ops._p(rot_views), ops._p(R), ops._p(pose), ops._p(spread),
              ops._p(slot_status), ops._p(row_status), ops._p(sym_index), ops._p(sym_margin), ops._p(n_changed),
              ops._stream(raw))


@ops._gpu_op("score_poses_out", ("err", "sym", "t_err", "rot_cos"), namespace="mvmatch_views")
def score_poses_out(pose: Tensor, scene: Tensor, gt_pose: Tensor, gt_offs: Tensor, verts: Tensor, syms: Tensor,
                    scene_base: int, g_max: int, row0: int, n_rows: int, err: Tensor, sym: Tensor,
                    t_err: Optional[Tensor], rot_cos: Optional[Tensor]) -> None:
    """The pose error of rows ``row0 : row0 + n_rows`` against every
    ground-truth object of their capture (mvm_score_poses).  ``pose`` /
    ``scene`` / ``gt_pose`` / ``gt_offs`` / ``verts`` / ``syms`` are read only
    (``gt_offs`` is trusted: non-decreasing and within ``gt_pose``); ``err`` /
    ``sym`` and ``t_err`` / ``rot_cos`` (None: not written) out."""
    dev = ops._gpu(pose, "pose", "pose scorer")
    if row0 < 0 or n_rows < 0:
        raise ValueError(f"rows: expected 0 <= begin <= end, got ({row0}, {row0 + n_rows})")
    if g_max < 1:
        raise ValueError(f"g_max: expected at least 1, got {g_max}")
    if pose.dim() != 3 or tuple(pose.shape[1:]) != (4, 4):
        raise ValueError(f"pose must be [n, 4, 4], got {tuple(pose.shape)}")
    if gt_pose.dim() != 3 or tuple(gt_pose.shape[1:]) != (4, 4):
        raise ValueError(f"gt_pose must be [G, 4, 4], got {tuple(gt_pose.shape)}")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise ValueError(f"verts must be [V, 3] with V >= 1, got {tuple(verts.shape)}")
    if syms.dim() != 3 or tuple(syms.shape[1:]) != (4, 4) or not 1 <= syms.shape[0] <= SCORE_MAX_SYMS:
        raise ValueError(f"syms must be [K, 4, 4] with 1 <= K <= {SCORE_MAX_SYMS}, got {tuple(syms.shape)}")
    if gt_offs.numel() < 1:
        raise ValueError("gt_offs: expected one entry per capture and one more")
    n_end, n_out, S = row0 + n_rows, n_rows * g_max, gt_offs.numel() - 1
    rows = [(pose, "pose", f64, 16 * n_end, AT_LEAST), (scene, "scene", i32, n_end, AT_LEAST),
            (gt_pose, "gt_pose", f64, None, ANY), (gt_offs, "gt_offs", i64, S + 1, EXACT),
            (verts, "verts", f64, None, ANY), (syms, "syms", f64, None, ANY),
            (err, "err", f64, n_out, EXACT), (sym, "sym", i32, n_out, EXACT)]
    if t_err is not None:
        rows.append((t_err, "t_err", f64, n_out, EXACT))
    if rot_cos is not None:
        rows.append((rot_cos, "rot_cos", f64, n_out, EXACT))
    ops._check_args(dev, rows)
    if n_rows == 0:
        return                       # no row: nothing to launch
    if gt_pose.shape[0] == 0:
        raise ValueError("gt_pose holds no pose")
    ops._call("mvm_score_poses", ops._p(pose), ops._p(scene), scene_base, ops._p(gt_pose), ops._p(gt_offs), S,
              g_max, ops._p(verts), int(verts.shape[0]), ops._p(syms), int(syms.shape[0]), row0, n_rows,
              ops._p(err), ops._p(sym), ops._p(t_err), ops._p(rot_cos), ops._stream(pose))


@ops._gpu_op("match_scores_out", ("gt_index", "tp"), namespace="mvmatch_views")
def match_scores_out(err: Tensor, row_offs: Tensor, gt_offs: Tensor, thresholds: List[float], gt_index: Tensor,
                     tp: Tensor) -> None:
    """Every capture's rows matched greedily to its ground truth, once per
    threshold (mvm_match_scores).  ``err`` / ``row_offs`` / ``gt_offs`` are
    read only; ``gt_index`` / ``tp`` out."""
    dev = ops._gpu(err, "err", "score matcher")
    if err.dim() != 2:
        raise ValueError(f"err must be [n, g_max], got {tuple(err.shape)}")
    n, g_max, T, S = int(err.shape[0]), int(err.shape[1]), len(thresholds), row_offs.numel() - 1
    if not 1 <= g_max <= SCORE_MAX_MATCH_GT:
        raise ValueError(f"err: expected 1..{SCORE_MAX_MATCH_GT} ground-truth columns (g_max), got {g_max}")
    if not 1 <= T <= SCORE_MAX_THRESHOLDS:
        raise ValueError(f"thresholds: expected 1..{SCORE_MAX_THRESHOLDS} values, got {T}")
    if any(math.isnan(v) for v in thresholds):
        raise ValueError("thresholds: a NaN is no threshold")
    if S < 0:
        raise ValueError("row_offs: expected one entry per capture and one more")
    ops._check_args(dev, [(err, "err", f64, n * g_max, EXACT), (row_offs, "row_offs", i64, S + 1, EXACT),
                          (gt_offs, "gt_offs", i64, S + 1, EXACT), (gt_index, "gt_index", i32, T * n, EXACT),
                          (tp, "tp", i32, T * S, EXACT)])
    if n == 0 and S == 0:
        return                       # no row and no capture: nothing to write
    ops._call("mvm_match_scores", ops._p(err), g_max, ops._p(row_offs), ops._p(gt_offs), S,
              (ctypes.c_double * T)(*thresholds), T, ops._p(gt_index), ops._p(tp), n, ops._stream(err))


@ops._gpu_op("fit_boxes_out", ("pose_out", "rms", "info", "cov", "resid"), namespace="mvmatch_views")
def fit_boxes_out(pose: Tensor, scene: Tensor, views: Tensor, boxes: Tensor, proj: Tensor, verts: Tensor,
                  n_cams: int, scene_base: int, max_evals: int, pose_out: Tensor, rms: Tensor, info: Tensor,
                  cov: Optional[Tensor], resid: Optional[Tensor]) -> None:
    """Fit every row's translation to its views' boxes, given the model
    (mvm_fit_boxes).  ``pose`` / ``scene`` / ``views`` / ``boxes`` / ``proj`` /
    ``verts`` are read only; ``pose_out`` / ``rms`` / ``info`` and ``cov`` /
    ``resid`` (None: not computed) out."""
    dev = ops._gpu(pose, "pose", "box fit")
    if not 3 <= n_cams <= _native.MVM_MAX_CAMS:
        raise ValueError(f"n_cams: expected 3..{_native.MVM_MAX_CAMS}, got {n_cams}")
    if pose.dim() != 3 or tuple(pose.shape[1:]) != (4, 4):
        raise ValueError(f"pose must be [n, 4, 4], got {tuple(pose.shape)}")
    if proj.dim() != 4 or tuple(proj.shape[1:]) != (n_cams, 3, 4):
        raise ValueError(f"proj must be [S, {n_cams}, 3, 4], got {tuple(proj.shape)}")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise ValueError(f"verts must be [V, 3] with V >= 1, got {tuple(verts.shape)}")
    max_evals = _check_max_evals(max_evals)
    n, S = int(pose.shape[0]), int(proj.shape[0])
    rows = [(pose, "pose", f64, 16 * n, EXACT), (scene, "scene", i32, n, EXACT),
            (views, "views", i32, n_cams * n, EXACT), (boxes, "boxes", i32, 4 * n_cams * n, EXACT),
            (proj, "proj", f64, 12 * n_cams * S, EXACT), (verts, "verts", f64, None, ANY),
            (pose_out, "pose_out", f64, 16 * n, EXACT), (rms, "rms", f64, 2 * n, EXACT),
            (info, "info", i32, 2 * n, EXACT)]
    if cov is not None:
        rows.append((cov, "cov", f64, 6 * n, EXACT))
    if resid is not None:
        rows.append((resid, "resid", f64, 4 * n_cams * n, EXACT))
    ops._check_args(dev, rows)
    if n == 0:
        return                       # no row: nothing to launch
    if pose_out.data_ptr() == pose.data_ptr():
        raise ValueError("pose_out must not be pose: the input is kept")
    if S == 0:
        raise ValueError("proj holds no capture")
    ops._call("mvm_fit_boxes", ops._p(pose), ops._p(scene), scene_base, ops._p(views), ops._p(boxes), n, n_cams,
              ops._p(proj), S, ops._p(verts), int(verts.shape[0]), max_evals, ops._p(pose_out), ops._p(rms),
              ops._p(info), ops._p(cov), ops._p(resid), ops._stream(pose))


def mark_used(views: Tensor, match_offs: Tensor, count: Tensor, cam_offs: Tensor, used: Tensor, n_cams: int,
              seed=(0, 1, 2), sub_cam_offs: Optional[Tensor] = None, orig: Optional[Tensor] = None) -> Tensor:
    """Flag the detections the matches of one pass hold (device).
    ``views`` int32 [cap, n_cams] with capture s's matches at rows
    ``match_offs[s] : match_offs[s] + count[s]``; ``used`` int32, one flag per
    detection of the n_cams-camera CSR ``cam_offs`` (original camera order),
    zeroed by the caller once and marked pass after pass.  A first pass passes
    its views as they are; a later one its ``seed`` and its sub-batch's
    ``sub_cam_offs`` / ``orig``, through which its views name original
    detections.  Entries that are negative or no index of their view mark
    nothing.  -> ``used``."""
    torch.ops.mvmatch_views.mark_used_out(views, match_offs, count, int(n_cams), list(seed), sub_cam_offs,
                                          orig, cam_offs, used)
    return used


def leftover_counts(used: Tensor, cam_offs: Tensor, n_cams: int, seed, out: Optional[Tensor] = None) -> Tensor:
    """-> int32 [C S]: the detections with ``used == 0`` per (capture, slot),
    slot q standing for camera ``seed_order(seed, n_cams)[q]`` (device)."""
    if out is None:
        out = torch.empty(max(int(cam_offs.numel()) - 1, 0), dtype=torch.int32, device=cam_offs.device)
    torch.ops.mvmatch_views.leftover_counts_out(used, cam_offs, int(n_cams), list(seed), out)
    return out


def leftover_gather(used: Tensor, pts: Tensor, boxes: Tensor, cam_offs: Tensor, sub_cam_offs: Tensor,
                    n_cams: int, seed, n_out: int):
    """The sub-batch of a seed pass (device): the ``n_out`` unused detections
    of ``pts`` f64 [n, 2] / ``boxes`` int32 [n, 4], per view in ascending
    index order, views in the seed's camera order; ``sub_cam_offs`` int64
    [C S + 1]: the prefix sum of ``leftover_counts``.
    -> (pts f64 [n_out, 2], boxes int32 [n_out, 4], orig int32 [n_out]: each
    one's index in its original view)."""
    dev = used.device
    outs = (torch.empty((n_out, 2), dtype=torch.float64, device=dev),
            torch.empty((n_out, 4), dtype=torch.int32, device=dev),
            torch.empty(n_out, dtype=torch.int32, device=dev))
    torch.ops.mvmatch_views.leftover_gather_out(used, pts, boxes, cam_offs, sub_cam_offs, int(n_cams),
                                                list(seed), *outs)
    return outs


def prune_views(views: Tensor, ext_cost: Tensor, X: Tensor, match_offs: Tensor, count: Tensor,
                pts: Tensor, cam_offs: Tensor, proj: Tensor, gate: float, n_cams: int,
                out: Optional[Tensor] = None) -> Tensor:
    """Prune the extra views of a C-camera result by reprojection residual and
    triangulate again (device).  ``views`` int32 [cap, n_cams],
    ``ext_cost`` f32 [cap, n_cams-3] and ``X`` f64 [cap, 3] as
    ``ops.extend_select_triangulate`` left them, updated in place: per match,
    while an extra view's residual (§3.12's, in pixels) is not <= ``gate``,
    the worst one (NaN first, then the largest, ties to the lowest camera) gets
    ``views = -1`` / ``ext_cost = +inf`` and X is the DLT over the views left.
    Cameras 0-2 are never dropped; a row that drops nothing is not written.
    ``match_offs`` int64 [S+1] / ``count`` int32 [S]: capture s's matches are
    rows ``match_offs[s] : match_offs[s] + count[s]``; ``pts`` / ``cam_offs``
    the n_cams-camera CSR, ``proj`` f64 [S, n_cams, 3, 4].
    -> pruned int32 [cap]: bit d set where camera d was dropped (``out`` to
    write into: only the captures' match rows are written; allocated here it
    is 0 elsewhere)."""
    if out is None:
        out = torch.zeros(int(views.shape[0]), dtype=torch.int32, device=views.device)
    torch.ops.mvmatch_views.prune_views_out(views, ext_cost, X, match_offs, count, pts, cam_offs,
                                            proj.contiguous(), float(gate), int(n_cams), out)
    return out


def refine_points(views: Tensor, X: Tensor, match_offs: Tensor, count: Tensor, pts: Tensor,
                  cam_offs: Tensor, proj: Tensor, n_cams: int, max_evals: int = 10, cov: bool = True):
    """Refine triangulated points by their reprojection error (device; DESIGN
    §3.17).  ``views`` int32 [cap, n_cams] (a three-camera batch: its
    ``match``) and ``X`` f64 [cap, 3] as the chain left them, neither written;
    ``match_offs`` / ``count`` / ``pts`` / ``cam_offs`` / ``proj`` as
    ``prune_views`` takes them.  Per match, over the views with ``views >= 0``:
    the summed squared reprojection error is minimised from X by damped
    Gauss-Newton steps that never raise it, at most ``max_evals`` (1..64)
    trial evaluations.
    -> (X_out f64 [cap, 3]; rms f64 [cap, 2]: sqrt(cost / views) at X and at
    X_out, pixels; info int32 [cap, 2]: (status, evaluations), status 0
    converged, 1 stopped at ``max_evals``, 2 not finite or singular (X_out =
    X), 3 skipped: fewer than two views or an index outside its view (X_out =
    X, rms / cov NaN); cov f64 [cap, 6] or None with ``cov=False``: the upper
    triangle, row-major, of the inverse normal matrix at X_out, mm^2 / px^2 --
    times the pixel variance, the point's covariance).  Only the captures'
    match rows are written; the others hold NaN / (3, 0)."""
    max_evals = _check_max_evals(max_evals)       # before the op's schema turns a bool or a float into an int
    cap, dev = int(views.shape[0]), views.device
    X_out = torch.full((cap, 3), math.nan, dtype=torch.float64, device=dev)
    rms = torch.full((cap, 2), math.nan, dtype=torch.float64, device=dev)
    info = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    info[:, 0] = 3
    cv = torch.full((cap, 6), math.nan, dtype=torch.float64, device=dev) if cov else None
    torch.ops.mvmatch_views.refine_points_out(views, X, match_offs, count, pts, cam_offs, proj.contiguous(),
                                              int(n_cams), max_evals, X_out, rms, info, cv)
    return X_out, rms, info, cv


def norm_lut(mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype: torch.dtype = torch.float32) -> Tensor:
    """The look-up table of ``crop_views`` (host): float32
    [3, 256], ``lut[c][v] = (float32(v) / float32(255) - float32(mean[c])) /
    float32(std[c])`` with one IEEE float32 operation each -- what ``to_tensor``
    followed by ``normalize`` computes for level v of plane c (``mean`` /
    ``std`` in plane order: R, G, B).  ``dtype=torch.float16``: that table
    rounded to nearest-even once."""
    if dtype not in _CROP_KINDS:
        raise ValueError(f"dtype: expected torch.float32 or torch.float16, got {dtype}")
    mean, std = (np.asarray([float(x) for x in v], np.float32) for v in (mean, std))
    if mean.shape != (3,) or std.shape != (3,):
        raise ValueError("mean / std: expected three values each (R, G, B)")
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    with np.errstate(divide="ignore", invalid="ignore"):
        lut = (v[None, :] - mean[:, None]) / std[:, None]
    return torch.from_numpy(np.ascontiguousarray(lut, np.float32)).to(dtype)


def crop_views(images: Tensor, scene: Tensor, views: Tensor, boxes: Tensor, n_cams: int,
               rows: Optional[Sequence[int]] = None, cams: Optional[Sequence[int]] = None, size: int = 256,
               mean=IMAGENET_MEAN, std=IMAGENET_STD, fill: int = 255, dtype: torch.dtype = torch.float32,
               scene_base: int = 0):
    """The pose head's input crops of a match table's views (device; DESIGN
    §3.18).  ``images`` uint8 [S, n_cams, H, W, 3], channel order B, G, R;
    ``scene`` int32 [n], ``views`` int32 [n, n_cams] (a three-camera table:
    its ``match``) and ``boxes`` int32 [n, n_cams, 4] a ``MatchTable``'s
    fields, none written.  For every row of ``rows`` ((begin, end), default
    all) and every camera of ``cams`` (default all, any order): the row's box
    in that camera is clipped to the image, resampled by the exact box
    integral so that its longer side is ``size``, centred on a ``size`` x
    ``size`` canvas of ``fill`` and sent through the table ``norm_lut(mean,
    std, dtype)``, R plane first.  tests/crop_model.py states every step; the result is its bits.
    -> (crops ``dtype`` [rows, cams, 3, size, size]; geom int32 [rows, cams,
    8]: (status, xa, ya, w, h, new_w, new_h, image index), status 0 made, 1
    made from a clipped box, 2 empty after clipping, 3 no view (``views <
    0``), 4 ``scene - scene_base`` is no capture of ``images``; for 2-4 the
    crop is all fill).  One float32 crop of 256 x 256 is 786 KB: pass row
    ranges."""
    n_cams = int(n_cams)
    n = int(scene.shape[0])
    if rows is None:
        rows = (0, n)
    try:
        begin, end = (int(r) for r in rows)
    except (TypeError, ValueError):
        raise ValueError(f"rows: expected a (begin, end) pair, got {rows!r}") from None
    if not 0 <= begin <= end <= n:
        raise ValueError(f"rows: expected 0 <= begin <= end <= {n}, got ({begin}, {end})")
    cams = list(range(n_cams)) if cams is None else [int(c) for c in cams]
    if isinstance(size, bool) or not isinstance(size, int):
        raise ValueError(f"size: expected an int in 1..{CROP_MAX_SIZE}, got {size!r}")
    if isinstance(fill, bool) or not isinstance(fill, int):
        raise ValueError(f"fill: expected an int in 0..255, got {fill!r}")
    if dtype not in _CROP_KINDS:
        raise ValueError(f"dtype: expected torch.float32 or torch.float16, got {dtype}")
    dev = images.device
    lut = norm_lut(mean, std, dtype).to(dev)
    if not 1 <= size <= CROP_MAX_SIZE:
        raise ValueError(f"size: expected 1..{CROP_MAX_SIZE}, got {size}")
    crops = torch.empty((end - begin, len(cams), 3, size, size), dtype=dtype, device=dev)
    geom = torch.empty((end - begin, len(cams), 8), dtype=torch.int32, device=dev)
    torch.ops.mvmatch_views.crop_views_out(images, scene.contiguous(), views.contiguous(), boxes.contiguous(),
                                           n_cams, int(scene_base), begin, end - begin, cams, size, fill, lut,
                                           crops, geom)
    return crops, geom


@dataclass
class FusedRotations:
    """What ``fuse_rotations`` returns, on the device (n rows, K selected cameras)."""
    R: Tensor                    # float64 [n, 3, 3]     the row's rotation (object -> world), NaN without one
    pose: Tensor                 # float64 [n, 4, 4]     [[R, X], [0, 0, 0, 1]]
    rot_views: Tensor            # float64 [n, K, 3, 3]  each view's rotation in the world, NaN where unusable
    spread: Tensor               # float64 [n, K]        |rot_views - R|_F^2: 0 .. 8, NaN where either is NaN
    slot_status: Tensor          # int32 [n, K]          0, SLOT_NO_VIEW, SLOT_NO_CAPTURE or SLOT_DEGENERATE (the
    #                                                    decoded matrix not finite, its world product not below 2^500)
    row_status: Tensor           # int32 [n]             0, ROW_NO_ROTATION or ROW_AMBIGUOUS


def fuse_rotations(raw: Tensor, scene: Tensor, views: Tensor, X: Tensor, RTs, n_cams: int, mode: str,
                   rows: Optional[Sequence[int]] = None, cams: Optional[Sequence[int]] = None,
                   fuse: str = "cam", cam: int = 2, scene_base: int = 0) -> FusedRotations:
    """From a rotation head's raw outputs to a pose per match (device; DESIGN
    §3.19).  ``raw`` float32 [rows, cams, D]: the head's output for the crops
    ``crop_views`` made with the same ``rows`` and ``cams``; ``mode`` "euler"
    (D = 3, radians), "quat" (D = 4: x, y, z, w) or "6d" (D = 6).  ``scene``
    int32 [n], ``views`` int32 [n, n_cams] (a three-camera table: its
    ``match``) and ``X`` f64 [n, 3] a ``MatchTable``'s fields, none written;
    ``RTs`` f64 [S, n_cams, 4, 4] (world -> camera), a host array (copied once)
    or a device tensor.  Per slot the raw vector is decoded in float32 as the
    reference decodes it and taken to the world, ``RTs[s, c, :3, :3].T @ M``
    in float64.  Per row the usable slots are fused: ``fuse="cam"`` keeps
    camera ``cam``'s rotation (default 2, the reference's ``final_rotation``),
    ``fuse="mean"`` takes the chordal mean of them all.  tests/pose_model.py
    states every step; the result is its bits.
    -> ``FusedRotations``.  ``slot_status``: SLOT_NO_CAPTURE where ``scene -
    scene_base`` is no capture of ``RTs``, SLOT_NO_VIEW where ``views < 0``,
    SLOT_DEGENERATE where the decoded matrix is not finite (a zero quaternion,
    a NaN) or its world product has an entry that is not below 2^500 in
    magnitude (a NaN, infinite or absurd rotation block of ``RTs``).
    ``row_status``: ROW_NO_ROTATION where no usable slot
    was left (R NaN), ROW_AMBIGUOUS where the mean is not determined (views
    half a turn apart; R still written).  ``R`` is NaN only under
    ROW_NO_ROTATION and ``rot_views`` only where ``slot_status`` is not 0,
    whatever ``RTs`` holds.  ``spread`` is the caller's consistency gate."""
    n_cams = int(n_cams)
    n = int(scene.shape[0])
    if rows is None:
        rows = (0, n)
    try:
        begin, end = (int(r) for r in rows)
    except (TypeError, ValueError):
        raise ValueError(f"rows: expected a (begin, end) pair, got {rows!r}") from None
    if not 0 <= begin <= end <= n:
        raise ValueError(f"rows: expected 0 <= begin <= end <= {n}, got ({begin}, {end})")
    cams = list(range(n_cams)) if cams is None else [int(c) for c in cams]
    if mode not in ROTATION_MODES:
        raise ValueError(f"mode: expected one of {sorted(ROTATION_MODES)}, got {mode!r}")
    if fuse not in ROTATION_FUSE:
        raise ValueError(f"fuse: expected one of {sorted(ROTATION_FUSE)}, got {fuse!r}")
    if isinstance(cam, bool) or not isinstance(cam, int):
        raise ValueError(f"cam: expected a camera, got {cam!r}")
    if fuse == "cam" and cam not in cams:
        raise ValueError(f"cam: camera {cam} is not among the selected cameras {cams}")
    dev = raw.device
    m, K, D = end - begin, len(cams), ROTATION_MODES[mode][1]
    if raw.dim() != 3 or tuple(raw.shape) != (m, K, D):
        raise ValueError(f"raw must be [{m}, {K}, {D}] for mode {mode!r}, got {tuple(raw.shape)}")
    if not isinstance(RTs, Tensor):
        RTs = torch.from_numpy(np.ascontiguousarray(RTs, np.float64)).to(dev)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = FusedRotations(R=e((m, 3, 3), f64), pose=e((m, 4, 4), f64), rot_views=e((m, K, 3, 3), f64),
                         spread=e((m, K), f64), slot_status=e((m, K), i32), row_status=e(m, i32))
    torch.ops.mvmatch_views.fuse_rotations_out(raw, scene.contiguous(), views.contiguous(), X.contiguous(),
                                               RTs.contiguous(), n_cams, int(scene_base), begin, m, cams, mode,
                                               fuse, cam, out.rot_views, out.R, out.pose, out.spread,
                                               out.slot_status, out.row_status)
    return out


@dataclass
class PoseScores:
    """What ``score_poses`` returns, on the device (n rows, Gmax ground-truth columns)."""
    err: Tensor                  # float64 [n, Gmax]   MSSD of (row, the capture's g-th object); +inf where sym < 0
    sym: Tensor                  # int32 [n, Gmax]     the symmetry that gave it, or SYM_PADDING (g is past the
    #                                                  capture's objects), SYM_NO_CAPTURE, SYM_NOT_FINITE
    t_err: Tensor                # float64 [n, Gmax]   the distance of the translations; +inf where sym < 0
    rot_cos: Tensor              # float64 [n, Gmax]   the cosine of the rotation between the two; NaN where sym < 0
    # set by MatchTable.score(thresholds=...): ``match_scores`` of err
    gt_index: Optional[Tensor] = None     # int32 [T, n]   the object each row took per threshold, or -1
    tp: Optional[Tensor] = None           # int32 [T, S]   matched rows per threshold and capture


def _host_offsets(offs, name: str) -> np.ndarray:
    """An offset table (host array, sequence or tensor) as a checked host int64 array."""
    if isinstance(offs, Tensor):
        offs = offs.detach().cpu().numpy()
    offs = np.ascontiguousarray(offs, np.int64).reshape(-1)
    if offs.size < 1 or offs[0] < 0 or (np.diff(offs) < 0).any():
        raise ValueError(f"{name}: expected non-decreasing offsets from 0 on, one per capture and one more")
    return offs


def _model_array(a, name: str, tail: tuple, dev) -> Tensor:
    """Vertices or symmetries: a device tensor taken as given, or a host array
    checked (finite and below 2^200 in magnitude) and copied."""
    if isinstance(a, Tensor):
        return a.contiguous()
    a = np.ascontiguousarray(a, np.float64)
    if a.ndim != len(tail) + 1 or a.shape[1:] != tail or a.shape[0] < 1:
        raise ValueError(f"{name} must be [k, {', '.join(str(t) for t in tail)}] with k >= 1, got {a.shape}")
    if not (np.abs(a) < SCORE_POSE_MAX).all():
        raise ValueError(f"{name}: expected finite values below 2^200 in magnitude")
    return torch.from_numpy(a).to(dev)


def score_poses(pose: Tensor, scene: Tensor, gt_pose, gt_offs, verts, syms=None,
                rows: Optional[Sequence[int]] = None, scene_base: int = 0) -> PoseScores:
    """The BOP pose error MSSD (maximum symmetry-aware surface distance) of
    every (estimate, ground-truth object) pair of a capture (device; DESIGN
    §3.20).  ``pose`` f64 [n, 4, 4]: the estimates in the world frame (for
    example ``FusedRotations.pose``) and ``scene`` int32 [n] their capture ids,
    neither written; ``gt_pose`` f64 [G, 4, 4] the ground-truth poses in the
    world frame and ``gt_offs`` int64 [S + 1] the rows of each capture among
    them (host arrays, copied once, or device tensors; ``gt_offs`` is read on
    the host either way: its largest count is the width of the result);
    ``verts`` f64 [V, 3] the model's vertices and ``syms`` f64 [K, 4, 4] (K <=
    64, default the identity) its symmetry transforms (host arrays are checked:
    finite and below 2^200).  For every row of ``rows`` ((begin, end), default
    all) and every g < Gmax: ``err = min_k max_v |(Rp v + tp) - (Rg (Sk v + sk)
    + tg)|`` in the affine form tests/score_model.py states; the result is its
    bits.
    -> ``PoseScores``; ``sym`` is the symmetry of the minimum (the lowest of
    equal ones), SYM_NO_CAPTURE where ``scene - scene_base`` is no capture of
    ``gt_offs``, SYM_PADDING where g is past the capture's objects,
    SYM_NOT_FINITE where either pose has a read entry that is not below 2^200
    in magnitude; in all three ``err`` and ``t_err`` are +inf and ``rot_cos``
    NaN.  The arccosine of ``rot_cos`` is the caller's."""
    dev = pose.device
    n = int(scene.shape[0])
    if rows is None:
        rows = (0, n)
    try:
        begin, end = (int(r) for r in rows)
    except (TypeError, ValueError):
        raise ValueError(f"rows: expected a (begin, end) pair, got {rows!r}") from None
    if not 0 <= begin <= end <= n:
        raise ValueError(f"rows: expected 0 <= begin <= end <= {n}, got ({begin}, {end})")
    offs = _host_offsets(gt_offs, "gt_offs")
    if not isinstance(gt_pose, Tensor):
        gt_pose = torch.from_numpy(np.ascontiguousarray(gt_pose, np.float64).reshape(-1, 4, 4)).to(dev)
    if gt_pose.dim() != 3 or tuple(gt_pose.shape[1:]) != (4, 4):
        raise ValueError(f"gt_pose must be [G, 4, 4], got {tuple(gt_pose.shape)}")
    if offs[-1] > gt_pose.shape[0]:
        raise ValueError(f"gt_offs ends at {offs[-1]}, gt_pose holds {gt_pose.shape[0]} poses")
    if gt_pose.shape[0] == 0:            # no object anywhere: a pose no offset reaches
        gt_pose = torch.zeros((1, 4, 4), dtype=f64, device=gt_pose.device)
    g_max = max(1, int(np.diff(offs).max())) if offs.size > 1 else 1
    verts = _model_array(verts, "verts", (3,), dev)
    syms = _model_array(np.eye(4)[None] if syms is None else syms, "syms", (4, 4), dev)
    m = end - begin
    e = lambda dt: torch.empty((m, g_max), dtype=dt, device=dev)
    out = PoseScores(err=e(f64), sym=e(i32), t_err=e(f64), rot_cos=e(f64))
    offs_dev = gt_offs if isinstance(gt_offs, Tensor) and gt_offs.device == dev and gt_offs.dtype == i64 \
        else torch.from_numpy(offs).to(dev)
    torch.ops.mvmatch_views.score_poses_out(pose.contiguous(), scene.contiguous(), gt_pose.contiguous(),
                                            offs_dev.contiguous(), verts, syms, int(scene_base), g_max, begin, m,
                                            out.err, out.sym, out.t_err, out.rot_cos)
    return out


@dataclass
class SymFusedRotations(FusedRotations):
    """What ``fuse_rotations_sym`` returns, on the device: ``FusedRotations``
    with ``rot_views`` the aligned views ``W S_k`` of the last round, ``spread``
    their distance to ``R``, SLOT_NO_SYM among ``slot_status``, and:"""
    sym_index: Tensor            # int32 [n, K]          the symmetry each view took in the last round, -1 where unusable
    sym_margin: Tensor           # float64 [n, K]        its score minus the next best (+inf: no other), NaN where unusable
    n_changed: Tensor            # int32 [n]             views whose symmetry the last round changed (0: converged)


def fuse_rotations_sym(raw: Tensor, scene: Tensor, views: Tensor, X: Tensor, RTs, n_cams: int, mode: str, syms,
                       rows: Optional[Sequence[int]] = None, cams: Optional[Sequence[int]] = None,
                       rounds: int = 2, scene_base: int = 0) -> SymFusedRotations:
    """``fuse_rotations(fuse="mean")`` for a symmetric object (device; DESIGN
    §3.21): a head may answer, per view, any of the rotations ``R S_k`` that
    look alike from there, and their plain mean is none of them.  ``syms`` f64
    [K, 4, 4], K >= 1: the object's symmetry transforms as ``score_poses``
    takes them (a host array, checked and copied once, or a device tensor;
    only the rotation blocks are read).  Every other argument is
    ``fuse_rotations``'s.  Per row the first usable view in the order of
    ``cams`` is the reference; every usable view is multiplied by the symmetry
    that takes it nearest the reference (the lowest index of equal ones), the
    chordal mean of the aligned views is taken, and the same is done again
    with that mean as the reference, ``rounds`` (1..4) times in all.
    tests/pose_sym_model.py states every step; the result is its bits, and
    with the identity alone ``fuse="mean"``'s numbers.
    -> ``SymFusedRotations``.  ``slot_status`` is SLOT_NO_SYM where no symmetry
    left the view usable (a NaN, infinite or absurd ``syms``); such a view
    leaves the mean.  ``sym_margin`` near 0 marks a view between two symmetry
    elements; ``n_changed`` > 0 a row that another round would still move."""
    n_cams = int(n_cams)
    n = int(scene.shape[0])
    if rows is None:
        rows = (0, n)
    try:
        begin, end = (int(r) for r in rows)
    except (TypeError, ValueError):
        raise ValueError(f"rows: expected a (begin, end) pair, got {rows!r}") from None
    if not 0 <= begin <= end <= n:
        raise ValueError(f"rows: expected 0 <= begin <= end <= {n}, got ({begin}, {end})")
    cams = list(range(n_cams)) if cams is None else [int(c) for c in cams]
    if mode not in ROTATION_MODES:
        raise ValueError(f"mode: expected one of {sorted(ROTATION_MODES)}, got {mode!r}")
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= SYM_MAX_ROUNDS:
        raise ValueError(f"rounds: expected 1..{SYM_MAX_ROUNDS}, got {rounds!r}")
    dev = raw.device
    m, K, D = end - begin, len(cams), ROTATION_MODES[mode][1]
    if raw.dim() != 3 or tuple(raw.shape) != (m, K, D):
        raise ValueError(f"raw must be [{m}, {K}, {D}] for mode {mode!r}, got {tuple(raw.shape)}")
    if not isinstance(RTs, Tensor):
        RTs = torch.from_numpy(np.ascontiguousarray(RTs, np.float64)).to(dev)
    syms = _model_array(syms, "syms", (4, 4), dev)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = SymFusedRotations(R=e((m, 3, 3), f64), pose=e((m, 4, 4), f64), rot_views=e((m, K, 3, 3), f64),
                            spread=e((m, K), f64), slot_status=e((m, K), i32), row_status=e(m, i32),
                            sym_index=e((m, K), i32), sym_margin=e((m, K), f64), n_changed=e(m, i32))
    torch.ops.mvmatch_views.fuse_rotations_sym_out(raw, scene.contiguous(), views.contiguous(), X.contiguous(),
                                                   RTs.contiguous(), syms, n_cams, int(scene_base), begin, m,
                                                   cams, mode, rounds, out.rot_views, out.R, out.pose, out.spread,
                                                   out.slot_status, out.row_status, out.sym_index,
                                                   out.sym_margin, out.n_changed)
    return out


def match_scores(err: Tensor, row_offs, gt_offs, thresholds):
    """Match every capture's rows greedily to its ground truth (device; DESIGN
    §3.20).  ``err`` f64 [n, Gmax <= 1024]: ``score_poses``'s err over the
    whole table, not written; ``row_offs`` int64 [S + 1]: a ``MatchTable``'s
    ``offs``; ``gt_offs`` int64 [S + 1] as ``score_poses`` takes it (host
    arrays or tensors; both are checked on the host); ``thresholds`` 1..16
    numbers, no NaN.  Per threshold and capture the rows are walked in table
    order -- the matcher's cost order, the confidence order BOP's greedy
    matching wants --, and a row takes the free object with the smallest error
    below the threshold (strict; the lowest index wins a tie) or -1.
    -> (gt_index int32 [T, n], tp int32 [T, S]: the matched rows per threshold
    and capture).  Rows outside every capture get -1."""
    ro, go = _host_offsets(row_offs, "row_offs"), _host_offsets(gt_offs, "gt_offs")
    if ro.size != go.size:
        raise ValueError(f"row_offs describes {ro.size - 1} captures, gt_offs {go.size - 1}")
    if err.dim() != 2:
        raise ValueError(f"err must be [n, g_max], got {tuple(err.shape)}")
    n, dev = int(err.shape[0]), err.device
    if ro[-1] > n:
        raise ValueError(f"row_offs ends at {ro[-1]}, err holds {n} rows")
    try:
        thresholds = [float(v) for v in thresholds]
    except TypeError:
        raise ValueError(f"thresholds: expected 1..{SCORE_MAX_THRESHOLDS} numbers, got {thresholds!r}") from None
    if not 1 <= len(thresholds) <= SCORE_MAX_THRESHOLDS or any(math.isnan(v) for v in thresholds):
        raise ValueError(f"thresholds: expected 1..{SCORE_MAX_THRESHOLDS} numbers and no NaN, got {thresholds}")
    T, S = len(thresholds), ro.size - 1
    gt_index = torch.empty((T, n), dtype=i32, device=dev)
    tp = torch.empty((T, S), dtype=i32, device=dev)
    torch.ops.mvmatch_views.match_scores_out(err.contiguous(), torch.from_numpy(ro).to(dev),
                                             torch.from_numpy(go).to(dev), thresholds, gt_index, tp)
    return gt_index, tp


def recall_precision(tp: Tensor, row_offs, gt_offs):
    """-> (recall f64 [T], precision f64 [T]) of ``match_scores``'s ``tp`` over
    the whole table, on ``tp``'s device: the matched rows over the ground-truth
    objects and over the table's rows (NaN where there are none).  Average
    recall is the mean of ``recall`` over the thresholds."""
    as_t = lambda o: o if isinstance(o, Tensor) else torch.from_numpy(np.ascontiguousarray(o, np.int64))
    n_rows = as_t(row_offs).diff().sum().to(tp.device, f64)
    n_gt = as_t(gt_offs).diff().sum().to(tp.device, f64)
    hit = tp.sum(dim=1).to(f64)
    return hit / n_gt, hit / n_rows


@dataclass
class BoxFit:
    """What ``fit_boxes`` returns, on the device (n rows, C cameras)."""
    pose: Tensor                 # float64 [n, 4, 4]   the input pose with the fitted translation
    rms: Tensor                  # float64 [n, 2]      sqrt(cost / (4 views)) at the start and at the result, pixels
    info: Tensor                 # int32 [n, 2]        (status, evaluations): 0 converged, 1 capped, 2 failed, 3 skipped
    cov: Optional[Tensor]        # float64 [n, 6]      the inverse normal matrix at the result (upper triangle)
    resid: Optional[Tensor]      # float64 [n, C, 4]   (umin - x1, vmin - y1, umax - x2, vmax - y2), NaN without a view


def fit_boxes(pose: Tensor, scene: Tensor, views: Tensor, boxes: Tensor, proj, n_cams: int, verts,
              rows: Optional[Sequence[int]] = None, max_evals: int = 10, cov: bool = True, resid: bool = True,
              scene_base: int = 0) -> BoxFit:
    """Fit each pose's translation to the detected boxes, given the model
    (device).  ``pose`` f64 [rows, 4, 4]: the rotation and the
    start of every row of ``rows`` (for example ``FusedRotations.pose``, whose
    translation is the table's X: the triangulation of the box centres, which
    are not the projections of the object's origin); ``scene`` int32 [n],
    ``views`` int32 [n, n_cams] (a three-camera table: its ``match``) and
    ``boxes`` int32 [n, n_cams, 4] a ``MatchTable``'s fields, none written;
    ``proj`` f64 [S, n_cams, 3, 4] (a host array, copied once, or a device
    tensor); ``verts`` f64 [V, 3] the model's vertices as ``score_poses`` takes
    them.  Per row, over the views with ``views >= 0`` (one is enough): the
    summed squared distance between the edges of the detected box and of the
    bounding box of the projected vertices is minimised over the translation
    by ``refine_points``' damped Gauss-Newton steps, which never raise it, at
    most ``max_evals`` (1..64) trial evaluations.  tests/box_fit_model.py
    states every step; the result is its bits.
    -> ``BoxFit``.  ``info[:, 0]``: 0 converged, 1 stopped at ``max_evals``, 2
    a vertex behind a camera at the start, something not finite or a singular
    normal matrix (the pose stands), 3 skipped: no view, or ``scene -
    scene_base`` is no capture of ``proj`` (the pose stands; rms, cov and resid
    NaN).  ``cov`` / ``resid`` are None with ``cov=False`` / ``resid=False``."""
    max_evals = _check_max_evals(max_evals)       # before the op's schema turns a bool or a float into an int
    n_cams = int(n_cams)
    n = int(scene.shape[0])
    if rows is None:
        rows = (0, n)
    try:
        begin, end = (int(r) for r in rows)
    except (TypeError, ValueError):
        raise ValueError(f"rows: expected a (begin, end) pair, got {rows!r}") from None
    if not 0 <= begin <= end <= n:
        raise ValueError(f"rows: expected 0 <= begin <= end <= {n}, got ({begin}, {end})")
    dev, m = pose.device, end - begin
    if pose.dim() != 3 or tuple(pose.shape) != (m, 4, 4):
        raise ValueError(f"pose must be [{m}, 4, 4], got {tuple(pose.shape)}")
    if views.dim() != 2 or tuple(views.shape) != (n, n_cams):
        raise ValueError(f"views must be [{n}, {n_cams}], got {tuple(views.shape)}")
    if boxes.dim() != 3 or tuple(boxes.shape) != (n, n_cams, 4):
        raise ValueError(f"boxes must be [{n}, {n_cams}, 4], got {tuple(boxes.shape)}")
    if not isinstance(proj, Tensor):
        proj = torch.from_numpy(np.ascontiguousarray(proj, np.float64)).to(dev)
    verts = _model_array(verts, "verts", (3,), dev)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = BoxFit(pose=e((m, 4, 4), f64), rms=e((m, 2), f64), info=e((m, 2), i32),
                 cov=e((m, 6), f64) if cov else None, resid=e((m, n_cams, 4), f64) if resid else None)
    torch.ops.mvmatch_views.fit_boxes_out(pose.contiguous(), scene[begin:end].contiguous(),
                                          views[begin:end].contiguous(), boxes[begin:end].contiguous(),
                                          proj.contiguous(), verts, n_cams, int(scene_base), max_evals, out.pose,
                                          out.rms, out.info, out.cov, out.resid)
    return out
