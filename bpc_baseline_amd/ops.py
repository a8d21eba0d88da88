"""PyTorch custom ops over the C ABI (``torch.ops.mvmatch.*``).

Each op is a thin shim: it validates dtypes/devices/shapes, then calls the
corresponding ``include/mvmatch.h`` entry point on the tensors' device
pointers and the current HIP stream.  Nothing here computes on the host.

Ops (all ``*_out`` ops write caller-allocated tensors, like the C ABI):
  mvmatch::pairwise_residual_argmin_out   e_ab (f32) + per-row argmin/min
  mvmatch::pairwise_residual_f64_out      e_ab kept in float64 (uniform layout)
  mvmatch::triplet_cost_argmin_out        3-camera cube + per-(i,j) argmin

An op states what it accepts as one row per tensor argument, ``(tensor, name,
dtype, numel, mode)``, checked by ``_check_args``: the mode (``EXACT``,
``AT_LEAST``, ``ANY``) says how the element count is compared with ``numel``.

Plans (``PairwisePlan`` / ``TripletPlan``) hold the host-side offset tables
(prefix sums of the per-view detection counts) and their device copies; a
plan is reusable for every batch with the same counts.

Kernel-path choices (``include/mvmatch.h`` ``mvm_options``) are explicit:
the high-level functions take ``options=dict(...)`` (field names of
``_native.MvmOptions``) and the ops an ``opts`` list of the field values; by
default (None) the library's compiled-in defaults apply.  The choices never
change results -- the parity tests run every path.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native

__all__ = [
    "PairwisePlan", "TripletPlan",
    "pairwise_residual_argmin", "pairwise_residual_f64", "triplet_cost_argmin",
    "hbm_write_probe", "LsapPlan", "linear_sum_assignment_batched",
    "pack_detections", "triangulate_dlt", "select_triangulate",
    "triplet_minima", "linear_sum_assignment_resid", "select_triangulate_resid",
    "cube_free_scenes", "sparse_class_bounds", "lsap_sparse_stats", "compact_matches",
    "rig_matrices", "extend_costs", "extend_select_triangulate", "compact_matches_views",
]

f32, f64, i16, i32, i64, u8 = (torch.float32, torch.float64, torch.int16, torch.int32, torch.int64,
                               torch.uint8)


def _h2d_int64(arrays: List[np.ndarray], device: torch.device) -> List[Tensor]:
    """Host int64 arrays -> device tensors with ONE copy: concatenated into a
    pinned staging buffer and copied without blocking (a plan's offsets used
    to cost one synchronous pageable copy each).  Returns views of the one
    device buffer, in order."""
    flat = np.concatenate([np.ascontiguousarray(a, dtype=np.int64).reshape(-1) for a in arrays])
    host = torch.from_numpy(flat)
    if device.type == "cuda":
        dev = host.pin_memory().to(device, non_blocking=True)
    else:
        dev = host.to(device)
    out, o = [], 0
    for a in arrays:
        out.append(dev[o:o + a.size])
        o += a.size
    return out


def _opts_list(options: Optional[dict]) -> Optional[List[int]]:
    """options dict -> the op's ``opts`` list (mvm_options fields after ``size``)."""
    o = _native.make_options(**(options or {}))
    return None if o is None else [int(getattr(o, n)) for n in _native.OPTION_FIELDS]


def _opts_ref(opts: Optional[List[int]]):
    """The op's ``opts`` list -> a pointer to an mvm_options (None = defaults)."""
    if opts is None:
        return None
    if len(opts) != len(_native.OPTION_FIELDS):
        raise ValueError(f"opts: expected {len(_native.OPTION_FIELDS)} values, got {len(opts)}")
    return ctypes.byref(_native.make_options(**dict(zip(_native.OPTION_FIELDS, opts))))


def _p(t: Optional[Tensor]):
    if t is None or t.numel() == 0:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _stream(t: Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _call(fn: str, *args) -> None:
    """The C entry point ``fn``; a status other than MVM_OK raises MvmError."""
    _native.check(fn, getattr(_native.load(), fn)(*args))


def _pair_arrays(pair_a: List[int], pair_b: List[int]):
    """The camera pair lists as the int32 arrays the C ABI reads."""
    n = len(pair_a)
    if len(pair_b) != n:
        raise ValueError("pair_a / pair_b differ in length")
    return (ctypes.c_int32 * n)(*pair_a), (ctypes.c_int32 * n)(*pair_b)


def _gpu(t: Tensor, name: str, what: str = "matcher") -> torch.device:
    """The device of the op's leading tensor, which must be a GPU."""
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be a GPU tensor (the {what} has no CPU path)")
    return t.device


def _require(t: Tensor, name: str, dtype: torch.dtype, device: torch.device) -> None:
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name}: expected device {device}, got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")


# how _check_args compares a tensor's element count with its row's ``numel``
EXACT, AT_LEAST, ANY = "exact", "at least", "any"


def _check_args(dev: torch.device, rows) -> None:
    """An op's tensor arguments against their spec, one row each: (tensor,
    name, dtype, numel, mode).  Every tensor has the dtype, lives on ``dev``
    and is contiguous (``_require``); it holds ``numel`` elements (EXACT), at
    least as many (AT_LEAST), or any number (ANY: ``numel`` is not read)."""
    for t, name, dtype, numel, mode in rows:
        _require(t, name, dtype, dev)
        if mode == EXACT:
            if t.numel() != numel:
                raise ValueError(f"{name} holds {t.numel()} elements, expected {numel}")
        elif mode == AT_LEAST:
            if t.numel() < numel:
                raise ValueError(f"{name} holds {t.numel()} elements, needs {numel}")
        elif mode != ANY:
            raise ValueError(f"{name}: unknown mode {mode!r}")


def _scene_rows(pts: Tensor, cam_offs: Tensor, F: Tensor, n_views: int, n_mats: int):
    """-> (device, rows of the three inputs the residual ops start with)."""
    dev = _gpu(pts, "pts")
    if pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError(f"pts: expected [n, 2], got {tuple(pts.shape)}")
    return dev, [(pts, "pts", f64, None, ANY), (cam_offs, "cam_offs", i64, n_views + 1, EXACT),
                 (F, "F", f64, 9 * n_mats, EXACT)]


def _fake_none(*args, **kwargs) -> None:
    """The fake of every op here: they return None (nothing to allocate or shape)."""
    return None


def _gpu_op(name: str, mutates_args, namespace: str = "mvmatch"):
    """``torch.library.custom_op("mvmatch::<name>")`` for an op that returns
    None, so one fake serves every op (nothing to allocate or shape).
    ``namespace``: for a module that registers its ops beside this one's."""
    def wrap(fn):
        op = torch.library.custom_op(f"{namespace}::{name}", mutates_args=mutates_args)(fn)
        op.register_fake(_fake_none)
        return op
    return wrap


# ------------------------------------------------------------------ ops ----
@_gpu_op("pairwise_residual_argmin_out", ("dist", "argmin", "minval"))
def pairwise_residual_argmin_out(pts: Tensor, cam_offs: Tensor, F: Tensor, pair_a: List[int],
                                 pair_b: List[int], n_scenes: int, n_cams: int, max_n: int,
                                 dist_offs: Tensor, row_offs: Tensor, dist: Tensor,
                                 argmin: Tensor, minval: Tensor,
                                 opts: Optional[List[int]] = None, row_align: int = 1) -> None:
    n_pairs = len(pair_a)
    dev, rows = _scene_rows(pts, cam_offs, F, n_scenes * n_cams, n_scenes * n_pairs)
    _check_args(dev, rows + [(dist_offs, "dist_offs", i64, None, ANY), (row_offs, "row_offs", i64, None, ANY),
                             (dist, "dist", f32, None, ANY), (argmin, "argmin", i32, None, ANY),
                             (minval, "minval", f32, None, ANY)])
    pa, pb = _pair_arrays(pair_a, pair_b)
    _call("mvm_pairwise_residual_argmin_pitched", _p(pts), _p(cam_offs), _p(F), pa, pb, n_scenes,
          n_cams, n_pairs, max_n, row_align, _p(dist_offs), _p(row_offs), _p(dist), _p(argmin),
          _p(minval), _opts_ref(opts), _stream(pts))


@_gpu_op("pairwise_residual_f64_out", ("e",))
def pairwise_residual_f64_out(pts: Tensor, cam_offs: Tensor, F: Tensor, pair_a: List[int],
                              pair_b: List[int], n_scenes: int, n_cams: int, max_n: int,
                              mat_stride: int, ld: int, e: Tensor) -> None:
    n_pairs = len(pair_a)
    dev, rows = _scene_rows(pts, cam_offs, F, n_scenes * n_cams, n_scenes * n_pairs)
    _check_args(dev, rows + [(e, "e", f64, n_scenes * n_pairs * mat_stride, AT_LEAST)])
    pa, pb = _pair_arrays(pair_a, pair_b)
    _call("mvm_pairwise_residual_f64", _p(pts), _p(cam_offs), _p(F), pa, pb, n_scenes, n_cams,
          n_pairs, max_n, mat_stride, ld, _p(e), _stream(pts))


@_gpu_op("triplet_cost_argmin_out", ("cube", "argmin", "minval", "workspace"))
def triplet_cost_argmin_out(pts: Tensor, cam_offs: Tensor, F: Tensor, n_scenes: int, max_n: int,
                            cube_offs: Tensor, row_offs: Tensor, cube: Tensor, argmin: Tensor,
                            minval: Tensor, workspace: Tensor,
                            opts: Optional[List[int]] = None) -> None:
    dev, rows = _scene_rows(pts, cam_offs, F, n_scenes * 3, n_scenes * 3)
    _check_args(dev, rows + [(cube_offs, "cube_offs", i64, None, ANY), (row_offs, "row_offs", i64, None, ANY),
                             (cube, "cube", f32, None, ANY), (argmin, "argmin", i32, None, ANY),
                             (minval, "minval", f32, None, ANY), (workspace, "workspace", u8, None, ANY)])
    _call("mvm_triplet_cost_argmin_ex", _p(pts), _p(cam_offs), _p(F), n_scenes, max_n, _p(cube_offs),
          _p(row_offs), _p(cube), _p(argmin), _p(minval), _p(workspace), workspace.numel(),
          _opts_ref(opts), _stream(pts))


@_gpu_op("triplet_cost_bmin8_out", ("cube", "argmin", "minval", "bmin8", "workspace"))
def triplet_cost_bmin8_out(pts: Tensor, cam_offs: Tensor, F: Tensor, n_scenes: int, max_n: int,
                           cube_offs: Tensor, row_offs: Tensor, cube: Tensor, argmin: Tensor,
                           minval: Tensor, bmin8: Tensor, bmin8_offs: Tensor, workspace: Tensor,
                           opts: Optional[List[int]] = None) -> None:
    """triplet_cost_argmin_out + the 8-row minima the assignment reduces
    (mvm_triplet_cost_argmin_bmin8)."""
    dev, rows = _scene_rows(pts, cam_offs, F, n_scenes * 3, n_scenes * 3)
    _check_args(dev, rows + [(cube_offs, "cube_offs", i64, None, ANY), (row_offs, "row_offs", i64, None, ANY),
                             (cube, "cube", f32, None, ANY), (argmin, "argmin", i32, None, ANY),
                             (minval, "minval", f32, None, ANY), (bmin8, "bmin8", i16, None, ANY),
                             (bmin8_offs, "bmin8_offs", i64, None, ANY),
                             (workspace, "workspace", u8, None, ANY)])
    _call("mvm_triplet_cost_argmin_bmin8", _p(pts), _p(cam_offs), _p(F), n_scenes, max_n,
          _p(cube_offs), _p(row_offs), _p(cube), _p(argmin), _p(minval), _p(bmin8), _p(bmin8_offs),
          _p(workspace), workspace.numel(), _opts_ref(opts), _stream(pts))


@_gpu_op("lsap_solve_bmin8_out", ("workspace", "row_ind", "col_ind", "status"))
def lsap_solve_bmin8_out(cost: Tensor, cost_offs: Tensor, dims: Tensor, ws_offs: Tensor,
                         out_offs: Tensor, workspace: Tensor, row_ind: Tensor, col_ind: Tensor,
                         status: Tensor, bmin8: Tensor, bmin8_offs: Tensor, segs: Tensor,
                         long_min: int, long_max: int, short_max: int,
                         opts: Optional[List[int]] = None) -> None:
    """lsap_solve_out taking a cube's 8-row minima (mvm_lsap_solve_ex3)."""
    dev = cost.device
    if dev.type != "cuda" or cost.dtype != torch.float32:
        raise ValueError("cost must be a float32 GPU tensor")
    _check_args(dev, [(cost_offs, "cost_offs", i64, None, ANY), (dims, "dims", i64, None, ANY),
                      (ws_offs, "ws_offs", i64, None, ANY), (out_offs, "out_offs", i64, None, ANY),
                      (workspace, "workspace", u8, None, ANY), (row_ind, "row_ind", i64, None, ANY),
                      (col_ind, "col_ind", i64, None, ANY), (status, "status", i32, None, ANY),
                      (bmin8, "bmin8", i16, None, ANY), (bmin8_offs, "bmin8_offs", i64, None, ANY),
                      (segs, "segs", i64, None, ANY)])
    _call("mvm_lsap_solve_ex3", _p(cost), _native.MVM_F32, _p(cost_offs), _p(dims), status.numel(),
          _p(ws_offs), _p(out_offs), _p(workspace), workspace.numel(), _p(row_ind), _p(col_ind),
          _p(status), long_min, long_max, short_max, _p(bmin8), _p(bmin8_offs), _p(segs),
          _opts_ref(opts), _stream(cost))


@_gpu_op("lsap_solve_out", ("workspace", "row_ind", "col_ind", "status"))
def lsap_solve_out(cost: Tensor, cost_offs: Tensor, dims: Tensor, ws_offs: Tensor,
                   out_offs: Tensor, workspace: Tensor, row_ind: Tensor, col_ind: Tensor,
                   status: Tensor, long_min: int = 1, long_max: int = 2 ** 62,
                   opts: Optional[List[int]] = None, short_max: int = -1) -> None:
    dev = _gpu(cost, "cost")
    if cost.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"cost: expected float32 or float64, got {cost.dtype}")
    _check_args(dev, [(cost, "cost", cost.dtype, None, ANY), (cost_offs, "cost_offs", i64, None, ANY),
                      (dims, "dims", i64, None, ANY), (ws_offs, "ws_offs", i64, None, ANY),
                      (out_offs, "out_offs", i64, None, ANY), (workspace, "workspace", u8, None, ANY),
                      (row_ind, "row_ind", i64, None, ANY), (col_ind, "col_ind", i64, None, ANY),
                      (status, "status", i32, None, ANY)])
    dtype = _native.MVM_F64 if cost.dtype == torch.float64 else _native.MVM_F32
    _call("mvm_lsap_solve_ex2", _p(cost), dtype, _p(cost_offs), _p(dims), status.numel(), _p(ws_offs),
          _p(out_offs), _p(workspace), workspace.numel(), _p(row_ind), _p(col_ind), _p(status),
          long_min, long_max, long_max if short_max < 0 else short_max, _opts_ref(opts),
          _stream(cost))


@_gpu_op("triplet_minima_out", ("bmin8", "resid"))
def triplet_minima_out(pts: Tensor, cam_offs: Tensor, F: Tensor, n_scenes: int, max_n: int,
                       bmin8: Tensor, bmin8_offs: Tensor, bm32: Tensor, bm32_offs: Tensor,
                       resid: Tensor, opts: Optional[List[int]] = None) -> None:
    """The cube's 8-row minima, the assignment's 32-column block minima and
    every scene's fp64 pair residuals, no cube (mvm_triplet_minima, ABI 7)."""
    dev, rows = _scene_rows(pts, cam_offs, F, n_scenes * 3, n_scenes * 3)
    _check_args(dev, rows + [(bmin8, "bmin8", i16, None, ANY), (bmin8_offs, "bmin8_offs", i64, None, ANY),
                             (bm32, "bm32", i16, None, ANY), (bm32_offs, "bm32_offs", i64, None, ANY),
                             (resid, "resid", u8, None, ANY)])
    _call("mvm_triplet_minima", _p(pts), _p(cam_offs), _p(F), n_scenes, max_n, _p(bmin8),
          _p(bmin8_offs), _p(bm32), _p(bm32_offs), _p(resid), resid.numel(), _opts_ref(opts),
          _stream(pts))


@_gpu_op("lsap_solve_resid_out", ("workspace", "row_ind", "col_ind", "status"))
def lsap_solve_resid_out(dims: Tensor, ws_offs: Tensor, out_offs: Tensor, workspace: Tensor,
                         row_ind: Tensor, col_ind: Tensor, status: Tensor, bmin8: Tensor,
                         bmin8_offs: Tensor, bm32: Tensor, bm32_offs: Tensor, segs: Tensor,
                         resid: Tensor, max_n: int, long_min: int, long_max: int, short_max: int,
                         opts: Optional[List[int]] = None) -> None:
    """The assignment of every flattened cube of a triplet_minima batch, from
    its 8-row minima and pair residuals (mvm_lsap_solve_resid, ABI 7)."""
    dev = _gpu(dims, "dims")
    _check_args(dev, [(dims, "dims", i64, None, ANY), (ws_offs, "ws_offs", i64, None, ANY),
                      (out_offs, "out_offs", i64, None, ANY), (workspace, "workspace", u8, None, ANY),
                      (row_ind, "row_ind", i64, None, ANY), (col_ind, "col_ind", i64, None, ANY),
                      (status, "status", i32, None, ANY), (bmin8, "bmin8", i16, None, ANY),
                      (bmin8_offs, "bmin8_offs", i64, None, ANY), (bm32, "bm32", i16, None, ANY),
                      (bm32_offs, "bm32_offs", i64, None, ANY), (segs, "segs", i64, None, ANY),
                      (resid, "resid", u8, None, ANY)])
    _call("mvm_lsap_solve_resid", _p(dims), status.numel(), _p(ws_offs), _p(out_offs), _p(workspace),
          workspace.numel(), _p(row_ind), _p(col_ind), _p(status), long_min, long_max, short_max,
          _p(bmin8), _p(bmin8_offs), _p(bm32), _p(bm32_offs), _p(segs), _p(resid), max_n,
          _opts_ref(opts), _stream(dims))


@_gpu_op("pack_detections_out", ("counts", "cam_offs", "pts", "boxes_out", "status"))
def pack_detections_out(boxes: Tensor, conf: Tensor, cls: Tensor, img_offs: Tensor,
                        conf_thresh: float, class_id: float, counts: Tensor, cam_offs: Tensor,
                        pts: Tensor, boxes_out: Tensor, status: Tensor) -> None:
    dev = _gpu(boxes, "boxes", "packer")
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError("boxes must be [n, 4] (xyxy)")
    n, n_img = boxes.shape[0], counts.numel()
    _check_args(dev, [(boxes, "boxes", f32, 4 * n, AT_LEAST), (conf, "conf", f32, n, AT_LEAST),
                      (cls, "cls", f32, n, AT_LEAST), (img_offs, "img_offs", i64, n_img + 1, AT_LEAST),
                      (counts, "counts", i32, n_img, AT_LEAST),
                      (cam_offs, "cam_offs", i64, n_img + 1, AT_LEAST), (pts, "pts", f64, 2 * n, AT_LEAST),
                      (boxes_out, "boxes_out", i32, 4 * n, AT_LEAST), (status, "status", i32, 1, AT_LEAST)])
    _call("mvm_pack_detections", _p(boxes), _p(conf), _p(cls), _p(img_offs), n_img, float(conf_thresh),
          float(class_id), _p(counts), _p(cam_offs), _p(pts), _p(boxes_out), _p(status),
          _stream(boxes))


@_gpu_op("triangulate_dlt_out", ("X",))
def triangulate_dlt_out(proj: Tensor, set_of_point: Optional[Tensor], pts2d: Tensor,
                        X: Tensor) -> None:
    dev = _gpu(pts2d, "pts2d", "triangulator")
    if pts2d.dim() != 3 or pts2d.shape[2] != 2:
        raise ValueError("pts2d must be [n_points, n_views, 2]")
    n_points, n_views = int(pts2d.shape[0]), int(pts2d.shape[1])
    rows = [(pts2d, "pts2d", f64, None, ANY), (proj, "proj", f64, None, ANY),
            (X, "X", f64, 3 * n_points, AT_LEAST)]
    if set_of_point is not None:
        rows.append((set_of_point, "set_of_point", i32, n_points, EXACT))
    _check_args(dev, rows)
    if proj.dim() != 4 or tuple(proj.shape[1:]) != (n_views, 3, 4):
        raise ValueError("proj must be [n_sets, n_views, 3, 4]")
    if set_of_point is None and proj.shape[0] < n_points:
        raise ValueError("without set_of_point, proj needs one set per point")
    _call("mvm_triangulate_dlt", _p(proj), _p(set_of_point), _p(pts2d), n_points, n_views, _p(X),
          _stream(pts2d))


@_gpu_op("select_triangulate_out", ("match", "cost", "X", "count"))
def select_triangulate_out(cube: Tensor, cube_offs: Tensor, cam_offs: Tensor, lsap_offs: Tensor,
                           row_ind: Tensor, col_ind: Tensor, pts: Tensor, proj: Tensor,
                           threshold: float, match: Tensor, cost: Tensor, X: Tensor,
                           count: Tensor) -> None:
    dev = _gpu(cube, "cube")
    n_scenes, n_out = count.numel(), row_ind.numel()
    _check_args(dev, [(cube, "cube", f32, None, ANY), (cube_offs, "cube_offs", i64, n_scenes + 1, EXACT),
                      (cam_offs, "cam_offs", i64, 3 * n_scenes + 1, EXACT),
                      (lsap_offs, "lsap_offs", i64, n_scenes + 1, EXACT),
                      (row_ind, "row_ind", i64, None, ANY), (col_ind, "col_ind", i64, None, ANY),
                      (pts, "pts", f64, None, ANY),
                      (proj, "proj", f64, 36 * n_scenes, EXACT if n_scenes else ANY),   # no scene: not read
                      (match, "match", i32, 3 * n_out, AT_LEAST), (cost, "cost", f32, n_out, AT_LEAST),
                      (X, "X", f64, 3 * n_out, AT_LEAST), (count, "count", i32, None, ANY)])
    if col_ind.numel() != n_out:
        raise ValueError("row_ind / col_ind differ in length")
    _call("mvm_select_triangulate", _p(cube), _p(cube_offs), _p(cam_offs), _p(lsap_offs), _p(row_ind),
          _p(col_ind), _p(pts), _p(proj), n_scenes, float(threshold), _p(match), _p(cost), _p(X),
          _p(count), _stream(cube))


@_gpu_op("select_triangulate_resid_out", ("match", "cost", "X", "count"))
def select_triangulate_resid_out(resid: Tensor, max_n: int, cam_offs: Tensor, lsap_offs: Tensor,
                                 row_ind: Tensor, col_ind: Tensor, pts: Tensor, proj: Tensor,
                                 threshold: float, match: Tensor, cost: Tensor, X: Tensor,
                                 count: Tensor) -> None:
    """select_triangulate_out with each assigned entry recomputed from a
    triplet_minima batch's residuals (mvm_select_triangulate_resid, ABI 7)."""
    dev = _gpu(pts, "pts")
    n_scenes, n_out = count.numel(), row_ind.numel()
    _check_args(dev, [(resid, "resid", u8, None, ANY), (cam_offs, "cam_offs", i64, 3 * n_scenes + 1, EXACT),
                      (lsap_offs, "lsap_offs", i64, n_scenes + 1, EXACT),
                      (row_ind, "row_ind", i64, None, ANY), (col_ind, "col_ind", i64, None, ANY),
                      (pts, "pts", f64, None, ANY),
                      (proj, "proj", f64, 36 * n_scenes, EXACT if n_scenes else ANY),   # no scene: not read
                      (match, "match", i32, 3 * n_out, AT_LEAST), (cost, "cost", f32, n_out, AT_LEAST),
                      (X, "X", f64, 3 * n_out, AT_LEAST), (count, "count", i32, None, ANY)])
    if col_ind.numel() != n_out:
        raise ValueError("row_ind / col_ind differ in length")
    _call("mvm_select_triangulate_resid", _p(resid), max_n, _p(cam_offs), _p(lsap_offs), _p(row_ind),
          _p(col_ind), _p(pts), _p(proj), n_scenes, float(threshold), _p(match), _p(cost), _p(X),
          _p(count), _stream(pts))


@_gpu_op("compact_matches_out", ("dense_offs", "scene_out", "match_out", "cost_out", "X_out", "boxes_out",
                                 "cent_out"))
def compact_matches_out(match: Tensor, cost: Tensor, X: Tensor, count: Tensor, seg_offs: Tensor,
                        pts: Tensor, boxes: Tensor, cam_offs: Tensor, scene_base: int,
                        dense_offs: Tensor, scene_out: Tensor, match_out: Tensor, cost_out: Tensor,
                        X_out: Tensor, boxes_out: Tensor, cent_out: Tensor) -> None:
    """The select kernels' matches as dense, self-contained rows
    (mvm_compact_matches, ABI 8).  Outputs hold ``match.shape[0]`` rows."""
    dev = _gpu(match, "match", "table")
    if match.dim() != 2 or match.shape[1] != 3:
        raise ValueError("match must be [cap, 3]")
    n_scenes, cap = count.numel(), int(match.shape[0])
    _check_args(dev, [(match, "match", i32, 3 * cap, AT_LEAST), (cost, "cost", f32, cap, AT_LEAST),
                      (X, "X", f64, 3 * cap, AT_LEAST), (count, "count", i32, n_scenes, AT_LEAST),
                      (seg_offs, "seg_offs", i64, n_scenes + 1, EXACT),
                      (pts, "pts", f64, None, ANY), (boxes, "boxes", i32, None, ANY),
                      (cam_offs, "cam_offs", i64, 3 * n_scenes + 1, EXACT),
                      (dense_offs, "dense_offs", i64, n_scenes + 1, EXACT),
                      (scene_out, "scene_out", i32, cap, AT_LEAST),
                      (match_out, "match_out", i32, 3 * cap, AT_LEAST),
                      (cost_out, "cost_out", f32, cap, AT_LEAST), (X_out, "X_out", f64, 3 * cap, AT_LEAST),
                      (boxes_out, "boxes_out", i32, 12 * cap, AT_LEAST),
                      (cent_out, "cent_out", f64, 6 * cap, AT_LEAST)])
    if boxes.numel() != 2 * pts.numel():
        raise ValueError("pts [n, 2] and boxes [n, 4] differ in rows")
    _call("mvm_compact_matches", _p(match), _p(cost), _p(X), _p(count), _p(seg_offs), _p(pts),
          _p(boxes), _p(cam_offs), n_scenes, int(scene_base), _p(dense_offs), _p(scene_out),
          _p(match_out), _p(cost_out), _p(X_out), _p(boxes_out), _p(cent_out), _stream(match))


@_gpu_op("compact_matches_views_out", ("dense_offs", "scene_out", "views_out", "n_views_out", "cost_out",
                                       "ext_cost_out", "X_out", "boxes_out", "cent_out", "reproj_out"))
def compact_matches_views_out(views: Tensor, cost: Tensor, ext_cost: Tensor, X: Tensor, count: Tensor,
                              seg_offs: Tensor, pts: Tensor, boxes: Tensor, cam_offs: Tensor,
                              proj: Tensor, scene_base: int, dense_offs: Tensor, scene_out: Tensor,
                              views_out: Tensor, n_views_out: Tensor, cost_out: Tensor,
                              ext_cost_out: Tensor, X_out: Tensor, boxes_out: Tensor, cent_out: Tensor,
                              reproj_out: Tensor) -> None:
    """The matches of a C-camera batch as dense, self-contained rows with the
    reprojection residual of every kept view (mvm_compact_matches_views).
    ``views`` [cap, C] gives C; outputs hold ``cap`` rows."""
    dev = _gpu(views, "views", "table")
    n_scenes = count.numel()
    if views.dim() != 2 or not 3 <= views.shape[1] <= _native.MVM_MAX_CAMS:
        raise ValueError(f"views must be [cap, C], 3 <= C <= {_native.MVM_MAX_CAMS}")
    cap, C = int(views.shape[0]), int(views.shape[1])
    _check_args(dev, [(views, "views", i32, C * cap, AT_LEAST), (cost, "cost", f32, cap, AT_LEAST),
                      (ext_cost, "ext_cost", f32, (C - 3) * cap, AT_LEAST),
                      (X, "X", f64, 3 * cap, AT_LEAST), (count, "count", i32, n_scenes, AT_LEAST),
                      (seg_offs, "seg_offs", i64, n_scenes + 1, EXACT),
                      (pts, "pts", f64, None, ANY), (boxes, "boxes", i32, None, ANY),
                      (cam_offs, "cam_offs", i64, C * n_scenes + 1, EXACT),
                      (proj, "proj", f64, 12 * C * n_scenes, EXACT if n_scenes else ANY),   # no scene: not read
                      (dense_offs, "dense_offs", i64, n_scenes + 1, EXACT),
                      (scene_out, "scene_out", i32, cap, AT_LEAST),
                      (views_out, "views_out", i32, C * cap, AT_LEAST),
                      (n_views_out, "n_views_out", i32, cap, AT_LEAST),
                      (cost_out, "cost_out", f32, cap, AT_LEAST),
                      (ext_cost_out, "ext_cost_out", f32, (C - 3) * cap, AT_LEAST),
                      (X_out, "X_out", f64, 3 * cap, AT_LEAST),
                      (boxes_out, "boxes_out", i32, 4 * C * cap, AT_LEAST),
                      (cent_out, "cent_out", f64, 2 * C * cap, AT_LEAST),
                      (reproj_out, "reproj_out", f64, C * cap, AT_LEAST)])
    if boxes.numel() != 2 * pts.numel():
        raise ValueError("pts [n, 2] and boxes [n, 4] differ in rows")
    _call("mvm_compact_matches_views", _p(views), _p(cost), _p(ext_cost), _p(X), _p(count), _p(seg_offs),
          _p(pts), _p(boxes), _p(cam_offs), _p(proj), n_scenes, C, int(scene_base), _p(dense_offs),
          _p(scene_out), _p(views_out), _p(n_views_out), _p(cost_out), _p(ext_cost_out), _p(X_out),
          _p(boxes_out), _p(cent_out), _p(reproj_out), _stream(views))


@_gpu_op("rig_matrices_out", ("F", "proj", "status"))
def rig_matrices_out(K: Tensor, RT: Tensor, pair_a: List[int], pair_b: List[int], F: Tensor,
                     proj: Tensor, status: Tensor) -> None:
    """F of every (capture, pair) and P = K @ RT[:3] of every (capture, camera)
    on the device (mvm_rig_matrices).  ``proj`` empty: not produced."""
    dev = _gpu(K, "K", "rig kernel")
    if K.dim() != 4 or tuple(K.shape[2:]) != (3, 3):
        raise ValueError(f"K: expected [S, C, 3, 3], got {tuple(K.shape)}")
    S, C = int(K.shape[0]), int(K.shape[1])
    if tuple(RT.shape) != (S, C, 4, 4):
        raise ValueError(f"RT: expected {(S, C, 4, 4)}, got {tuple(RT.shape)}")
    pa, pb = _pair_arrays(pair_a, pair_b)
    n_pairs = len(pair_a)
    _check_args(dev, [(K, "K", f32, 9 * S * C, EXACT), (RT, "RT", f64, 16 * S * C, EXACT),
                      (F, "F", f64, 9 * S * n_pairs, EXACT),
                      (proj, "proj", f64, 12 * S * C if proj.numel() else 0, EXACT),
                      (status, "status", i32, S, EXACT)])
    _call("mvm_rig_matrices", _p(K), _p(RT), pa, pb, S, C, n_pairs, _p(F), _p(proj), _p(status),
          _stream(K))


@_gpu_op("extend_costs_out", ("E",))
def extend_costs_out(pts: Tensor, cam_offs: Tensor, F_ext: Tensor, match: Tensor, match_offs: Tensor,
                     count: Tensor, ext_offs: Tensor, n_cams: int, max_rows: int, E: Tensor) -> None:
    """The extension cost matrices E_d of every (capture, extra camera)
    (mvm_extend_costs)."""
    dev = _gpu(pts, "pts")
    n_scenes = count.numel()
    n_ext = n_cams - 3
    if n_ext < 0 or n_cams > _native.MVM_MAX_CAMS:
        raise ValueError(f"n_cams: expected 3..{_native.MVM_MAX_CAMS}, got {n_cams}")
    if match.dim() != 2 or match.shape[1] != 3:
        raise ValueError("match must be [cap, 3]")
    _check_args(dev, [(pts, "pts", f64, None, ANY), (cam_offs, "cam_offs", i64, n_cams * n_scenes + 1, EXACT),
                      # no scene or no extra camera: not read
                      (F_ext, "F_ext", f64, 27 * n_ext * n_scenes, EXACT if n_ext and n_scenes else ANY),
                      (match, "match", i32, None, ANY),
                      (match_offs, "match_offs", i64, n_scenes + 1, EXACT),
                      (count, "count", i32, n_scenes, EXACT),
                      (ext_offs, "ext_offs", i64, n_ext * n_scenes + 1, EXACT), (E, "E", f32, None, ANY)])
    if n_scenes == 0 or n_ext == 0 or max_rows == 0 or E.numel() == 0:
        return                       # no matrix has an entry: nothing to launch
    _call("mvm_extend_costs", _p(pts), _p(cam_offs), _p(F_ext), _p(match), _p(match_offs), _p(count),
          _p(ext_offs), n_scenes, n_cams, int(max_rows), _p(E), _stream(pts))


@_gpu_op("extend_select_triangulate_out", ("views", "ext_cost", "X"))
def extend_select_triangulate_out(E: Tensor, ext_offs: Tensor, lsap_offs: Tensor, row_ind: Tensor,
                                  col_ind: Tensor, match: Tensor, match_offs: Tensor, count: Tensor,
                                  pts: Tensor, cam_offs: Tensor, proj: Tensor, threshold: float,
                                  views: Tensor, ext_cost: Tensor, X: Tensor) -> None:
    """Threshold + scatter of the extension's assignments and the V-view DLT
    (mvm_extend_select_triangulate).  ``X`` is in/out."""
    dev = _gpu(match, "match")
    n_scenes = count.numel()
    if views.dim() != 2 or not 3 <= views.shape[1] <= _native.MVM_MAX_CAMS:
        raise ValueError(f"views must be [cap, C], 3 <= C <= {_native.MVM_MAX_CAMS}")
    cap, n_cams = int(views.shape[0]), int(views.shape[1])
    n_ext = n_cams - 3
    if match.dim() != 2 or tuple(match.shape) != (cap, 3):
        raise ValueError(f"match must be [{cap}, 3] (the rows of views)")
    _check_args(dev, [(E, "E", f32, None, ANY), (ext_offs, "ext_offs", i64, n_ext * n_scenes + 1, EXACT),
                      (lsap_offs, "lsap_offs", i64, n_ext * n_scenes + 1, EXACT),
                      (row_ind, "row_ind", i64, None, ANY), (col_ind, "col_ind", i64, None, ANY),
                      (match, "match", i32, 3 * cap, EXACT),
                      (match_offs, "match_offs", i64, n_scenes + 1, EXACT),
                      (count, "count", i32, n_scenes, EXACT), (pts, "pts", f64, None, ANY),
                      (cam_offs, "cam_offs", i64, n_cams * n_scenes + 1, EXACT),
                      (proj, "proj", f64, 12 * n_cams * n_scenes, EXACT),
                      (views, "views", i32, n_cams * cap, EXACT),
                      (ext_cost, "ext_cost", f32, n_ext * cap, EXACT), (X, "X", f64, 3 * cap, EXACT)])
    if col_ind.numel() != row_ind.numel():
        raise ValueError("row_ind / col_ind differ in length")
    if n_scenes == 0 or n_ext == 0 or cap == 0:
        return                       # no row to fill: nothing to launch
    _call("mvm_extend_select_triangulate", _p(E), _p(ext_offs), _p(lsap_offs), _p(row_ind), _p(col_ind),
          _p(match), _p(match_offs), _p(count), _p(pts), _p(cam_offs), _p(proj), n_scenes, n_cams,
          float(threshold), _p(views), _p(ext_cost), _p(X), _stream(match))


# ---------------------------------------------------------------- plans ----
class PairwisePlan:
    """Offsets of every (scene, pair) residual matrix and argmin row block.

    Built on the host from ``cam_offs`` (the per-view counts are host
    knowledge: they come from the detector), copied once to ``device``.

    ``row_align``: rows of matrix (s, p) are ``ld = roundup(n_b, row_align)``
    floats apart (include/mvmatch.h, mvm_pairwise_residual_argmin_pitched).
    1 (the default) is the unpitched layout: matrices back to back, rows of
    n_b floats.  "auto" (what the bench and the batch paths ask for) pitches
    rows to 128-byte lines (32 floats) when some view's count is not a
    multiple of 32 -- the ragged views real detectors produce, whose unpitched
    rows would start mid-line, ~1.4x slower per byte -- and keeps the
    unpitched layout otherwise (then the two are the same).  ``matrix()``
    returns the (n_a, n_b) view of a matrix either way; ``compact()`` the
    unpitched flat layout.
    """

    def __init__(self, cam_offs: np.ndarray, n_scenes: int, n_cams: int, pairs,
                 device: torch.device | str = "cuda", row_align=1):
        cam_offs = np.asarray(cam_offs, dtype=np.int64)
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        counts = np.diff(cam_offs).reshape(n_scenes, n_cams)
        na = counts[:, pairs[:, 0]].reshape(-1)
        nb = counts[:, pairs[:, 1]].reshape(-1)
        if row_align == "auto":
            row_align = 32 if (nb % 32).any() else 1
        row_align = int(row_align)
        if row_align < 1 or row_align > 256 or row_align & (row_align - 1):
            raise ValueError(f"row_align {row_align}: a power of two in [1, 256]")
        ld = (nb + row_align - 1) // row_align * row_align
        dist_offs = np.zeros(na.size + 1, np.int64)
        row_offs = np.zeros(na.size + 1, np.int64)
        np.cumsum(na * ld, out=dist_offs[1:])
        np.cumsum(na, out=row_offs[1:])
        self.n_scenes, self.n_cams = int(n_scenes), int(n_cams)
        self.pairs = pairs
        self.pair_a = [int(a) for a in pairs[:, 0]]
        self.pair_b = [int(b) for b in pairs[:, 1]]
        self.max_rows = int(na.max()) if na.size else 0
        self.max_cols = int(nb.max()) if nb.size else 0
        self.max_n = max(self.max_rows, self.max_cols)
        self.na, self.nb, self.ld = na, nb, ld
        self.row_align = row_align
        self.n_dist = int((na * nb).sum())      # residuals (pairs)
        self.dist_size = int(dist_offs[-1])     # floats of the (pitched) output
        self.n_rows = int(row_offs[-1])
        self.dist_offs_host, self.row_offs_host = dist_offs, row_offs
        self.device = torch.device(device)
        self.dist_offs, self.row_offs = _h2d_int64([dist_offs, row_offs], self.device)

    def matrix(self, dist: Tensor, scene: int, pair: int) -> Tensor:
        """(n_a, n_b) view of the (scene, pair) residual matrix inside ``dist``
        (strided when the rows are pitched)."""
        sp = scene * len(self.pair_a) + pair
        o = int(self.dist_offs_host[sp])
        na, nb, ld = int(self.na[sp]), int(self.nb[sp]), int(self.ld[sp])
        return dist[o:o + na * ld].view(na, ld)[:, :nb]

    def compact(self, dist: Tensor) -> Tensor:
        """The residuals in the unpitched layout (matrices back to back, rows
        of n_b): ``dist`` itself when the plan is unpitched, else a copy."""
        if self.dist_size == self.n_dist:
            return dist[:self.n_dist]
        parts = [self.matrix(dist, sp // len(self.pair_a), sp % len(self.pair_a)).reshape(-1)
                 for sp in range(self.na.size)]
        return torch.cat(parts) if parts else dist[:0]


def pairwise_residual_argmin(pts: Tensor, cam_offs: Tensor, F: Tensor, plan: PairwisePlan, *,
                             want_dist: bool = True,
                             out: Optional[Tuple[Tensor, Tensor, Tensor]] = None,
                             options: Optional[dict] = None):
    """-> (dist f32 [plan.dist_size], argmin i32 [plan.n_rows], minval f32 [plan.n_rows]).
    ``dist`` has the plan's (possibly pitched) layout: ``plan.matrix()`` /
    ``plan.compact()`` read it.  ``options``: mvm_options fields, e.g.
    ``{"pairwise_argmin": "eager"}``."""
    dev = pts.device
    if out is None:
        dist = torch.empty(plan.dist_size if want_dist else 0, dtype=torch.float32, device=dev)
        argmin = torch.empty(plan.n_rows, dtype=torch.int32, device=dev)
        minval = torch.empty(plan.n_rows, dtype=torch.float32, device=dev)
    else:
        dist, argmin, minval = out
    if not (options or {}).get("pairwise_xcd_fronts"):
        # the library's default front count is sized from the padded bound
        # (scenes x pairs x max rows x max columns); the plan knows the bytes
        # this launch really writes: 4 fronts per XCD from 8 GB
        options = dict(options or {})
        options["pairwise_xcd_fronts"] = 4 if (dist.numel() and 4.0 * plan.dist_size >= 8e9) else 1
    torch.ops.mvmatch.pairwise_residual_argmin_out(
        pts, cam_offs, F, plan.pair_a, plan.pair_b, plan.n_scenes, plan.n_cams, plan.max_n,
        plan.dist_offs, plan.row_offs, dist, argmin, minval, _opts_list(options), plan.row_align)
    return dist, argmin, minval


def pairwise_residual_f64(pts: Tensor, cam_offs: Tensor, F: Tensor, plan: PairwisePlan):
    """fp64 residual matrices -> Tensor [S*P, max_rows, ld] (padding unspecified)."""
    ld = (max(plan.max_cols, 1) + 3) // 4 * 4
    rows = max(plan.max_rows, 1)
    e = torch.zeros(plan.n_scenes * len(plan.pair_a) * rows * ld, dtype=torch.float64,
                    device=pts.device)
    torch.ops.mvmatch.pairwise_residual_f64_out(
        pts, cam_offs, F, plan.pair_a, plan.pair_b, plan.n_scenes, plan.n_cams, plan.max_n,
        rows * ld, ld, e)
    return e.view(plan.n_scenes * len(plan.pair_a), rows, ld)


class TripletPlan:
    """Offsets + workspace for batched 3-camera cubes (cam_offs has S*3+1 entries)."""

    def __init__(self, cam_offs: np.ndarray, n_scenes: int, device: torch.device | str = "cuda"):
        cam_offs = np.asarray(cam_offs, dtype=np.int64)
        counts = np.diff(cam_offs).reshape(n_scenes, 3)
        rows = counts[:, 0] * counts[:, 1]
        cube_offs = np.zeros(n_scenes + 1, np.int64)
        row_offs = np.zeros(n_scenes + 1, np.int64)
        np.cumsum(rows * counts[:, 2], out=cube_offs[1:])
        np.cumsum(rows, out=row_offs[1:])
        self.n_scenes = int(n_scenes)
        self.counts = counts
        self.max_n = int(counts.max()) if counts.size else 0
        self.n_cube = int(cube_offs[-1])
        self.n_rows = int(row_offs[-1])
        self.cube_offs_host, self.row_offs_host = cube_offs, row_offs
        self.device = torch.device(device)
        self.cube_offs, self.row_offs = _h2d_int64([cube_offs, row_offs], self.device)
        self.workspace_bytes = int(_native.load().mvm_triplet_workspace_bytes(self.n_scenes,
                                                                               self.max_n))
        # the cube's 8-row minima for the assignment (mvm_triplet_cost_argmin_bmin8):
        # N * ceil(M/8) rows of P 16-bit keys per scene, scenes 4 keys aligned
        # (the kernel's 8-byte stores)
        bm8 = np.zeros(n_scenes + 1, np.int64)
        np.cumsum((counts[:, 0] * ((counts[:, 1] + 7) // 8) * counts[:, 2] + 3) // 4 * 4, out=bm8[1:])
        self.bmin8_offs_host = bm8
        self.n_bmin8 = int(bm8[-1])
        # the cube-free path's 32-column block minima (mvm_triplet_minima): per
        # scene P rows of ceil(M/32) * roundup(N, 16) 16-bit keys (32-byte runs)
        b32 = np.zeros(n_scenes + 1, np.int64)
        np.cumsum(counts[:, 2] * ((counts[:, 1] + 31) // 32) * ((counts[:, 0] + 15) // 16 * 16), out=b32[1:])
        self.bm32_offs_host = b32
        self.n_bm32 = int(b32[-1])
        self.bmin8_offs, self.segs, self.bm32_offs = _h2d_int64(
            [bm8, np.ascontiguousarray(counts[:, 1]), b32], self.device)
        self.workspace = torch.empty(max(self.workspace_bytes, 16), dtype=torch.uint8,
                                     device=self.device)


def triplet_cost_argmin(pts: Tensor, cam_offs: Tensor, F: Tensor, plan: TripletPlan, *,
                        want_cube: bool = True,
                        out: Optional[Tuple[Tensor, Tensor, Tensor]] = None,
                        options: Optional[dict] = None, bmin8: Optional[Tensor] = None):
    """-> (cube f32 [plan.n_cube], argmin i32 [plan.n_rows], minval f32 [plan.n_rows]).
    ``options``: mvm_options fields, e.g. ``{"cube_kernel": "workspace"}``.
    ``bmin8`` (int16 [plan.n_bmin8]): also the 8-row minima that
    ``linear_sum_assignment_batched(..., bmin8=)`` reduces (needs the cube)."""
    dev = pts.device
    if out is None:
        cube = torch.empty(plan.n_cube if want_cube else 0, dtype=torch.float32, device=dev)
        argmin = torch.empty(plan.n_rows, dtype=torch.int32, device=dev)
        minval = torch.empty(plan.n_rows, dtype=torch.float32, device=dev)
    else:
        cube, argmin, minval = out
    if bmin8 is not None:
        torch.ops.mvmatch.triplet_cost_bmin8_out(
            pts, cam_offs, F, plan.n_scenes, plan.max_n, plan.cube_offs, plan.row_offs, cube, argmin,
            minval, bmin8, plan.bmin8_offs, plan.workspace, _opts_list(options))
        return cube, argmin, minval
    torch.ops.mvmatch.triplet_cost_argmin_out(
        pts, cam_offs, F, plan.n_scenes, plan.max_n, plan.cube_offs, plan.row_offs, cube, argmin,
        minval, plan.workspace, _opts_list(options))
    return cube, argmin, minval


def triplet_minima(pts: Tensor, cam_offs: Tensor, F: Tensor, plan: TripletPlan, *,
                   bmin8: Optional[Tensor] = None, bm32: Optional[Tensor] = None,
                   with_bmin8: bool = True, options: Optional[dict] = None):
    """Cube-free input of the assignment (mvm_triplet_minima, ABI 7): the
    cube's 8-row minima (int16 [plan.n_bmin8], the same bits
    ``triplet_cost_argmin(..., bmin8=)`` writes), the assignment's 32-column
    block minima (16-bit keys, int16 [plan.n_bm32]) and every scene's fp64 pair residuals,
    written into ``plan.workspace`` (which the default cube kernels do not
    use; a later cube launch on the plan with the workspace kernel would
    overwrite them).  -> (bmin8, bm32).  Views of at most 256 detections.
    ``with_bmin8=False``: no 8-row minima (bmin8 an empty tensor; the
    assignment then gathers whole 32-column candidate blocks)."""
    if not with_bmin8:
        bmin8 = torch.empty(0, dtype=torch.int16, device=pts.device)
    elif bmin8 is None:
        bmin8 = torch.empty(max(plan.n_bmin8, 1), dtype=torch.int16, device=pts.device)
    if bm32 is None:
        bm32 = torch.empty(max(plan.n_bm32, 8), dtype=torch.int16, device=pts.device)
    torch.ops.mvmatch.triplet_minima_out(pts, cam_offs, F, plan.n_scenes, plan.max_n, bmin8,
                                         plan.bmin8_offs, bm32, plan.bm32_offs, plan.workspace,
                                         _opts_list(options))
    return bmin8, bm32


def sparse_class_bounds() -> Tuple[int, int, int]:
    """(default lower bound of the long side, largest long side, largest
    short side) of the candidate-list assignment class (mvm_lsap_sparse_bounds)."""
    v = [ctypes.c_int32(0) for _ in range(3)]
    _native.load().mvm_lsap_sparse_bounds(*(ctypes.byref(x) for x in v))
    return tuple(int(x.value) for x in v)


def sparse_class(long_side, short_side, min_cols: Optional[int] = None) -> np.ndarray:
    """Per assignment problem, given its longer and shorter side: True where
    it is of the candidate-list class (``sparse_class_bounds``; ``min_cols``:
    the lower bound of the long side if not the default).  The one statement
    of that predicate on the Python side: what else a caller needs (a
    non-empty problem, views the minima kernel takes) it adds itself."""
    lo, hi, sh = sparse_class_bounds()
    lo = lo if min_cols is None else int(min_cols)
    return (long_side >= lo) & (long_side > 1024) & (long_side <= hi) & (short_side <= sh)


def cube_free_scenes(counts: np.ndarray, min_cols: Optional[int] = None) -> np.ndarray:
    """Per scene of a (S, 3) count array: True where the cube-free association
    (triplet_minima -> linear_sum_assignment_resid -> select_triangulate_resid)
    can take it: views of <= 256 detections (what the minima kernel takes) and
    either an empty problem or a flattened (N*M, P) problem of the
    candidate-list class."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    nm, p = c[:, 0] * c[:, 1], c[:, 2]
    empty = (nm == 0) | (p == 0)
    ok = sparse_class(np.maximum(nm, p), np.minimum(nm, p), min_cols)
    return (empty | ok) & (c.max(axis=1) <= 256)


def hbm_write_probe(buf: Tensor) -> None:
    """Stream 16-byte nontemporal stores over ``buf`` (roofline reference)."""
    if buf.device.type != "cuda" or not buf.is_contiguous():
        raise ValueError("hbm_write_probe needs a contiguous GPU tensor")
    nbytes = buf.numel() * buf.element_size() // 16 * 16
    _call("mvm_hbm_write_probe", _p(buf), nbytes, _stream(buf))


class LsapPlan:
    """Workspace / output layout of a batch of assignment problems (host dims)
    whose costs are ``dtype`` (float32, or float64 as scipy assigns a float64
    matrix: the workspace holds transposed costs of that type)."""

    def __init__(self, rows, cols, device: torch.device | str = "cuda",
                 dtype: torch.dtype = torch.float32, resid: bool = False):
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"LsapPlan: dtype must be float32 or float64, got {dtype}")
        if resid and dtype != torch.float32:
            raise ValueError("LsapPlan: the cube-free form assigns float32 cube entries")
        n = rows.size
        ws_offs = np.zeros(n + 1, np.int64)
        out_offs = np.zeros(n + 1, np.int64)
        if resid:      # cube-free (mvm_lsap_solve_resid): the candidate lists only
            fn = "mvm_lsap_plan_resid"
            total = _native.load().mvm_lsap_plan_resid(n, rows.ctypes.data, cols.ctypes.data,
                                                       ws_offs.ctypes.data, out_offs.ctypes.data)
        else:
            fn = "mvm_lsap_plan_ex"
            code = _native.MVM_F64 if dtype == torch.float64 else _native.MVM_F32
            total = _native.load().mvm_lsap_plan_ex(n, rows.ctypes.data, cols.ctypes.data, code,
                                                    ws_offs.ctypes.data, out_offs.ctypes.data)
        if total < 0:
            raise _native.MvmError(fn, -1, _native.load().mvm_last_error_string().decode())
        self.resid = bool(resid)
        self.ws_offs_host = ws_offs
        self.dtype = dtype
        self.n = n
        self.rows, self.cols = rows, cols
        self.out_offs_host = out_offs
        self.device = torch.device(device)
        self.dims, self.ws_offs, self.out_offs = _h2d_int64(
            [np.stack([rows, cols], axis=1).reshape(-1), ws_offs, out_offs], self.device)
        self.workspace = torch.empty(max(int(total), 16), dtype=torch.uint8, device=self.device)
        self.n_out = int(out_offs[-1])
        longs = np.maximum(rows, cols)[(rows > 0) & (cols > 0)]
        self.long_min = int(longs.min()) if longs.size else 0     # bounds for the launch
        self.long_max = int(longs.max()) if longs.size else 0
        shorts = np.minimum(rows, cols)[(rows > 0) & (cols > 0)]
        self.short_max = int(shorts.max()) if shorts.size else 0


def _assignment_outputs(plan: LsapPlan, dev: torch.device) -> Tuple[Tensor, Tensor, Tensor]:
    """(row_ind i64, col_ind i64, status i32 [n]) for the solvers to write;
    the index arrays hold max(plan.n_out, 1) entries."""
    return (torch.empty(max(plan.n_out, 1), dtype=i64, device=dev),
            torch.empty(max(plan.n_out, 1), dtype=i64, device=dev),
            torch.empty(plan.n, dtype=i32, device=dev))


def linear_sum_assignment_batched(cost: Tensor, cost_offs: Tensor, plan: LsapPlan, *,
                                  options: Optional[dict] = None,
                                  bmin8: Optional[Tuple[Tensor, Tensor, Tensor]] = None):
    """scipy.optimize.linear_sum_assignment for every problem of ``plan`` on the GPU.
    -> (row_ind i64 [n_out], col_ind i64 [n_out], status i32 [n]) device tensors.
    ``cost`` must have the plan's dtype.  ``bmin8`` = (keys, the TripletPlan's
    bmin8_offs, its segs) when the costs are the flattened cubes of a
    ``triplet_cost_argmin(..., bmin8=keys)`` call: the assignment then reduces
    those instead of reading every cost once more (same result)."""
    if cost.dtype != plan.dtype:
        raise ValueError(f"cost is {cost.dtype} but the plan was built for {plan.dtype}")
    row_ind, col_ind, status = _assignment_outputs(plan, cost.device)
    if bmin8 is not None and cost.dtype == torch.float32:
        torch.ops.mvmatch.lsap_solve_bmin8_out(cost, cost_offs, plan.dims, plan.ws_offs, plan.out_offs,
                                               plan.workspace, row_ind, col_ind, status, bmin8[0],
                                               bmin8[1], bmin8[2], plan.long_min, plan.long_max,
                                               plan.short_max, _opts_list(options))
    else:
        torch.ops.mvmatch.lsap_solve_out(cost, cost_offs, plan.dims, plan.ws_offs, plan.out_offs,
                                         plan.workspace, row_ind, col_ind, status, plan.long_min,
                                         plan.long_max, _opts_list(options), plan.short_max)
    return row_ind[:plan.n_out], col_ind[:plan.n_out], status


def lsap_sparse_stats(plan: LsapPlan, min_cols: Optional[int] = None) -> np.ndarray:
    """After a solve with ``plan``: per problem the candidate-list solver's
    counters (mvm_lsap_sparse_stats_offset) -- int64 [n, 4] = dense free-minimum
    scans, dense tie scans, overflowed lists, Dijkstra steps; -1 for problems
    outside the class (``min_cols``: its lower bound if not the default)."""
    lib = _native.load()
    lng, sht = np.maximum(plan.rows, plan.cols), np.minimum(plan.rows, plan.cols)
    cls = sparse_class(lng, sht, min_cols) & (sht >= 1)
    out = np.full((plan.n, 4), -1, np.int64)
    if not cls.any():
        return out
    ps = np.nonzero(cls)[0]
    offs = np.array([plan.ws_offs_host[p] + lib.mvm_lsap_sparse_stats_offset(int(plan.rows[p]),
                                                                             int(plan.cols[p]))
                     for p in ps], np.int64)
    idx = torch.from_numpy((offs[:, None] // 4 + np.arange(4)).reshape(-1)).to(plan.workspace.device)
    words = plan.workspace[:plan.workspace.numel() // 4 * 4].view(torch.int32)
    out[ps] = words.index_select(0, idx).cpu().numpy().reshape(-1, 4)
    return out


def linear_sum_assignment_resid(plan: LsapPlan, tplan: TripletPlan, minima, *,
                                options: Optional[dict] = None):
    """linear_sum_assignment_batched of every flattened (N*M, P) cube of a
    ``triplet_minima(..., tplan)`` batch without the cubes (mvm_lsap_solve_resid):
    the same result (scipy's).  ``plan`` = LsapPlan(N*M, P, resid=True);
    ``minima`` = what triplet_minima returned (bmin8, bm32).
    -> (row_ind, col_ind, status) as linear_sum_assignment_batched; status 4:
    a problem outside the candidate-list class (cube_free_scenes)."""
    if not plan.resid:
        raise ValueError("linear_sum_assignment_resid needs LsapPlan(..., resid=True)")
    bmin8, bm32 = minima                  # what triplet_minima returned (bmin8 may be empty)
    row_ind, col_ind, status = _assignment_outputs(plan, bm32.device)
    torch.ops.mvmatch.lsap_solve_resid_out(plan.dims, plan.ws_offs, plan.out_offs, plan.workspace,
                                           row_ind, col_ind, status, bmin8, tplan.bmin8_offs, bm32,
                                           tplan.bm32_offs, tplan.segs, tplan.workspace, tplan.max_n,
                                           plan.long_min, plan.long_max, plan.short_max,
                                           _opts_list(options))
    return row_ind[:plan.n_out], col_ind[:plan.n_out], status


def pack_detections(boxes: Tensor, conf: Tensor, cls: Tensor, img_offs: Tensor,
                    conf_thresh: float, class_id: float = 0.0):
    """PoseEstimator._detect's box filtering + centres for a batch of images, on device.

    ``boxes`` f32 [n, 4] xyxy, ``conf``/``cls`` f32 [n] of all images
    concatenated, image k owning rows ``img_offs[k]:img_offs[k+1]`` (int64
    device tensor).  The threshold is rounded to float32 first, as numpy does
    when comparing a float32 array with a Python float (process_pose.py:130).
    -> (pts f64 [n, 2], cam_offs i64 [n_img+1], boxes_int i32 [n, 4],
    counts i32 [n_img], status i32 [1]) — rows past ``cam_offs[-1]`` are
    unused capacity; the matcher reads only the rows the offsets name.
    """
    dev = boxes.device
    n = int(boxes.shape[0])
    n_img = int(img_offs.numel()) - 1
    counts = torch.empty(max(n_img, 0), dtype=torch.int32, device=dev)
    cam_offs = torch.zeros(max(n_img, 0) + 1, dtype=torch.int64, device=dev)
    pts = torch.empty((n, 2), dtype=torch.float64, device=dev)
    boxes_out = torch.empty((n, 4), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    thresh = float(np.float32(conf_thresh))
    torch.ops.mvmatch.pack_detections_out(boxes.contiguous(), conf.contiguous(), cls.contiguous(),
                                          img_offs, thresh, float(np.float32(class_id)), counts,
                                          cam_offs, pts, boxes_out, status)
    return pts, cam_offs, boxes_out, counts, status


def triangulate_dlt(proj: Tensor, pts2d: Tensor, set_of_point: Optional[Tensor] = None) -> Tensor:
    """triangulate_multi_view for every point at once -> X f64 [n_points, 3] (device)."""
    X = torch.empty((int(pts2d.shape[0]), 3), dtype=torch.float64, device=pts2d.device)
    torch.ops.mvmatch.triangulate_dlt_out(proj.contiguous(), set_of_point, pts2d.contiguous(), X)
    return X


def _select_outputs(row_ind: Tensor, lsap_offs: Tensor, dev: torch.device):
    """(match i32 [cap, 3], cost f32 [cap], X f64 [cap, 3], count i32 [S]) for
    the select kernels to write: one row per assigned pair."""
    cap = int(row_ind.numel())
    return (torch.empty((cap, 3), dtype=i32, device=dev), torch.empty(cap, dtype=f32, device=dev),
            torch.empty((cap, 3), dtype=f64, device=dev),
            torch.empty(int(lsap_offs.numel()) - 1, dtype=i32, device=dev))


def select_triangulate(cube: Tensor, cube_offs: Tensor, cam_offs: Tensor, lsap_offs: Tensor,
                       row_ind: Tensor, col_ind: Tensor, pts: Tensor, proj: Tensor,
                       threshold: float):
    """Filter + stable cost sort + DLT of every scene's assignment (device).
    -> (match i32 [cap, 3], cost f32 [cap], X f64 [cap, 3], count i32 [S]); scene
    s's matches are rows ``lsap_offs[s] : lsap_offs[s] + count[s]``."""
    outs = _select_outputs(row_ind, lsap_offs, cube.device)
    torch.ops.mvmatch.select_triangulate_out(cube, cube_offs, cam_offs, lsap_offs, row_ind,
                                             col_ind, pts, proj.contiguous(), float(threshold), *outs)
    return outs


def select_triangulate_resid(tplan: TripletPlan, cam_offs: Tensor, lsap_offs: Tensor,
                             row_ind: Tensor, col_ind: Tensor, pts: Tensor, proj: Tensor,
                             threshold: float):
    """select_triangulate for a ``triplet_minima(..., tplan)`` batch: each
    assigned entry recomputed from the residuals in ``tplan.workspace``."""
    outs = _select_outputs(row_ind, lsap_offs, pts.device)
    torch.ops.mvmatch.select_triangulate_resid_out(tplan.workspace, tplan.max_n, cam_offs, lsap_offs,
                                                   row_ind, col_ind, pts, proj.contiguous(),
                                                   float(threshold), *outs)
    return outs


def _h2d_rig(Ks: np.ndarray, RTs: np.ndarray, device: torch.device) -> Tuple[Tensor, Tensor]:
    """Host K (f32) and RT (f64) -> device tensors with ONE copy, as
    ``_h2d_int64``: both in a pinned byte buffer (RT first: 8-byte aligned),
    copied without blocking."""
    rt = np.ascontiguousarray(RTs, dtype=np.float64)
    k = np.ascontiguousarray(Ks, dtype=np.float32)
    if rt.size == 0 or k.size == 0:      # nothing to stage (an empty batch)
        return torch.from_numpy(k).to(device), torch.from_numpy(rt).to(device)
    host =torch.from_numpy(np.concatenate([rt.reshape(-1).view(np.uint8), k.reshape(-1).view(np.uint8)]))
    if device.type == "cuda":
        dev = host.pin_memory().to(device, non_blocking=True)
    else:
        dev = host.to(device)
    return (dev[rt.nbytes:].view(torch.float32).view(k.shape),
            dev[:rt.nbytes].view(torch.float64).view(rt.shape))


def rig_matrices(Ks, RTs, pairs=None, *, want_proj: bool = True,
                 device: Optional[torch.device] = None):
    """compute_fundamental_matrix for every (capture, pair) and P = K @ RT[:3]
    for every (capture, camera), on the device (mvm_rig_matrices).

    ``Ks`` float32 [S, C, 3, 3], ``RTs`` float64 [S, C, 4, 4]: numpy arrays
    (uploaded in one pinned non-blocking copy, to ``device`` or the tensor
    input's device or the current GPU) or device tensors.  ``pairs``
    [P, 2]: default ``camera_pairs(C)``.
    -> (F f64 [S*P, 9], proj f64 [S, C, 3, 4] or None, status i32 [S]), all on
    the device.  status[s] = 1: some K of capture s is not of the pinhole form
    (include/mvmatch.h) and its F / proj rows are NOT written."""
    tensors = [x for x in (Ks, RTs) if isinstance(x, Tensor)]
    if device is None:
        device = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("rig_matrices needs a GPU device (the rig kernel has no CPU path)")
    for x, name, dt in ((Ks, "K", np.float32), (RTs, "RT", np.float64)):
        if not isinstance(x, Tensor) and np.asarray(x).dtype != dt:
            raise ValueError(f"{name}: expected {np.dtype(dt)}, got {np.asarray(x).dtype}")
    if not tensors:
        K, RT = _h2d_rig(np.asarray(Ks), np.asarray(RTs), device)
    else:       # one of them already on the device: the other goes up on its own
        K, RT = (x if isinstance(x, Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(device)
                 for x in (Ks, RTs))
    if K.dim() != 4 or tuple(K.shape[2:]) != (3, 3):
        raise ValueError(f"K: expected [S, C, 3, 3], got {tuple(K.shape)}")
    S, C = int(K.shape[0]), int(K.shape[1])
    if pairs is None:
        pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]    # camera_pairs(C)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_pairs = int(pairs.shape[0])
    F = torch.empty((S * n_pairs, 9), dtype=torch.float64, device=device)
    proj = torch.empty((S, C, 3, 4) if want_proj else (0,), dtype=torch.float64, device=device)
    status = torch.empty(S, dtype=torch.int32, device=device)
    torch.ops.mvmatch.rig_matrices_out(K, RT, [int(a) for a in pairs[:, 0]],
                                       [int(b) for b in pairs[:, 1]], F, proj, status)
    return F, (proj if want_proj else None), status


def compact_matches(match: Tensor, cost: Tensor, X: Tensor, count: Tensor, seg_offs: Tensor,
                    pts: Tensor, boxes: Tensor, cam_offs: Tensor, scene_base: int = 0):
    """The dense match table of a select_triangulate(_resid) result (device):
    scene s's ``count[s]`` matches, found at rows ``seg_offs[s]`` of match /
    cost / X, copied to rows ``dense_offs[s]`` with their boxes and centroids
    gathered from the packer's ``boxes`` / ``pts`` (CSR ``cam_offs``).
    -> (dense_offs i64 [S+1], scene i32 [cap], match i32 [cap, 3], cost f32 [cap],
    X f64 [cap, 3], boxes i32 [cap, 3, 4], centroids f64 [cap, 3, 2]); rows
    at and beyond ``dense_offs[S]`` (= count.sum()) are unused capacity."""
    dev = match.device
    cap = int(match.shape[0])
    n_scenes = int(count.numel())
    dense_offs = torch.zeros(n_scenes + 1, dtype=torch.int64, device=dev)
    rows = max(cap, 1)
    scene = torch.empty(rows, dtype=torch.int32, device=dev)
    match_out = torch.empty((rows, 3), dtype=torch.int32, device=dev)
    cost_out = torch.empty(rows, dtype=torch.float32, device=dev)
    X_out = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    boxes_out = torch.empty((rows, 3, 4), dtype=torch.int32, device=dev)
    cent_out = torch.empty((rows, 3, 2), dtype=torch.float64, device=dev)
    # no row to copy (no capacity, or no detection a match could name): every
    # count is 0 and the offsets stay 0; nothing is launched
    if n_scenes and cap and pts.numel():
        torch.ops.mvmatch.compact_matches_out(match, cost, X, count, seg_offs, pts, boxes, cam_offs,
                                              int(scene_base), dense_offs, scene, match_out, cost_out,
                                              X_out, boxes_out, cent_out)
    return (dense_offs, scene[:cap], match_out[:cap], cost_out[:cap], X_out[:cap], boxes_out[:cap],
            cent_out[:cap])


def compact_matches_views(views: Tensor, cost: Tensor, ext_cost: Optional[Tensor], X: Tensor,
                          count: Tensor, seg_offs: Tensor, pts: Tensor, boxes: Tensor, cam_offs: Tensor,
                          proj: Tensor, scene_base: int = 0):
    """The dense match table of a C-camera result with its reprojection
    residuals (device; mvm_compact_matches_views): ``compact_matches`` over the
    C view slots of ``views`` int32 [cap, C] (a three-camera result: its
    ``match``; ``ext_cost`` f32 [cap, C-3], None for C == 3), ``proj`` f64
    [S, C, 3, 4].  A slot of -1 gets a box of -1 and NaN centroid / residual.
    -> (dense_offs i64 [S+1], scene i32 [cap], views i32 [cap, C], n_views i32
    [cap], cost f32 [cap], ext_cost f32 [cap, C-3], X f64 [cap, 3], boxes i32
    [cap, C, 4], centroids f64 [cap, C, 2], reproj f64 [cap, C]); rows at and
    beyond ``dense_offs[S]`` (= count.sum()) are unused capacity."""
    dev = views.device
    cap, C = int(views.shape[0]), int(views.shape[1])
    n_scenes = int(count.numel())
    if ext_cost is None:
        ext_cost = torch.empty((cap, C - 3), dtype=torch.float32, device=dev)
    dense_offs = torch.zeros(n_scenes + 1, dtype=torch.int64, device=dev)
    rows = max(cap, 1)
    e = lambda shape, dt: torch.empty((rows,) + shape, dtype=dt, device=dev)
    outs = (e((), torch.int32), e((C,), torch.int32), e((), torch.int32), e((), torch.float32),
            e((C - 3,), torch.float32), e((3,), torch.float64), e((C, 4), torch.int32),
            e((C, 2), torch.float64), e((C,), torch.float64))
    # no row to copy: every count is 0 and the offsets stay 0; nothing is launched
    if n_scenes and cap and pts.numel():
        torch.ops.mvmatch.compact_matches_views_out(views, cost, ext_cost, X, count, seg_offs, pts, boxes,
                                                    cam_offs, proj.contiguous(), int(scene_base),
                                                    dense_offs, *outs)
    return (dense_offs,) + tuple(o[:cap] for o in outs)


def extend_costs(pts: Tensor, cam_offs: Tensor, F_ext: Tensor, match: Tensor, match_offs: Tensor,
                 count: Tensor, ext_offs: Tensor, n_cams: int, max_rows: int, *,
                 size: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """The cost of extending each three-view match into each detection of the
    extra cameras 3 .. n_cams-1 (mvm_extend_costs): for capture
    s and camera d the float32 matrix ``E_d [count[s], n_d]`` at
    ``ext_offs[s * (n_cams - 3) + d - 3]`` of the result, a cube entry whose
    anchors are the match's own detections.  ``pts`` / ``cam_offs`` the
    n_cams-camera CSR, ``F_ext`` f64 [S, n_cams-3, 3, 9] (F_0d, F_1d, F_2d per
    extra camera), ``match`` int32 [cap, 3] / ``match_offs`` int64 [S+1] /
    ``count`` int32 [S] as select_triangulate left them, ``max_rows`` a host
    bound on ``count``.  ``size`` = ``ext_offs[-1]`` when the caller knows it
    on the host (otherwise it is read back: one sync); ``out``: the float32
    buffer to write.  Entries outside the matrices are not written."""
    if out is None:
        if size is None:
            size = int(ext_offs[-1].item())
        out = torch.empty(max(int(size), 1), dtype=torch.float32, device=pts.device)
    torch.ops.mvmatch.extend_costs_out(pts, cam_offs, F_ext, match, match_offs, count, ext_offs,
                                       int(n_cams), int(max_rows), out)
    return out


def extend_select_triangulate(E: Tensor, ext_offs: Tensor, lsap_offs: Tensor, row_ind: Tensor,
                              col_ind: Tensor, match: Tensor, match_offs: Tensor, count: Tensor,
                              pts: Tensor, cam_offs: Tensor, proj: Tensor, threshold: float,
                              X: Tensor, n_cams: int, *,
                              out: Optional[Tuple[Tensor, Tensor]] = None):
    """The tail of the extension (mvm_extend_select_triangulate): the
    assignment (``row_ind`` / ``col_ind`` under ``lsap_offs``) of every
    ``extend_costs`` matrix, kept where ``E < threshold``.
    -> (views int32 [cap, n_cams] = (i, j, k, kept index or -1 ...),
    ext_cost f32 [cap, n_cams-3] = the kept E or +inf, X): ``X`` f64 [cap, 3]
    is updated in place -- matches that kept an extra view are triangulated
    over all their views, the others keep their value.  ``out`` = (views,
    ext_cost) to write into; rows outside the captures' matches keep their
    values."""
    dev = match.device
    cap = int(match.shape[0])
    if out is None:
        views = torch.empty((cap, n_cams), dtype=torch.int32, device=dev)
        ext_cost = torch.empty((cap, n_cams - 3), dtype=torch.float32, device=dev)
    else:
        views, ext_cost = out
    torch.ops.mvmatch.extend_select_triangulate_out(E, ext_offs, lsap_offs, row_ind, col_ind, match,
                                                    match_offs, count, pts, cam_offs, proj.contiguous(),
                                                    float(threshold), views, ext_cost, X)
    return views, ext_cost, X
