"""The view-pruning op over the C ABI (``torch.ops.mvmatch_views.*``).

``bpc_baseline_amd.ops`` keeps its frozen op surface (``mvmatch::*_out``); the
op that acts on the views of a C-camera batch after the fact registers here,
under a namespace of its own, with the same boundary layer: spec rows checked
by ``ops._check_args``, the C entry point through ``ops._call``, and the shared
fake that returns None.

  mvmatch_views::prune_views_out   mvm_prune_views_triangulate
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor

from . import _native, ops
from .ops import ANY, AT_LEAST, EXACT, f32, f64, i32, i64

__all__ = ["prune_views"]


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
