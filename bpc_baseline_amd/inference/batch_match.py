"""Batched, device-resident matching of many 3-camera captures.

The reference processes one capture at a time through host Python:
``PoseEstimator._detect`` packs YOLO boxes into dicts (process_pose.py:116-142),
``_match`` builds F12/F13/F23, the cost cube, the assignment, the threshold
filter and the cost sort (:144-183), and ``PosePrediction`` triangulates each
match (:79-94).  ``match_captures`` runs the same steps for S captures at once
with every O(n) and larger step on the GPU:

  1. mvm_pack_detections      boxes/conf/cls -> half-integer centroids (CSR)
  2. host                     F (batched, bit-equal to compute_fundamental_matrix)
                              and P = K @ RT[:3]; O(1) per capture
     or mvm_rig_matrices      (rig="device") the same on the device, one launch
  3. mvm_triplet_cost_argmin  the (N, M, P) cube of every capture (+ its 8-row
                              minima when an assignment is large: _bmin8)
  4. mvm_lsap_solve           scipy-identical assignment of every flattened cube
  5. mvm_select_triangulate   cost < threshold, stable sort by cost, DLT

The only device->host transfer before the results is the per-image kept
count (n_img int32, with the packing status), which sizes the cube and
assignment layouts; the results need one more (statuses + match counts).

Results equal, capture by capture, the reference's ``_match`` outputs fed with
``_detect``'s detections: match indices and order exactly, ``t`` to rounding
(tests/test_batch_match_gpu.py).
"""
from __future__ import annotations

import threading
import weakref
from dataclasses import dataclass
from typing import Iterable, Iterator, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import ops, ops_views
from .utils.camera_utils import (fundamental_matrices_batched, pinhole_intrinsics, projection_matrices,
                                 rig_matrices)

__all__ = ["MatchBatch", "MatchTable", "extension_pairs", "match_capture_stream", "match_captures",
           "projection_matrices", "rig_matrices", "rig_worker_pool"]


def _check_n_cams(n_cams) -> int:
    if not 3 <= int(n_cams) <= 8:
        raise ValueError(f"n_cams: expected 3..8, got {n_cams}")
    return int(n_cams)


def _check_rig(rig: str) -> None:
    if rig not in ("host", "device", "auto"):
        raise ValueError(f"rig: expected 'host', 'device' or 'auto', got {rig!r}")


def _raise_failed(bad) -> None:
    """``bad``: per capture, nonzero where an assignment's status was."""
    raise ValueError(f"assignment failed for captures {np.nonzero(bad)[0][:8].tolist()} "
                     "(cost matrix contains invalid numeric entries or is infeasible)")


def extension_pairs(n_cams: int) -> np.ndarray:
    """The camera pairs whose F ``match_captures(n_cams=C)`` uses, in its
    order -> int32 [3 + 3 (C - 3), 2]: (0,1), (0,2), (1,2) of the three-camera
    chain, then per extra camera d = 3 .. C-1 its pairs with the three anchor
    cameras (0,d), (1,d), (2,d)."""
    C = _check_n_cams(n_cams)
    out = [(0, 1), (0, 2), (1, 2)] + [(c, d) for d in range(3, C) for c in range(3)]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


class _Rig(NamedTuple):
    """The packed detections and camera matrices of a batch of S captures of
    C cameras, as the device chain reads them."""
    pts: torch.Tensor            # float64 [n, 2]
    cam_offs: torch.Tensor       # int64 [C S + 1]  CSR of pts (device)
    cam_offs_host: np.ndarray    # the same on the host
    counts: np.ndarray           # int64 [S, C]     detections per view
    F: torch.Tensor              # float64, flat: 3 + 3 (C - 3) matrices per capture
    proj: torch.Tensor           # float64 [S, C, 3, 4]


class _Chain(NamedTuple):
    """What the three-camera chain leaves on the device (scene s owns rows
    ``offs_host[s] : offs_host[s] + count[s]`` of match / cost / X)."""
    match: torch.Tensor          # int32 [cap, 3]
    cost: torch.Tensor           # float32 [cap]
    X: torch.Tensor              # float64 [cap, 3]
    status: torch.Tensor         # int32 [S]        the assignment's, 0 = solved
    count: torch.Tensor          # int32 [S]
    offs_host: np.ndarray        # int64 [S + 1]
    cube: Optional[torch.Tensor]
    offs_dev: torch.Tensor       # offs_host on the device


def _host_rig(Ks: np.ndarray, RTs: np.ndarray, n_cams: int):
    """F and P of every capture on the host: ``rig_matrices`` for three
    cameras, the same batched functions over ``extension_pairs`` above."""
    if n_cams == 3:
        return rig_matrices(Ks, RTs)
    return (fundamental_matrices_batched(Ks, RTs, extension_pairs(n_cams)),
            projection_matrices(Ks, RTs))


@dataclass
class MatchBatch:
    """Device results of ``match_captures`` (scene s owns rows
    ``offs[s] : offs[s] + count[s]`` of match / cost / X)."""
    match: torch.Tensor          # int32 [cap, 3]   (i, j, k) per match
    cost: torch.Tensor           # float32 [cap]    cube value of the match
    X: torch.Tensor              # float64 [cap, 3] triangulated centre
    count: np.ndarray            # int32 [S]
    offs: np.ndarray             # int64 [S + 1]
    pts: torch.Tensor            # float64 [n, 2]   packed centroids
    boxes: torch.Tensor          # int32 [n, 4]     packed int boxes
    cam_offs: np.ndarray         # int64 [C S + 1]  CSR of pts / boxes (C = n_cams views per capture)
    cube: Optional[torch.Tensor] = None
    # what ``table`` hands the compaction kernel, kept on the device by
    # match_captures (a batch built without them uploads the host copies)
    offs_dev: Optional[torch.Tensor] = None       # int64 [S + 1]
    count_dev: Optional[torch.Tensor] = None      # int32 [S]
    cam_offs_dev: Optional[torch.Tensor] = None   # int64 [C S + 1]
    # a rig of n_cams > 3 cameras (match_captures(n_cams=C)):
    # the match's detection in every view, -1 where an extra view has none
    # (views[:, :3] == match), and the extension cost of the kept ones (+inf
    # where none)
    views: Optional[torch.Tensor] = None          # int32 [cap, C]
    ext_cost: Optional[torch.Tensor] = None       # float32 [cap, C - 3]
    n_cams: int = 3
    # the projection matrices X was triangulated with, all C cameras (what
    # the table's reprojection residuals are measured against)
    proj: Optional[torch.Tensor] = None           # float64 [S, C, 3, 4]
    # match_captures(reproj_gate=G): bit d set where the extra
    # view of camera d was dropped for its reprojection residual (0 in every
    # row of a three-camera batch); None without a gate
    pruned: Optional[torch.Tensor] = None         # int32 [cap]
    # match_captures(extra_seeds=[...]): the results of the
    # extra seed passes hang off the first pass's batch, in order.  Each is a
    # batch of its own over the detections the passes before it left, with the
    # cameras in ``cam_order`` (view slot q is original camera cam_order[q]; the
    # seed triple first) and ``orig`` naming each of its detections' index in
    # its original view.  Both are None on the first pass's batch, whose
    # fields the extra passes never touch.
    cam_order: Optional[tuple] = None
    orig: Optional[torch.Tensor] = None           # int32 [n]
    passes: tuple = ()
    # match_captures(refine=...): X then holds the points
    # refined by reprojection error and these the DLT points they started
    # from, sqrt(cost / views) before and after in pixels, (status,
    # evaluations) and the upper triangle of the inverse normal matrix at X
    # (mm^2 / px^2; times the pixel variance: the covariance).  All None
    # without the keyword
    X_dlt: Optional[torch.Tensor] = None          # float64 [cap, 3]
    refine_rms: Optional[torch.Tensor] = None     # float64 [cap, 2]
    refine_info: Optional[torch.Tensor] = None    # int32 [cap, 2]
    cov: Optional[torch.Tensor] = None            # float64 [cap, 6]

    def host(self) -> dict:
        """One D2H copy of everything ``predictions`` reads (and ``pruned``
        and the refinement's fields when the batch has them)."""
        if not hasattr(self, "_host"):
            keys = ("match", "cost", "X", "pts", "boxes") + (("views",) if self.n_cams > 3 else ())
            keys += ("pruned",) if self.pruned is not None else ()
            keys += tuple(k for k in ("X_dlt", "refine_rms", "refine_info", "cov") if getattr(self, k) is not None)
            self._host = {k: getattr(self, k).cpu().numpy() for k in keys}
        return self._host

    def predictions(self, s: int) -> List[tuple]:
        """Scene s as the reference's PosePrediction fields, in _match's order:
        list of (boxes int32 [3, 4], centroids f64 [3, 2], t f64 [3]).  A
        batch of n_cams > 3: per match its V views, (boxes [V, 4], centroids
        [V, 2], t, cams int64 [V]) with cams ascending."""
        o, n = int(self.offs[s]), int(self.count[s])
        h = self.host()
        C = self.n_cams
        if C > 3:
            out = []
            for q in range(n):
                v = h["views"][o + q].astype(np.int64)
                cams = np.nonzero(v >= 0)[0]
                rows = self.cam_offs[C * s + cams] + v[cams]
                out.append((h["boxes"][rows], h["pts"][rows], h["X"][o + q], cams))
            return out
        rows = self.cam_offs[3 * s:3 * s + 3][None, :] + h["match"][o:o + n].astype(np.int64)
        return [(h["boxes"][rows[q]], h["pts"][rows[q]], h["X"][o + q]) for q in range(n)]

    def table(self, scene_base: int = 0, reproj: Optional[bool] = None) -> "MatchTable":
        """The batch as a dense ``MatchTable`` (mvm_compact_matches): the
        ``count.sum()`` matches in consecutive rows, each with its boxes and
        centroids, scene ids starting at ``scene_base``.  No host sync: the
        row count is ``count``, already on the host.

        ``reproj=True`` goes through mvm_compact_matches_views: rows over all
        C view slots (``views`` / ``n_views`` / ``ext_cost``) with ``reproj``,
        the reprojection residual of X in every kept view against ``proj``
        (DESIGN §3.12).  A three-camera table so made holds the six fields of
        the plain one bit for bit.  Needs the batch's ``proj``.  That is the
        only table a batch of n_cams > 3 has: the plain rows hold three
        views, so without ``reproj=True`` such a batch raises
        ``NotImplementedError`` as it always did."""
        C = self.n_cams
        with_views = bool(reproj)
        if C > 3 and not with_views:
            raise NotImplementedError("MatchTable rows without reproj hold three views; a batch of "
                                      f"n_cams={C} has its table as table(reproj=True)")
        if with_views and self.proj is None:
            raise ValueError("the reprojection residuals need the batch's proj (match_captures sets it)")
        S = int(self.count.size)
        offs = np.zeros(S + 1, np.int64)
        np.cumsum(self.count, out=offs[1:])
        n = int(offs[-1])
        dev = self.match.device
        if n == 0:
            return MatchTable.empty(dev, offs, n_cams=C, reproj=with_views)
        seg, cam, cnt = self.offs_dev, self.cam_offs_dev, self.count_dev
        if seg is None or cam is None:
            seg, cam = ops._h2d_int64([self.offs, self.cam_offs], dev)
        if cnt is None:
            cnt = torch.from_numpy(np.ascontiguousarray(self.count, np.int32)).to(dev)
        if with_views:
            views = self.views if C > 3 else self.match
            _, scene, views, n_views, cost, ext, X, boxes, cent, rep = ops.compact_matches_views(
                views, self.cost, self.ext_cost if C > 3 else None, self.X, cnt, seg, self.pts,
                self.boxes, cam, self.proj.reshape(S, C, 3, 4), scene_base)
            return MatchTable(scene=scene[:n], match=views[:n, :3], cost=cost[:n], X=X[:n],
                              boxes=boxes[:n], centroids=cent[:n], offs=offs, views=views[:n],
                              n_views=n_views[:n], ext_cost=ext[:n], reproj=rep[:n], n_cams=C)
        _, scene, match, cost, X, boxes, cent = ops.compact_matches(
            self.match, self.cost, self.X, cnt, seg, self.pts, self.boxes, cam, scene_base)
        return MatchTable(scene=scene[:n], match=match[:n], cost=cost[:n], X=X[:n], boxes=boxes[:n],
                          centroids=cent[:n], offs=offs)

    def _table_in_original_order(self) -> "MatchTable":
        """``table(reproj=True)`` of an extra pass with its per-camera columns
        back in original camera order and its views naming original
        detections (torch indexing on the device; no host sync)."""
        tab = self.table(reproj=True)
        if self.cam_order is None:
            return tab
        C, dev = self.n_cams, self.match.device
        inv = np.argsort(np.asarray(self.cam_order, np.int64))       # inv[cam_order[q]] = q
        inv_dev, seed_dev = ops._h2d_int64([inv, np.asarray(self.cam_order[:3], np.int64)], dev)
        views = tab.views
        if int(views.shape[0]):
            cam = self.cam_offs_dev
            if cam is None:
                cam, = ops._h2d_int64([self.cam_offs], dev)
            slot = tab.scene.to(torch.int64)[:, None] * C + torch.arange(C, device=dev)[None, :]
            rows = cam[slot] + views.clamp(min=0).to(torch.int64)
            # a slot with no detection (-1) stays as it is
            views = torch.where(views >= 0, self.orig[rows.clamp(max=max(int(self.orig.numel()) - 1, 0))],
                                views)
        views = views.index_select(1, inv_dev)
        return MatchTable(scene=tab.scene, match=views.index_select(1, seed_dev), cost=tab.cost, X=tab.X,
                          boxes=tab.boxes.index_select(1, inv_dev),
                          centroids=tab.centroids.index_select(1, inv_dev), offs=tab.offs, views=views,
                          n_views=tab.n_views, ext_cost=tab.ext_cost,
                          reproj=tab.reproj.index_select(1, inv_dev), n_cams=C)

    def table_all(self, scene_base: int = 0) -> "MatchTable":
        """The matches of every pass as one ``MatchTable`` in original camera
        order (``match_captures(extra_seeds=...)``): per
        capture the first pass's rows, then the second's, and so on, each
        pass in its own order.  Every pass's ``table(reproj=True)`` is built
        on the device; the per-camera columns (``boxes``, ``centroids``,
        ``views``, ``reproj``) of an extra pass are put back in original
        camera order and its ``views`` go through its ``orig``, so they name
        the detections of the first pass's ``pts`` / ``boxes``.  ``ext_cost``
        stays in the slot order of its pass (column e belongs to camera
        ``cam_order[3 + e]``).  ``seed_pass`` int32 [n] holds the pass index;
        ``match`` of a row with ``seed_pass > 0`` holds the detections of the
        pass's seed triple (original indices, the triple's order), so
        ``views[:, :3] == match`` holds only where ``seed_pass == 0``.  No
        host sync.  A batch without extra passes gives ``table(reproj=True)``
        with ``seed_pass`` all zero."""
        tabs = [b._table_in_original_order() for b in (self,) + tuple(self.passes)]
        dev = self.match.device
        counts = np.stack([np.diff(np.asarray(t.offs, np.int64)) for t in tabs])      # [passes, S]
        base = np.concatenate([[0], np.cumsum(counts.sum(axis=1))[:-1]])
        offs = np.zeros(counts.shape[1] + 1, np.int64)
        np.cumsum(counts.sum(axis=0), out=offs[1:])
        # row r of the merged table: capture by capture, pass by pass
        src = [np.arange(base[p] + t.offs[s], base[p] + t.offs[s + 1])
               for s in range(counts.shape[1]) for p, t in enumerate(tabs)]
        src = np.concatenate(src).astype(np.int64) if src else np.zeros(0, np.int64)
        which = np.repeat(np.arange(len(tabs)), counts.sum(axis=1))[src] if src.size else np.zeros(0, np.int64)
        if src.size:
            src_dev, which_dev = ops._h2d_int64([src, which], dev)
        else:
            src_dev = which_dev = torch.zeros(0, dtype=torch.int64, device=dev)
        take = lambda k: torch.cat([getattr(t, k) for t in tabs]).index_select(0, src_dev)
        out = {k: take(k) for k in MatchTable.FIELDS + MatchTable.VIEW_FIELDS}
        out["scene"] = out["scene"] + int(scene_base)
        return MatchTable(offs=offs, n_cams=self.n_cams, seed_pass=which_dev.to(torch.int32), **out)


@dataclass
class MatchTable:
    """Matches of a batch as dense, self-contained rows (capture s owns rows
    ``offs[s] : offs[s + 1]``, in _match's order): what ``MatchBatch`` holds
    without its unused rows and with every index resolved, so a table can be
    copied to the host in one piece or gathered from another rank
    (``distributed.gather_tables``)."""
    scene: torch.Tensor          # int32 [n]        capture id of the row
    match: torch.Tensor          # int32 [n, 3]     (i, j, k)
    cost: torch.Tensor           # float32 [n]
    X: torch.Tensor              # float64 [n, 3]   triangulated centre (PosePrediction.t)
    boxes: torch.Tensor          # int32 [n, C, 4]  the views' boxes (C = n_cams)
    centroids: torch.Tensor      # float64 [n, C, 2]
    offs: np.ndarray             # int64 [S + 1]    host
    # a table made by mvm_compact_matches_views (a batch of n_cams > 3, or
    # table(reproj=True)): the detection of every view slot, -1 where an extra
    # view has none (its box is then -1, its centroid and residual NaN;
    # match == views[:, :3]), and the reprojection residual of X per view
    views: Optional[torch.Tensor] = None      # int32 [n, C]
    n_views: Optional[torch.Tensor] = None    # int32 [n]        views >= 0 per row
    ext_cost: Optional[torch.Tensor] = None   # float32 [n, C - 3]
    reproj: Optional[torch.Tensor] = None     # float64 [n, C]   pixels
    n_cams: int = 3
    # a table made by MatchBatch.table_all: the seed pass the row came from
    # (0: cameras 0-2).  Where it is > 0, ``match`` holds the detections of
    # that pass's seed triple, not views[:, :3], and ext_cost is in the slot
    # order of that pass
    seed_pass: Optional[torch.Tensor] = None  # int32 [n]

    FIELDS = ("scene", "match", "cost", "X", "boxes", "centroids")
    VIEW_FIELDS = ("views", "n_views", "ext_cost", "reproj")

    def fields(self) -> tuple:
        """The names of the row fields this table holds: ``FIELDS``, then
        those of ``VIEW_FIELDS`` that are set, then ``seed_pass`` if set."""
        return (self.FIELDS + tuple(k for k in self.VIEW_FIELDS if getattr(self, k) is not None)
                + (("seed_pass",) if self.seed_pass is not None else ()))

    @classmethod
    def empty(cls, device, offs: Optional[np.ndarray] = None, n_cams: int = 3,
              reproj: bool = False) -> "MatchTable":
        """A table of no rows (``offs``: all zero, one entry per capture + 1;
        default no captures), of the shapes ``MatchBatch.table(reproj=reproj)``
        gives a batch of ``n_cams`` cameras."""
        C = int(n_cams)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        extra = {}
        if C > 3 or reproj:
            extra = dict(views=e((0, C), torch.int32), n_views=e(0, torch.int32),
                         ext_cost=e((0, C - 3), torch.float32), reproj=e((0, C), torch.float64))
        return cls(scene=e(0, torch.int32), match=e((0, 3), torch.int32), cost=e(0, torch.float32),
                   X=e((0, 3), torch.float64), boxes=e((0, C, 4), torch.int32),
                   centroids=e((0, C, 2), torch.float64),
                   offs=np.zeros(1, np.int64) if offs is None else offs, n_cams=C, **extra)

    def host(self) -> dict:
        """One D2H copy of the n rows."""
        if not hasattr(self, "_host"):
            self._host = {k: getattr(self, k).cpu().numpy() for k in self.fields()}
        return self._host

    def predictions(self, s: int) -> List[tuple]:
        """Exactly ``MatchBatch.predictions(s)``: (boxes int32 [3, 4],
        centroids f64 [3, 2], t f64 [3]) per match of capture s; for
        n_cams > 3 (boxes [V, 4], centroids [V, 2], t, cams int64 [V]) over
        the row's V kept views, cams ascending."""
        h = self.host()
        rows = range(int(self.offs[s]), int(self.offs[s + 1]))
        if self.n_cams > 3:
            out = []
            for r in rows:
                cams = np.nonzero(h["views"][r] >= 0)[0]
                out.append((h["boxes"][r][cams], h["centroids"][r][cams], h["X"][r], cams))
            return out
        return [(h["boxes"][r], h["centroids"][r], h["X"][r]) for r in rows]

    def reprojection(self, s: int) -> List[np.ndarray]:
        """Per match of capture s, the reprojection residual (pixels, f64 [V])
        of its X in each view it kept, in the order of ``predictions(s)``'s
        cams.  Needs a table with ``reproj``."""
        if self.reproj is None:
            raise ValueError("this table holds no reprojection residuals (table(reproj=True))")
        h = self.host()
        return [h["reproj"][r][h["views"][r] >= 0]
                for r in range(int(self.offs[s]), int(self.offs[s + 1]))]

    def crops(self, images: torch.Tensor, rows=None, cams=None, **kw):
        """The pose head's input crops of the table's views
        (``ops_views.crop_views`` on the table's own ``scene`` / ``views`` /
        ``boxes``): ``images`` uint8 [S, n_cams, H, W, 3] (B, G,
        R) on the device, ``rows`` a (begin, end) pair (default all), ``cams``
        the cameras wanted (default all), the other keywords ``crop_views``'s
        (``size``, ``mean``, ``std``, ``fill``, ``dtype``, ``scene_base``: what
        the table's scene ids start at).  Works on the plain three-camera
        table, on the view table and on ``table_all()``, whose views and boxes
        are in original camera order.
        -> (crops [rows, cams, 3, size, size], geom int32 [rows, cams, 8]).
        One float32 crop of 256 x 256 is 786 KB, so a caller feeds its head
        in row ranges, not the whole table at once.  ``cams=(2,)`` is what
        the reference's ``final_rotation`` uses."""
        views = self.views if self.views is not None else self.match
        return ops_views.crop_views(images, self.scene, views, self.boxes, self.n_cams, rows=rows, cams=cams,
                                    **kw)

    def poses(self, raw: torch.Tensor, RTs, mode: str, rows=None, cams=None, syms=None, rounds: int = 2, **kw):
        """The poses of the table's rows from a rotation head's raw outputs
        (``ops_views.fuse_rotations`` on the table's own ``scene`` / ``views``
        / ``X``): ``raw`` float32 [rows, cams, D] on the device,
        what the head made of ``crops(images, rows=rows, cams=cams)``; ``RTs``
        f64 [S, n_cams, 4, 4] (host or device); ``mode`` "euler", "quat" or
        "6d"; ``rows`` and ``cams`` exactly as in ``crops``; the other keywords
        ``fuse_rotations``'s (``fuse``, ``cam``, ``scene_base``).  Works on the
        plain three-camera table, on the view table and on ``table_all()``.
        -> ``ops_views.FusedRotations``: ``pose`` f64 [rows, 4, 4] holds the
        fused rotation and the row's X (refined where the batch was), ``spread``
        each view's distance to it.
        With ``syms`` f64 [K, 4, 4] (the object's symmetries, as ``score``
        takes them) the mean is taken under them, in ``rounds`` rounds
        (``ops_views.fuse_rotations_sym``): every view is first
        moved by the symmetry that takes it nearest the others.  That is a
        mean: ``fuse`` is left out or "mean", and ``cam`` is a ValueError.
        Without ``syms`` there are no rounds: ``rounds`` is not read.
        -> ``ops_views.SymFusedRotations``."""
        views = self.views if self.views is not None else self.match
        if syms is not None:
            if kw.pop("fuse", "mean") != "mean":
                raise ValueError('syms: the mean under symmetries needs fuse="mean"')
            if "cam" in kw:
                raise ValueError('syms: the mean under symmetries takes every view; cam= goes with fuse="cam"')
            return ops_views.fuse_rotations_sym(raw, self.scene, views, self.X, RTs, self.n_cams, mode, syms,
                                                rows=rows, cams=cams, rounds=rounds, **kw)
        return ops_views.fuse_rotations(raw, self.scene, views, self.X, RTs, self.n_cams, mode, rows=rows,
                                        cams=cams, **kw)

    def fit_boxes(self, pose: torch.Tensor, verts, proj=None, Ks=None, RTs=None, rows=None, **kw):
        """Each pose's translation fitted to the table's boxes, given the
        model (``ops_views.fit_boxes`` on the table's own ``scene`` / ``views``
        / ``boxes``): ``pose`` f64 [rows, 4, 4] on the device,
        for example ``poses(...).pose``, whose translation is the table's X --
        the triangulation of box centres, which are not the projections of
        the object's origin; ``verts`` f64 [V, 3] the model's vertices as
        ``score`` takes them; ``rows`` exactly as in ``poses``.  The rig is
        ``proj`` f64 [S, n_cams, 3, 4] (host or device), or ``Ks`` [S, n_cams,
        3, 3] and ``RTs`` [S, n_cams, 4, 4], from which it is built as the
        host rig builds it (``projection_matrices``); giving both or neither
        is a ValueError.  The other keywords are ``fit_boxes``'s
        (``max_evals``, ``cov``, ``resid``, ``scene_base``).  Works on the
        plain three-camera table, on the view table and on ``table_all()``.
        -> ``ops_views.BoxFit``; its ``pose`` goes straight into
        ``score(pose=...)``."""
        if (proj is None) == (Ks is None and RTs is None):
            raise ValueError("the rig: give proj, or Ks and RTs, not both and not neither")
        if proj is None:
            if Ks is None or RTs is None:
                raise ValueError("the rig: Ks and RTs go together")
            proj = projection_matrices(np.asarray(Ks), np.asarray(RTs))
        views = self.views if self.views is not None else self.match
        return ops_views.fit_boxes(pose, self.scene, views, self.boxes, proj, self.n_cams, verts, rows=rows, **kw)

    def score(self, gt_pose, gt_offs, verts=None, syms=None, pose=None, thresholds=None, rows=None,
              scene_base: int = 0):
        """The table's rows against ground truth (``ops_views.score_poses`` on
        the table's own ``scene``): ``gt_pose`` f64 [G, 4, 4] the
        ground-truth poses in the world frame, ``gt_offs`` int64 [S + 1] each
        capture's rows among them (host or device).  With ``pose=None`` the
        estimates are identity rotations with the table's ``X`` and ``verts``
        defaults to the single origin: ``err`` is then the distance of the
        centres, which scores the matcher alone, with no head.  With
        ``pose=fused.pose`` (f64 [rows, 4, 4]) and ``rows`` as given to
        ``poses`` it scores full poses over ``verts`` f64 [V, 3] and ``syms``
        f64 [K, 4, 4] (default the identity).  ``thresholds`` (1..16 numbers):
        the rows are also matched greedily to the ground truth per capture
        (``ops_views.match_scores`` with the table's ``offs``); matching is per
        whole capture, so it needs ``rows=None``.  Works on the plain
        three-camera table, on the view table and on ``table_all()``.
        -> ``ops_views.PoseScores``, with ``gt_index`` / ``tp`` set where
        ``thresholds`` is given (``ops_views.recall_precision`` takes ``tp``)."""
        n = int(self.scene.shape[0])
        if thresholds is not None and rows is not None:
            raise ValueError("thresholds: matching is per whole capture and needs rows=None")
        if rows is None:
            rows = (0, n)
        try:
            begin, end = (int(r) for r in rows)
        except (TypeError, ValueError):
            raise ValueError(f"rows: expected a (begin, end) pair, got {rows!r}") from None
        if not 0 <= begin <= end <= n:
            raise ValueError(f"rows: expected 0 <= begin <= end <= {n}, got ({begin}, {end})")
        if pose is None:
            pose = torch.eye(4, dtype=torch.float64, device=self.X.device).repeat(end - begin, 1, 1)
            pose[:, :3, 3] = self.X[begin:end]
            if verts is None:
                verts = np.zeros((1, 3))
        elif verts is None:
            raise ValueError("verts: a full pose is scored over the model's vertices")
        if pose.dim() != 3 or tuple(pose.shape) != (end - begin, 4, 4):
            raise ValueError(f"pose must be [{end - begin}, 4, 4], got {tuple(pose.shape)}")
        res = ops_views.score_poses(pose, self.scene[begin:end], gt_pose, gt_offs, verts, syms,
                                    scene_base=scene_base)
        if thresholds is not None:
            res.gt_index, res.tp = ops_views.match_scores(res.err, self.offs, gt_offs, thresholds)
        return res


def match_captures(boxes: torch.Tensor, conf: torch.Tensor, cls: torch.Tensor,
                   img_offs: torch.Tensor, Ks: np.ndarray, RTs: np.ndarray, *,
                   conf_thresh: float = 0.1, matching_threshold: float = 30,
                   keep_cube: bool = False, timings: Optional[dict] = None,
                   F: Optional[torch.Tensor] = None,
                   proj: Optional[torch.Tensor] = None, rig: str = "host",
                   n_cams: int = 3, reproj_gate: Optional[float] = None,
                   extra_seeds: Optional[Sequence] = None, refine=None) -> MatchBatch:
    """Detect-packing + matching + triangulation of S 3-camera captures.

    ``boxes`` f32 [n, 4] xyxy, ``conf``/``cls`` f32 [n]: the detector outputs
    of the 3S images (capture s, camera c = image 3s + c) concatenated on the
    device; ``img_offs`` int64 [3S + 1] device.  ``Ks`` float32 [S, 3, 3, 3],
    ``RTs`` float64 [S, 3, 4, 4] (host).  Defaults are PoseEstimatorParams'
    (process_pose.py:36-37).

    ``F`` (f64 [S*3, 9], F12/F13/F23 per capture) and ``proj`` (f64 [S, 3, 3, 4])
    may be passed as device tensors when the rigs repeat across batches (a
    static camera rig): they are then not recomputed on the host.  They must
    be what ``fundamental_matrices_batched`` / ``projection_matrices`` return.

    ``rig`` says where F and proj are computed when they are not passed:
    ``"host"`` (the default) by ``rig_matrices`` in numpy; ``"device"`` by
    ``ops.rig_matrices`` (mvm_rig_matrices: no per-capture host work; F and proj
    bit-equal to the host's where numpy's BLAS uses FMA kernels, F within a
    few 1e-14 relative elsewhere),
    with ``Ks`` / ``RTs`` as host arrays or device tensors; ``"auto"``
    ``"device"`` when every K has the pinhole form the kernel inverts
    (``pinhole_intrinsics``; device tensors are not inspected and go to the
    device), else ``"host"``.  Under ``"device"`` a capture with another K is
    computed on the host when ``Ks`` / ``RTs`` are host arrays, and raises
    ``ValueError`` when they are device tensors.  ``F`` / ``proj`` cannot be
    combined with ``rig="device"`` or ``"auto"``.

    ``n_cams`` = C, 3 <= C <= 8: captures of C cameras (``img_offs`` int64
    [C S + 1], ``Ks`` [S, C, 3, 3], ``RTs`` [S, C, 4, 4]; ``F`` f64
    [S (3 + 3 (C - 3)), 9] in the order of ``extension_pairs(C)``, ``proj``
    [S, C, 3, 4]).  Cameras 0, 1, 2 are matched as above, unchanged; each
    extra camera d then assigns its detections to those matches by the cost
    of a cube entry anchored at the match's three detections (scipy's
    assignment, kept below ``matching_threshold``), and a match is
    triangulated over all the views it kept.  The result has
    ``views`` / ``ext_cost`` / ``n_cams`` set; matches, costs and order are
    those of the three cameras alone.

    The result keeps ``proj`` (device, [S, C, 3, 4], all C cameras), computed
    here or passed in: what ``MatchBatch.table`` measures the reprojection
    residuals against.

    ``reproj_gate`` = G pixels, 0 <= G <= +inf (None, the default: off,
    nothing launched): after the extension, every match drops the extra views
    whose reprojection residual is not <= G, the worst first and one at a
    time, and is triangulated again over the views left after each drop
    (``ops_views.prune_views``; on the device, no further
    device -> host copy).  A dropped view reads -1 in ``views`` and +inf in
    ``ext_cost``; the result's ``pruned`` holds bit d where camera d was
    dropped.  Cameras 0-2, the matches, their costs, order and counts never
    change.  With ``n_cams=3`` the gate is accepted and ``pruned`` is zeros.

    ``extra_seeds`` = [(a, b, c), ...], 1 to 4 triples of distinct cameras
    < C, needs C >= 4 (None, the default: nothing launched, today's result):
    an object that one of cameras 0-2 misses can never become a match above,
    so after that first pass each triple in turn runs the same C-camera path
    on the detections no earlier pass's match holds (read after that pass's
    gate: a pruned view is free again), with the cameras reordered so that
    (a, b, c) are matched as the cube's N, M, P axes and the others extend
    them.  The sub-batch is built on the device
    (``ops_views.mark_used`` / ``leftover_counts`` / ``leftover_gather``); a
    pass adds one device -> host copy, of its leftover counts, to those of
    the path it runs.  The passes' results are ``MatchBatch.passes``, each a
    batch of its own with ``cam_order`` / ``orig``; the first pass's fields
    are byte for byte those of the call without the keyword, and
    ``MatchBatch.table_all()`` merges all passes into one table in original
    camera order.  ``ValueError`` for a bad triple or ``n_cams=3``;
    ``TypeError`` with ``F`` / ``proj``, since a pass needs the F and P of
    its own pair list.

    ``refine`` (None, the default: off, nothing launched, today's result;
    True: at most 10 evaluations; an int 1..64: that many): at the end of
    every pass -- behind the extension and the gate, so over the views the gate
    left --, every match's X is refined from its DLT point by minimising the
    summed squared reprojection error over its views (``n_cams=3``: the three
    of them), by damped Gauss-Newton steps that never raise it
    (``ops_views.refine_points``; on the device, no further
    device -> host copy).  ``X`` then holds the refined points, so tables and
    ``predictions`` carry them; ``X_dlt`` the DLT points, ``refine_rms`` the
    rms reprojection error before and after, ``refine_info`` (status,
    evaluations) and ``cov`` the inverse normal matrix at X, whose product
    with the pixel variance is the point's covariance.  Every other field is
    byte for byte that of the call without the keyword.  ``ValueError`` for
    anything else.
    """
    C = _check_n_cams(n_cams)
    refine = _check_refine(refine)
    _check_rig(rig)
    gate = None if reproj_gate is None else ops_views._check_gate(reproj_gate)
    if rig != "host" and (F is not None or proj is not None):
        raise TypeError(f"F / proj cannot be passed with rig={rig!r}: that path computes them")
    seeds = _check_extra_seeds(extra_seeds, C)
    if seeds and (F is not None or proj is not None):
        raise TypeError("F / proj cannot be passed with extra_seeds: every pass computes those of its "
                        "own camera order")
    dev = boxes.device
    import time
    clock = [time.perf_counter()]

    def mark(name):                      # optional stage timings (synchronising)
        if timings is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            timings[name] = timings.get(name, 0.0) + now - clock[0]
            clock[0] = now

    n_img = int(img_offs.numel()) - 1
    if n_img % C:
        raise ValueError(f"img_offs must describe {C} images per capture")
    S = n_img // C
    n_pairs = 3 + 3 * (C - 3)
    on_device = isinstance(Ks, torch.Tensor) or isinstance(RTs, torch.Tensor)
    if rig == "host" or not on_device:
        Ks = np.asarray(Ks, dtype=np.float32).reshape(S, C, 3, 3)
        RTs = np.asarray(RTs, dtype=np.float64).reshape(S, C, 4, 4)
    else:
        Ks, RTs = Ks.reshape(S, C, 3, 3), RTs.reshape(S, C, 4, 4)
    if rig == "auto":
        rig = "device" if on_device or bool(pinhole_intrinsics(Ks).all()) else "host"

    pts, cam_offs, boxes_int, counts, status = ops.pack_detections(boxes, conf, cls, img_offs,
                                                                   conf_thresh)
    mark("pack")
    # F and P of every capture: on the device by one launch behind the packing
    # (its per-capture status rides on the count copy below: no extra sync), or
    # host work while the packing runs
    F, proj, rig_status = _rig_launch(Ks, RTs, C, rig, dev, F, proj, mark)
    F_dev = F.reshape(-1)

    # one device -> host copy: the kept counts and the packing status (and the
    # device rig's per-capture status)
    ch = torch.cat([counts, status] + ([rig_status] if rig_status is not None else []))
    ch = ch.cpu().numpy().astype(np.int64)
    if rig_status is not None:
        ch, rig_bad = ch[:n_img + 1], np.nonzero(ch[n_img + 1:])[0]
        _rig_fallback(F, proj, rig_bad, Ks, RTs, S, C, on_device, dev)
    counts_host = ch[:-1]
    if ch[-1] != 0:
        raise ValueError("detector box with a non-finite or out-of-range coordinate")
    cam_offs_host = np.zeros(n_img + 1, np.int64)
    np.cumsum(counts_host, out=cam_offs_host[1:])
    mark("counts D2H")

    threshold = float(matching_threshold)
    full = _Rig(pts, cam_offs, cam_offs_host, counts_host.reshape(S, C), F_dev, proj)
    out = _match_rig(full, boxes_int, S, C, threshold, keep_cube, gate, refine, mark)
    if seeds:
        out.passes = _seed_passes(out, seeds, Ks, RTs, rig, on_device, S, C, threshold, gate, refine, mark)
    return out


def _check_refine(refine) -> Optional[int]:
    """``match_captures``' refine as the cap of the evaluations (None: off)."""
    if refine is None:
        return None
    if refine is True:
        return 10
    if isinstance(refine, (int, np.integer)) and not isinstance(refine, bool) and 1 <= refine <= 64:
        return int(refine)
    raise ValueError(f"refine: expected None, True or an int in 1..64, got {refine!r}")


def _check_extra_seeds(extra_seeds, C: int) -> tuple:
    """``match_captures``' extra_seeds as a tuple of triples (empty: None)."""
    if extra_seeds is None:
        return ()
    if C < 4:
        raise ValueError(f"extra_seeds needs n_cams >= 4, got n_cams={C}")
    seeds = tuple(ops_views._check_seed(seed, C) for seed in extra_seeds)
    if not 1 <= len(seeds) <= 4:
        raise ValueError(f"extra_seeds: expected 1 to 4 triples, got {len(seeds)}")
    return seeds


def _rig_launch(Ks, RTs, C, rig, dev, F, proj, mark):
    """F and P of every capture where ``rig`` says (what of ``F`` / ``proj`` is
    passed in is kept) -> (F, proj, the device rig's per-capture status or None)."""
    if rig == "device":
        F, proj, rig_status = ops.rig_matrices(Ks, RTs, pairs=extension_pairs(C) if C > 3 else None,
                                               device=dev)
        mark("F+P device")
        return F, proj, rig_status
    # once per distinct rig
    if F is None or proj is None:
        F_h, P_h = _host_rig(Ks, RTs, C)
        if F is None:
            F = torch.from_numpy(F_h).to(dev)
        if proj is None:
            proj = torch.from_numpy(P_h).to(dev)
    mark("F+P host")
    return F, proj, None


def _rig_fallback(F, proj, rig_bad, Ks, RTs, S, C, on_device, dev) -> None:
    """The captures ``rig_bad`` whose K the device rig refused: their rows of
    ``F`` / ``proj`` from the host, in place."""
    if rig_bad.size and on_device:
        raise ValueError(f"captures {rig_bad[:8].tolist()} have a K outside the pinhole form "
                         "mvm_rig_matrices inverts; pass Ks / RTs as host arrays (those captures "
                         "are then computed on the host) or use rig='host'")
    if rig_bad.size:
        # the kernel left those captures' rows unwritten: the host's values
        n_pairs = 3 + 3 * (C - 3)
        F_h, P_h = _host_rig(Ks[rig_bad], RTs[rig_bad], C)
        idx, = ops._h2d_int64([rig_bad], dev)
        F.view(S, 9 * n_pairs).index_copy_(0, idx,
                                           torch.from_numpy(F_h.reshape(-1, 9 * n_pairs)).to(dev))
        proj.index_copy_(0, idx, torch.from_numpy(P_h).to(dev))


def _seed_passes(first: MatchBatch, seeds, Ks, RTs, rig, on_device, S, C, threshold, gate, refine,
                 mark) -> tuple:
    """The extra seed passes behind the first: per triple the
    leftovers of every view as a sub-batch in the triple's camera order, F and
    P of the reordered rig by the call's ``rig`` path, and ``_match_rig`` on
    it.  One device -> host copy a pass beside ``_match_rig``'s: the leftover
    counts (the device rig's status rides on it)."""
    dev = first.pts.device
    full_offs = first.cam_offs_dev
    used = torch.zeros(int(first.pts.shape[0]), dtype=torch.int32, device=dev)
    ops_views.mark_used(first.views, first.offs_dev, first.count_dev, full_offs, used, C)
    mark("mark used")
    passes = []
    for p, seed in enumerate(seeds, 1):
        mark_p = lambda name, p=p: mark(f"pass {p}: {name}")
        order = ops_views.seed_order(seed, C)
        counts = ops_views.leftover_counts(used, full_offs, C, seed)
        mark_p("leftover counts")
        sel = list(order)
        Kp, RTp = Ks[:, sel], RTs[:, sel]
        if not isinstance(Kp, torch.Tensor):
            Kp, RTp = np.ascontiguousarray(Kp), np.ascontiguousarray(RTp)
        F, proj, rig_status = _rig_launch(Kp, RTp, C, rig, dev, None, None, mark_p)
        ch = torch.cat([counts] + ([rig_status] if rig_status is not None else []))
        ch = ch.cpu().numpy().astype(np.int64)
        if rig_status is not None:
            _rig_fallback(F, proj, np.nonzero(ch[S * C:])[0], Kp, RTp, S, C, on_device, dev)
        sub_counts = ch[:S * C]
        sub_offs = np.zeros(S * C + 1, np.int64)
        np.cumsum(sub_counts, out=sub_offs[1:])
        mark_p("leftover counts D2H")
        sub_offs_dev, = ops._h2d_int64([sub_offs], dev)
        pts, boxes, orig = ops_views.leftover_gather(used, first.pts, first.boxes, full_offs, sub_offs_dev,
                                                     C, seed, int(sub_offs[-1]))
        mark_p("leftover gather")
        sub = _Rig(pts, sub_offs_dev, sub_offs, sub_counts.reshape(S, C), F.reshape(-1), proj)
        res = _match_rig(sub, boxes, S, C, threshold, False, gate, refine, mark_p, cam_order=order,
                         orig=orig)
        passes.append(res)
        if p < len(seeds):
            ops_views.mark_used(res.views, res.offs_dev, res.count_dev, full_offs, used, C, seed,
                                sub_offs_dev, orig)
            mark_p("mark used")
    return tuple(passes)


def _match_rig(full: _Rig, boxes_int, S, C, threshold, keep_cube, gate, refine, mark, **fields) -> MatchBatch:
    """What follows the count copy: the three-camera chain on the first three
    views of ``full``, the extension into the others, the gate and the
    refinement if set -> the ``MatchBatch`` (``fields``: further fields of it)."""
    pts = full.pts
    dev = pts.device
    counts_host = full.counts.reshape(-1)
    n_pairs = 3 + 3 * (C - 3)
    three = full
    if C > 3:
        # cameras 0, 1, 2 of every capture as a three-camera batch of its own
        # (centroids, F and P gathered on the device); the existing chain runs
        # on it untouched
        rows = np.nonzero(np.repeat(np.arange(S * C) % C < 3, counts_host))[0].astype(np.int64)
        c3 = np.ascontiguousarray(full.counts[:, :3])
        co3 = np.zeros(3 * S + 1, np.int64)
        np.cumsum(c3.reshape(-1), out=co3[1:])
        sel, co3_dev = ops._h2d_int64([rows, co3], dev)
        three = _Rig(pts.index_select(0, sel) if rows.size else pts[:0], co3_dev, co3, c3,
                     full.F.view(S, n_pairs, 9)[:, :3].reshape(-1),
                     full.proj.view(S, C, 3, 4)[:, :3].contiguous())
        mark("three-view gather")
    free = ops.cube_free_scenes(three.counts) if not keep_cube else np.zeros(S, bool)
    if free.all() or not free.any():
        res = _device_chain(three, S, threshold, bool(free.all()) and S > 0, keep_cube, mark)
    else:
        # a mixed batch: the scenes of the candidate-list class without the
        # cube, the others (small views: the dense assignment classes read
        # the cost) with it; each part is a contiguous sub-batch
        res = _split_chain(three, S, threshold, free, mark)
    # one device -> host copy: assignment statuses and match counts
    sc = torch.cat([res.status, res.count]).cpu().numpy()
    bad, count_h = sc[:S], sc[S:]
    if np.any(bad):
        _raise_failed(bad)
    mark("results D2H")
    views = ext_cost = pruned = None
    if C > 3:
        views, ext_cost = _extend(full, res, count_h, S, C, threshold, mark)
    if gate is not None:
        pruned = torch.zeros(int(res.match.shape[0]), dtype=torch.int32, device=dev)
        if C > 3:
            ops_views.prune_views(views, ext_cost, res.X, res.offs_dev, res.count, full.pts, full.cam_offs,
                                  full.proj, gate, C, out=pruned)
            mark("prune")
    X = res.X
    if refine is not None:
        # over the views the gate left; the DLT points stay as X_dlt
        X, rms, info, cov = ops_views.refine_points(views if C > 3 else res.match, res.X, res.offs_dev,
                                                    res.count, full.pts, full.cam_offs, full.proj, C, refine)
        fields.update(X_dlt=res.X, refine_rms=rms, refine_info=info, cov=cov)
        mark("refine")
    return MatchBatch(match=res.match, cost=res.cost, X=X, count=count_h, offs=res.offs_host,
                      pts=full.pts, boxes=boxes_int, cam_offs=full.cam_offs_host,
                      cube=res.cube if keep_cube else None, offs_dev=res.offs_dev, count_dev=res.count,
                      cam_offs_dev=full.cam_offs, views=views, ext_cost=ext_cost, n_cams=C,
                      proj=full.proj.reshape(S, C, 3, 4), pruned=pruned, **fields)


def _extend(full: _Rig, res: _Chain, count_h, S, C, threshold, mark):
    """The extension of the three-view matches into cameras 3 .. C-1 (DESIGN
    §3.14): cost matrices -> assignment -> threshold + V-view DLT, behind the
    results copy (``count_h``: the match counts on the host).  ``res.X`` is
    updated in place.  -> (views int32 [cap, C], ext_cost f32 [cap, C - 3]).
    One device -> host copy: the assignment statuses."""
    pts, cam_offs, match, count, out_offs = full.pts, full.cam_offs, res.match, res.count, res.offs_dev
    dev = pts.device
    n_ext = C - 3
    cap = int(match.shape[0])
    views = torch.empty((cap, C), dtype=torch.int32, device=dev)
    ext_cost = torch.empty((cap, n_ext), dtype=torch.float32, device=dev)
    rows = np.repeat(np.asarray(count_h, np.int64), n_ext)
    cols = full.counts[:, 3:].reshape(-1).astype(np.int64)
    # every matrix starts on a 16-byte boundary (aligned rows then store 16 bytes a lane)
    ext_offs_host = np.zeros(S * n_ext + 1, np.int64)
    np.cumsum((rows * cols + 3) // 4 * 4, out=ext_offs_host[1:])
    max_rows = int(rows.max()) if rows.size else 0
    if cap == 0 or max_rows == 0:
        return views, ext_cost
    ext_offs, = ops._h2d_int64([ext_offs_host], dev)
    F_ext = full.F.view(S, 3 + 3 * n_ext, 9)[:, 3:].contiguous()
    E = ops.extend_costs(pts, cam_offs, F_ext, match, out_offs, count, ext_offs, C, max_rows,
                         size=int(ext_offs_host[-1]))
    mark("extend costs")
    lplan = ops.LsapPlan(rows, cols, device=dev)
    row_ind, col_ind, lstat = ops.linear_sum_assignment_batched(E, ext_offs[:-1].contiguous(), lplan)
    mark("extend lsap")
    ops.extend_select_triangulate(E, ext_offs, lplan.out_offs, row_ind, col_ind, match, out_offs, count,
                                  pts, cam_offs, full.proj, threshold, res.X, C, out=(views, ext_cost))
    mark("extend select")
    bad = lstat.cpu().numpy().reshape(S, n_ext).any(axis=1)
    if np.any(bad):
        _raise_failed(bad)
    mark("extend D2H")
    return views, ext_cost


def _device_chain(rig: _Rig, S, threshold, cube_free, keep_cube, mark) -> _Chain:
    """Cube (or, cube_free, its 8-row minima + pair residuals) -> assignment ->
    select/DLT of the S three-camera scenes of ``rig``."""
    pts, cam_offs, F_dev, proj_dev = rig.pts, rig.cam_offs, rig.F, rig.proj
    dev = pts.device
    plan = ops.TripletPlan(rig.cam_offs_host, S, device=dev)
    c3 = plan.counts
    mark("cube plan")
    if cube_free:
        # the assignment never reads a cube: the 32-column block minima its
        # candidate lists start from and the fp64 pair residuals it recomputes
        # its entries from (no 8-row minima: the lists gather
        # whole candidate blocks)
        minima = ops.triplet_minima(pts, cam_offs, F_dev, plan, with_bmin8=False)
        mark("cube")
        lplan = ops.LsapPlan(c3[:, 0] * c3[:, 1], c3[:, 2], device=dev, resid=True)
        mark("lsap plan")
        row_ind, col_ind, lstat = ops.linear_sum_assignment_resid(lplan, plan, minima)
        mark("lsap")
        match, cost, X, count = ops.select_triangulate_resid(plan, cam_offs, lplan.out_offs, row_ind,
                                                             col_ind, pts, proj_dev, threshold)
        mark("select")
        return _Chain(match, cost, X, lstat, count, lplan.out_offs_host, None, lplan.out_offs)
    # flattened cubes of the candidate-list class: the cube kernel also writes
    # the 8-row minima that class reduces
    bm8 = None
    nm = c3[:, 0] * c3[:, 1]
    if S and bool((ops.sparse_class(nm, c3[:, 2]) & (nm > c3[:, 2])).any()):
        bm8 = torch.empty(max(plan.n_bmin8, 1), dtype=torch.int16, device=dev)
    cube, _, _ = ops.triplet_cost_argmin(pts, cam_offs, F_dev, plan, bmin8=bm8)
    mark("cube")
    lplan = ops.LsapPlan(nm, c3[:, 2], device=dev)
    mark("lsap plan")
    row_ind, col_ind, lstat = ops.linear_sum_assignment_batched(
        cube, plan.cube_offs[:-1].contiguous(), lplan,
        bmin8=(bm8, plan.bmin8_offs, plan.segs) if bm8 is not None else None)
    mark("lsap")
    match, cost, X, count = ops.select_triangulate(cube, plan.cube_offs, cam_offs, lplan.out_offs,
                                                   row_ind, col_ind, pts, proj_dev, threshold)
    mark("select")
    return _Chain(match, cost, X, lstat, count, lplan.out_offs_host, cube if keep_cube else None,
                  lplan.out_offs)


def _split_chain(rig: _Rig, S, threshold, free, mark) -> _Chain:
    """_device_chain over the cube-free scenes and the others as two
    contiguous sub-batches (their centroids, F and P gathered on the device),
    merged back into the batch's scene order and assignment offsets."""
    pts, co, c3 = rig.pts, rig.cam_offs_host, rig.counts
    dev = pts.device
    caps = np.minimum(c3[:, 0] * c3[:, 1], c3[:, 2])
    out_offs = np.zeros(S + 1, np.int64)
    np.cumsum(caps, out=out_offs[1:])
    cap = int(out_offs[-1])
    match = torch.zeros((max(cap, 1), 3), dtype=torch.int32, device=dev)
    cost = torch.zeros(max(cap, 1), dtype=torch.float32, device=dev)
    X = torch.zeros((max(cap, 1), 3), dtype=torch.float64, device=dev)
    status = torch.zeros(S, dtype=torch.int32, device=dev)
    count = torch.zeros(S, dtype=torch.int32, device=dev)
    F3 = rig.F.reshape(S, 27)
    for part in (np.nonzero(free)[0], np.nonzero(~free)[0]):
        if part.size == 0:
            continue
        rows = np.concatenate([np.arange(co[3 * s], co[3 * s + 3]) for s in part]).astype(np.int64)
        sub_co = np.zeros(3 * part.size + 1, np.int64)
        np.cumsum(c3[part].reshape(-1), out=sub_co[1:])
        sel, idx, dst_rows, src_rows, sub_co_dev = ops._h2d_int64(
            [rows, part.astype(np.int64),
             np.concatenate([np.arange(out_offs[s], out_offs[s] + caps[s]) for s in part]).astype(np.int64),
             np.arange(int(caps[part].sum()), dtype=np.int64), sub_co], dev)
        sub_pts = pts.index_select(0, sel) if rows.size else pts[:0]
        sub = _device_chain(_Rig(sub_pts, sub_co_dev, sub_co, c3[part],
                                 F3.index_select(0, idx).reshape(-1), rig.proj.index_select(0, idx)),
                            part.size, threshold, bool(free[part[0]]), False, mark)
        if src_rows.numel():
            match.index_copy_(0, dst_rows, sub.match.index_select(0, src_rows))
            cost.index_copy_(0, dst_rows, sub.cost.index_select(0, src_rows))
            X.index_copy_(0, dst_rows, sub.X.index_select(0, src_rows))
        status.index_copy_(0, idx, sub.status)
        count.index_copy_(0, idx, sub.count)
    # the merged layout's offsets, for MatchBatch.table: uploaded once
    out_offs_dev, = ops._h2d_int64([out_offs], dev)
    return _Chain(match[:cap], cost[:cap], X[:cap], status, count, out_offs, None, out_offs_dev)


def _rig_inputs(batch: Sequence, n_cams: int = 3):
    """(Ks f32 [S,C,3,3], RTs f64 [S,C,4,4]) of one ``match_capture_stream`` batch."""
    boxes, conf, cls, img_offs, Ks, RTs = batch
    S = (int(img_offs.numel()) - 1) // n_cams
    return (np.asarray(Ks, dtype=np.float32).reshape(S, n_cams, 3, 3),
            np.asarray(RTs, dtype=np.float64).reshape(S, n_cams, 4, 4))


_TLS = threading.local()


class _ThreadPools:
    """One thread's RigWorkers by size.  Its finalizer closes them when the
    thread ends (its thread-local storage, the only strong reference to this
    holder, is released) or at interpreter exit, whichever comes first: a
    service that starts a thread per request does not accumulate worker
    processes or shared-memory slots."""

    def __init__(self):
        self.by_n = {}
        weakref.finalize(self, _ThreadPools._close_all, self.by_n)

    @staticmethod
    def _close_all(by_n):
        for pool in list(by_n.values()):
            pool.close()
        by_n.clear()


def rig_worker_pool(n: int):
    """The calling thread's ``RigWorkers`` of ``n`` processes (started on first
    use, reused by every stream of that thread, closed when the thread ends or
    at exit).  Per thread: a pool has one job in flight, and two threads
    streaming at once must not share it."""
    from .rig_workers import RigWorkers
    holder = getattr(_TLS, "pools", None)
    if holder is None:
        holder = _TLS.pools = _ThreadPools()
    pool = holder.by_n.get(n)
    if pool is None or not pool.procs:      # first use, or closed
        pool = holder.by_n[n] = RigWorkers(n)
    return pool


def match_capture_stream(batches: Iterable[Sequence], *, rig_workers: int = 3, rig: str = "host",
                         **kwargs) -> Iterator[MatchBatch]:
    """``match_captures`` over a sequence of batches, pipelined: the host F and
    P of batch b+1 (``rig_matrices``: numpy, the same function, so the same
    bits) are computed by ``rig_workers`` worker PROCESSES
    (``rig_workers.RigWorkers``, shared memory) while the main process runs
    batch b's device chain -- off its GIL, which a worker thread was not
    (DESIGN.md §3.10).  ``rig_workers=0`` computes them inline.  Each batch is
    ``(boxes, conf, cls, img_offs, Ks, RTs)`` as ``match_captures`` takes them;
    ``kwargs`` are passed through (``F`` / ``proj`` are computed here).
    Results equal ``match_captures`` on each batch.

    ``rig="device"`` / ``"auto"`` (``match_captures``' keyword): every batch
    is ``match_captures(..., rig=rig)``; there is no host F / P to overlap, so
    no worker pool is started or used (``rig_workers`` is ignored).

    ``n_cams`` (in ``kwargs``) is passed through; the worker processes compute
    three-camera rigs, so a stream of n_cams > 3 computes F / P inline.
    ``extra_seeds`` is passed through as well (it needs n_cams > 3, so that
    inline path), and so is ``refine``.
    """
    if "F" in kwargs or "proj" in kwargs:
        raise TypeError("match_capture_stream computes F and proj itself")
    _check_rig(rig)
    if rig != "host" or _check_n_cams(kwargs.get("n_cams", 3)) != 3:
        for cur in batches:
            yield match_captures(*cur, rig=rig, **kwargs)
        return
    it = iter(batches)
    cur = next(it, None)
    if cur is None:
        return
    pool = rig_worker_pool(rig_workers) if rig_workers > 0 else None
    try:
        ticket = pool.submit(*_rig_inputs(cur)) if pool is not None else None
        while cur is not None:
            F_h, P_h = pool.result(ticket) if pool is not None else rig_matrices(*_rig_inputs(cur))
            nxt = next(it, None)
            if nxt is not None and pool is not None:
                ticket = pool.submit(*_rig_inputs(nxt))   # batch b+1's F/P while batch b runs
            dev = cur[0].device
            yield match_captures(*cur, F=torch.from_numpy(F_h).to(dev),
                                 proj=torch.from_numpy(P_h).to(dev), **kwargs)
            cur = nxt
    finally:
        # a consumer that stops early (break, exception, the generator
        # collected) leaves batch b+1's job in flight: collect it, so the
        # thread's pool takes the next stream's submit
        if pool is not None:
            pool.drain()
