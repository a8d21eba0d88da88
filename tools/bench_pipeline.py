"""End-to-end batched capture matching (match_captures: pack -> cube -> LSAP ->
select + DLT) on the GPU, with a parity spot-check and the CPU chain beside it.

python tools/bench_pipeline.py [--captures 1000 --dets 24 --steps 5 --warmup 2] [--rig device]
Prints one JSON line (captures/s, ms per batch, CPU captures/s on a sample).
--rig device: F and P of every capture on the device (mvm_rig_matrices; the
stage "F+P host" becomes "F+P device"); the static-rig line is the floor either way.
--cams C (4..8): captures of C cameras from make_capture, matched with
match_captures(n_cams=C); --first-three matches only cameras 0-2
of the same captures, the three-camera line the extension is measured against.
--reproj-gate G (with --cams C > 3): match_captures(reproj_gate=G) (DESIGN
§3.15); the stage "prune" and the number of matches that dropped a view are
in the line.
--extra-seeds a,b,c[;a,b,c...] (with --cams C > 3):
match_captures(extra_seeds=[(a, b, c), ...]); the stages of
every extra pass ("pass 1: ...") and the matches each pass adds are in the line.
--refine [N] (with --cams C > 3): match_captures(refine=True or N) (DESIGN
§3.17); the stage "refine" and the distribution of the refinement's status and
evaluations over the matches are in the line.
--crops [ROWS] (with --cams C > 3): the pose head's input crops of the batch's
table (MatchTable.crops) in ranges of ROWS rows (default 256),
on synthetic uint8 images of --image-size H W held for --image-captures K
captures (row r reads the images of capture scene[r] mod K: 1000 captures of
2400 x 2400 images would be 69 GB); the stage time, crops per second and
output GB/s are in the line, beside the write probe over one range's bytes.
--poses MODE (with --cams C > 3; euler, quat, 6d or all): the batch's table
through MatchTable.poses on random raw vectors, all rows, all
cameras, fuse="mean"; the stage time (host clock around the launch and one
synchronise, median of --steps) is in the line, beside the same work done on the
host one row at a time through tests/pose_model.py, timed on --cpu-sample rows
and scaled to the table.
--score (with --cams C > 3): the batch's table against the synthetic object
centres through MatchTable.score: centre distances of every
(row, object) pair of a capture and the greedy matching at --score-thresholds
(mm); recall, precision and the stage time (host clock around the two launches
and one synchronise, median of --steps) are in the line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bpc_baseline_amd.inference.batch_match import match_capture_stream, match_captures  # noqa: E402
from bpc_baseline_amd.inference.utils.camera_utils import camera_pairs, fundamental_matrices  # noqa: E402
from bpc_baseline_amd.synth import make_detector_batch  # noqa: E402


def cpu_chain(b, s):
    """One capture through the CPU restatements (oracle) + scipy, as the
    reference computes it: _detect packing, F, cube, LSA, filter, sort, DLT."""
    from scipy.optimize import linear_sum_assignment
    from oracle import oracle as O
    from oracle import pipeline as OP
    o = b.img_offs[3 * s:3 * s + 4]
    sl = slice(int(o[0]), int(o[3]))
    bbox, cent, co = OP.detect_pack(b.boxes[sl], b.conf[sl], b.cls[sl], o - o[0], 0.1)
    F = fundamental_matrices(list(b.Ks[s]), list(b.RTs[s]), camera_pairs(3))
    n = np.diff(co)
    cube = O.cube(cent, co, F, 1, nthreads=1)[0].reshape(n)
    flat = cube.reshape(n[0] * n[1], n[2])
    r, c = linear_sum_assignment(flat)
    m = [(int(i) // n[1], int(i) % n[1], int(k)) for i, k in zip(r, c) if flat[i, k] < 30]
    m = sorted(m, key=lambda t: cube[t])
    P = np.stack([b.Ks[s][v] @ b.RTs[s][v][:3] for v in range(3)])
    X = [OP.triangulate(P[None], cent[co[:3] + np.array(t)][None])[0] for t in m]
    return m, X


def wide_batch(captures, dets, C, seed=5, centres=None):
    """Detector outputs of `captures` C-camera captures (make_capture: half of
    every view true objects, half clutter), capture s from default_rng(seed + s)
    -> (boxes f32 [n, 4], conf, cls, img_offs i64 [C S + 1], Ks, RTs).
    ``centres``: a list that gets every capture's object centres f64 [n_obj, 3]."""
    from bpc_baseline_amd.synth import make_capture_gt
    boxes, counts = [], []
    Ks, RTs = np.empty((captures, C, 3, 3), np.float32), np.empty((captures, C, 4, 4))
    for s in range(captures):
        k, rt, det, X = make_capture_gt(np.random.default_rng(seed + s), C, dets)
        if centres is not None:
            centres.append(X)
        Ks[s], RTs[s] = np.stack(k), np.stack(rt)
        for c in range(C):
            boxes.append(np.array([d["bbox"] for d in det[c]], np.float32).reshape(-1, 4))
            counts.append(len(det[c]))
    offs = np.zeros(captures * C + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    boxes = np.concatenate(boxes)
    return boxes, np.full(len(boxes), 0.9, np.float32), np.zeros(len(boxes), np.float32), offs, Ks, RTs


def bench_crops(res, args, dev):
    """--crops: every row of the batch's table through MatchTable.crops in
    ranges of args.crops rows -> the line's "crops" entry."""
    import dataclasses
    from bpc_baseline_amd import ops
    C, (H, W) = args.cams, args.image_size
    K = max(1, min(args.image_captures, args.captures))
    gen = torch.Generator(device=dev)
    gen.manual_seed(318)
    images = torch.randint(0, 256, (K, C, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    tab = res.table_all() if res.passes else res.table(reproj=True)
    tab = dataclasses.replace(tab, scene=tab.scene % K)
    n, step = int(tab.offs[-1]), args.crops
    dtype = torch.float16 if args.crop_dtype == "float16" else torch.float32
    ranges = [(b, min(b + step, n)) for b in range(0, n, step)]
    kw = dict(cams=args.crop_cams, size=args.crop_size, dtype=dtype)
    for r in ranges[:3]:
        crops, geom = tab.crops(images, rows=r, **kw)
    torch.cuda.synchronize()
    status = np.zeros(5, np.int64)
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        for r in ranges:
            crops, geom = tab.crops(images, rows=r, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    for r in ranges:
        status += np.bincount(tab.crops(images, rows=r, **kw)[1][..., 0].reshape(-1).cpu().numpy(), minlength=5)
    n_sel = C if args.crop_cams is None else len(args.crop_cams)
    dt = float(np.median(times))
    out_bytes = n * n_sel * 3 * args.crop_size ** 2 * (2 if dtype == torch.float16 else 4)
    # the write probe over one range's output bytes, as often as there are ranges
    buf = torch.empty(min(step, n) * n_sel * 3 * args.crop_size ** 2, dtype=dtype, device=dev)
    ops.hbm_write_probe(buf)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps * len(ranges)):
        ops.hbm_write_probe(buf)
    torch.cuda.synchronize()
    probe = buf.numel() * buf.element_size() * args.steps * len(ranges) / (time.perf_counter() - t0)
    return {"rows": n, "rows_per_range": step, "ranges": len(ranges), "cams": n_sel, "size": args.crop_size,
            "dtype": args.crop_dtype, "image_size": [H, W], "image_captures": K,
            "stage_ms": dt * 1e3, "stage_ms_all_steps": [round(t * 1e3, 3) for t in times],
            "crops_per_s": n * n_sel / dt, "output_GBps": out_bytes / dt / 1e9,
            "write_probe_GBps": probe / 1e9, "status_counts": status.tolist(),
            "note": "host clock around every range's launch and one device synchronise; the allocation of "
                    "each range's output (torch's caching allocator) is inside the stage"}


def bench_poses(res, args, dev, RTs):
    """--poses: every row and camera of the batch's table through
    MatchTable.poses -> the line's "poses" entry, one item per mode."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import pose_model as M
    C = args.cams
    tab = res.table_all() if res.passes else res.table(reproj=True)
    n = int(tab.offs[-1])
    RTs = np.ascontiguousarray(RTs, np.float64)
    rts_dev = torch.from_numpy(RTs).to(dev)
    host = tab.host()
    rng = np.random.default_rng(319)
    out = {"rows": n, "cams": C, "fuse": "mean", "modes": {}}
    for mode in (("euler", "quat", "6d") if args.poses == "all" else (args.poses,)):
        raw_h = M.random_raw(rng, n * C, mode).reshape(n, C, -1)
        raw = torch.from_numpy(raw_h).to(dev)
        for _ in range(3):
            got = tab.poses(raw, rts_dev, mode, fuse="mean")
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            got = tab.poses(raw, rts_dev, mode, fuse="mean")
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        k = max(1, min(args.cpu_sample, n))
        t0 = time.perf_counter()
        for r in range(k):
            M.fuse_rotations(raw_h[r:r + 1], host["scene"], host["views"], host["X"], RTs, mode, rows=(r, r + 1),
                             fuse="mean")
        per_row = (time.perf_counter() - t0) / k
        out["modes"][mode] = {"stage_ms": float(np.median(times)) * 1e3,
                              "stage_ms_all_steps": [round(t * 1e3, 4) for t in times],
                              "slots_per_s": n * C / float(np.median(times)),
                              "host_row_at_a_time_ms": per_row * n * 1e3, "host_rows_timed": k,
                              "row_status_counts": np.bincount(got.row_status.cpu().numpy(), minlength=3).tolist()}
    out["note"] = ("host clock around the launch and one device synchronise; the allocation of the outputs "
                   "(torch's caching allocator) is inside the stage; the host figure is the numpy model called "
                   "on one row at a time, scaled from host_rows_timed rows to the table")
    return out


def bench_score(res, args, dev, centres):
    """--score: the batch's table against the captures' object centres through
    MatchTable.score -> the line's "score" entry."""
    from bpc_baseline_amd import ops_views
    tab = res.table_all() if res.passes else res.table(reproj=True)
    n = int(tab.offs[-1])
    gt_offs = np.concatenate([[0], np.cumsum([len(X) for X in centres])]).astype(np.int64)
    gt = np.tile(np.eye(4), (int(gt_offs[-1]), 1, 1))
    gt[:, :3, 3] = np.concatenate(centres)
    gt_dev = torch.from_numpy(gt).to(dev)
    thresholds = list(args.score_thresholds)
    for _ in range(3):
        got = tab.score(gt_dev, gt_offs, thresholds=thresholds)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        got = tab.score(gt_dev, gt_offs, thresholds=thresholds)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    recall, precision = ops_views.recall_precision(got.tp, tab.offs, gt_offs)
    return {"rows": n, "objects": int(gt_offs[-1]), "g_max": int(got.err.shape[1]), "thresholds_mm": thresholds,
            "recall": [round(v, 6) for v in recall.tolist()],
            "precision": [round(v, 6) for v in precision.tolist()],
            "average_recall": round(float(recall.mean()), 6),
            "stage_ms": float(np.median(times)) * 1e3, "stage_ms_all_steps": [round(t * 1e3, 4) for t in times],
            "note": "identity rotations at the table's X against the synthetic centres, one origin vertex: err is "
                    "the centre distance; host clock around the score and match launches and one device "
                    "synchronise; the estimates' assembly, the offsets' upload and the allocation of the outputs "
                    "are inside the stage"}


def main_wide(args):
    """--cams C > 3: ms per batch and synchronised stage times of
    match_captures(n_cams=C), or (--first-three) of the three-camera chain on
    cameras 0-2 of the same captures."""
    dev = torch.device("cuda", 0)
    C = args.cams
    centres = [] if args.score else None
    boxes, conf, cls, offs, Ks, RTs = wide_batch(args.captures, args.dets, C, centres=centres)
    kw = dict(keep_cube=args.keep_cube, rig=args.rig)
    if args.first_three:
        rows = np.concatenate([np.arange(offs[C * s], offs[C * s + 3]) for s in range(args.captures)])
        n3 = np.diff(offs).reshape(-1, C)[:, :3].reshape(-1)
        offs = np.concatenate([[0], np.cumsum(n3)]).astype(np.int64)
        boxes, conf, cls = boxes[rows], conf[rows], cls[rows]
        Ks, RTs = np.ascontiguousarray(Ks[:, :3]), np.ascontiguousarray(RTs[:, :3])
    else:
        kw["n_cams"] = C
        if args.reproj_gate is not None:
            kw["reproj_gate"] = args.reproj_gate
        if args.extra_seeds:
            kw["extra_seeds"] = [tuple(int(c) for c in seed.split(",")) for seed in args.extra_seeds.split(";")]
        if args.refine is not None:
            kw["refine"] = True if args.refine == 0 else args.refine
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    inp = (t(boxes), t(conf), t(cls), t(offs), Ks, RTs)
    for _ in range(args.warmup):
        res = match_captures(*inp, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = match_captures(*inp, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    stages = {}
    for _ in range(args.steps):
        match_captures(*inp, timings=stages, **kw)
    stages = {k: round(v / args.steps * 1e3, 3) for k, v in stages.items()}
    out = {"metric": "captures matched/sec (detect-pack + cube + LSAP + select + DLT"
                     + ("" if args.first_three else " + extension") + ")",
           "value": args.captures / dt, "unit": "captures/s", "ms_per_batch": dt * 1e3,
           "config": {"captures": args.captures, "dets_per_view": args.dets, "cams": C,
                      "matched_cams": 3 if args.first_three else C, "keep_cube": args.keep_cube,
                      "rig": args.rig, **({"reproj_gate": kw["reproj_gate"]} if "reproj_gate" in kw else {})},
           "matches": int(res.count.sum()), "stage_ms_synchronised": stages}
    if res.pruned is not None:
        out["prune_ms_synchronised"] = stages.get("prune")
        out["matches_that_dropped_a_view"] = int((res.pruned != 0).sum())
    if res.refine_info is not None:
        keep = np.concatenate([np.arange(o, o + n) for o, n in zip(res.offs[:-1], res.count)]
                              + [np.zeros(0, np.int64)]).astype(np.int64)
        info = res.refine_info.cpu().numpy()[keep]
        out["config"]["refine"] = kw["refine"]
        out["refine_ms_synchronised"] = stages.get("refine")
        out["refine_status_counts"] = np.bincount(info[:, 0], minlength=4).tolist()
        out["refine_evals_counts"] = np.bincount(info[:, 1]).tolist()
    if res.passes:
        out["config"]["extra_seeds"] = [list(seed) for seed in kw["extra_seeds"]]
        out["matches_per_extra_pass"] = [int(p.count.sum()) for p in res.passes]
    if not args.first_three:
        v = res.views.cpu().numpy()
        keep = np.concatenate([np.arange(o, o + n) for o, n in zip(res.offs[:-1], res.count)]
                              + [np.zeros(0, np.int64)]).astype(np.int64)
        out["matches_with_an_extra_view"] = int((v[keep, 3:] >= 0).any(axis=1).sum())
    if args.crops is not None:
        out["crops"] = bench_crops(res, args, dev)
    if args.poses is not None:
        out["poses"] = bench_poses(res, args, dev, RTs)
    if args.score:
        out["score"] = bench_score(res, args, dev, centres)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=3, choices=range(3, 9),
                    help="cameras per capture; above 3: make_capture captures through "
                         "match_captures(n_cams=C) (DESIGN §3.14)")
    ap.add_argument("--first-three", action="store_true",
                    help="with --cams C > 3: match cameras 0-2 of the same captures only")
    ap.add_argument("--reproj-gate", type=float, default=None,
                    help="with --cams C > 3: match_captures(reproj_gate=G), pixels (DESIGN §3.15)")
    ap.add_argument("--extra-seeds", default=None, metavar="a,b,c[;a,b,c...]",
                    help="with --cams C > 3: match_captures(extra_seeds=[(a, b, c), ...]) (DESIGN §3.16)")
    ap.add_argument("--refine", type=int, nargs="?", const=0, default=None, metavar="N",
                    help="with --cams C > 3: match_captures(refine=True), or refine=N evaluations (DESIGN §3.17)")
    ap.add_argument("--crops", type=int, nargs="?", const=256, default=None, metavar="ROWS",
                    help="with --cams C > 3: MatchTable.crops over the table in ranges of ROWS rows (DESIGN §3.18)")
    ap.add_argument("--image-size", type=int, nargs=2, default=(2400, 2400), metavar=("H", "W"),
                    help="with --crops: the synthetic images' size")
    ap.add_argument("--image-captures", type=int, default=16, metavar="K",
                    help="with --crops: captures whose images are held (row r reads capture scene[r] mod K)")
    ap.add_argument("--crop-size", type=int, default=256, help="with --crops: the canvas side")
    ap.add_argument("--crop-cams", type=lambda v: tuple(int(c) for c in v.split(",")), default=None,
                    metavar="a[,b...]", help="with --crops: the cameras wanted (default all)")
    ap.add_argument("--crop-dtype", choices=("float32", "float16"), default="float32")
    ap.add_argument("--poses", choices=("euler", "quat", "6d", "all"), default=None, metavar="MODE",
                    help="with --cams C > 3: MatchTable.poses over the table, fuse=\"mean\" (DESIGN §3.19)")
    ap.add_argument("--score", action="store_true",
                    help="with --cams C > 3: MatchTable.score of the table against the synthetic centres (DESIGN §3.20)")
    ap.add_argument("--score-thresholds", type=lambda v: tuple(float(x) for x in v.split(",")),
                    default=(1.0, 2.0, 5.0, 10.0), metavar="a[,b...]",
                    help="with --score: the centre-distance thresholds, mm")
    ap.add_argument("--captures", type=int, default=1000)
    ap.add_argument("--dets", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-sample", type=int, default=50)
    ap.add_argument("--keep-cube", action="store_true",
                    help="match_captures(keep_cube=True): the cube written and read (default: cube-free "
                         "where the batch allows)")
    ap.add_argument("--rig-group", type=int, default=1,
                    help="consecutive captures sharing one camera rig (IPD: the images of a scene)")
    ap.add_argument("--rig", choices=("host", "device"), default="host",
                    help="where match_captures computes F and P (DESIGN §3.13)")
    args = ap.parse_args()
    if args.reproj_gate is not None and (args.cams == 3 or args.first_three):
        ap.error("--reproj-gate needs --cams C > 3 without --first-three (it acts on the extra views)")
    if args.refine is not None and (args.cams == 3 or args.first_three):
        ap.error("--refine needs --cams C > 3 without --first-three")
    if args.crops is not None and (args.cams == 3 or args.first_three or args.crops < 1):
        ap.error("--crops needs --cams C > 3 without --first-three, and ROWS >= 1")
    if args.poses is not None and (args.cams == 3 or args.first_three):
        ap.error("--poses needs --cams C > 3 without --first-three")
    if args.score and (args.cams == 3 or args.first_three):
        ap.error("--score needs --cams C > 3 without --first-three")
    if args.cams > 3:
        return main_wide(args)
    dev = torch.device("cuda", 0)
    b = make_detector_batch(args.captures, args.dets, seed=5)
    if args.rig_group > 1:   # rig of the group's first capture (match_captures dedupes F/P)
        src = np.arange(args.captures) // args.rig_group * args.rig_group
        b.Ks, b.RTs = np.ascontiguousarray(b.Ks[src]), np.ascontiguousarray(b.RTs[src])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    boxes, conf, cls, offs = t(b.boxes), t(b.conf), t(b.cls), t(b.img_offs)
    res = None
    for _ in range(args.warmup):
        res = match_captures(boxes, conf, cls, offs, b.Ks, b.RTs, keep_cube=args.keep_cube, rig=args.rig)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = match_captures(boxes, conf, cls, offs, b.Ks, b.RTs, keep_cube=args.keep_cube, rig=args.rig)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    # a static rig: F and P computed once and passed in
    from bpc_baseline_amd.inference.batch_match import projection_matrices
    from bpc_baseline_amd.inference.utils.camera_utils import fundamental_matrices_batched
    Fd = torch.from_numpy(fundamental_matrices_batched(b.Ks, b.RTs, camera_pairs(3))).to(dev)
    Pd = torch.from_numpy(projection_matrices(b.Ks, b.RTs)).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        match_captures(boxes, conf, cls, offs, b.Ks, b.RTs, F=Fd, proj=Pd, keep_cube=args.keep_cube)
    torch.cuda.synchronize()
    dt_cached = (time.perf_counter() - t0) / args.steps
    # the same batches through the pipelined stream (host F/P of batch b+1
    # in worker processes while batch b runs on the device)
    batches = [(boxes, conf, cls, offs, b.Ks, b.RTs)] * args.steps
    for _ in match_capture_stream(batches[:2], rig=args.rig):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in match_capture_stream(batches, rig=args.rig):
        res_stream = r
    torch.cuda.synchronize()
    dt_stream = (time.perf_counter() - t0) / args.steps
    # the same stream with F/P computed inline (no worker processes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in match_capture_stream(batches, rig_workers=0, rig=args.rig):
        pass
    torch.cuda.synchronize()
    dt_inline = (time.perf_counter() - t0) / args.steps
    assert np.array_equal(res_stream.count, res.count)
    ms, mr = res_stream.match.cpu().numpy(), res.match.cpu().numpy()
    for s in range(args.captures):   # rows past count[s] are unused capacity
        o, k = int(res.offs[s]), int(res.count[s])
        assert np.array_equal(ms[o:o + k], mr[o:o + k]), s
    stages = {}
    for _ in range(args.steps):
        match_captures(boxes, conf, cls, offs, b.Ks, b.RTs, timings=stages, keep_cube=args.keep_cube, rig=args.rig)
    stages = {k: round(v / args.steps * 1e3, 3) for k, v in stages.items()}

    # parity spot-check on a few captures, then the CPU chain on a sample
    rng = np.random.default_rng(0)
    check = rng.choice(args.captures, min(20, args.captures), replace=False)
    for s in check:
        m, X = cpu_chain(b, int(s))
        o, n = int(res.offs[s]), int(res.count[s])
        got = res.match[o:o + n].cpu().numpy()
        assert n == len(m) and np.array_equal(got, np.asarray(m, np.int64).reshape(-1, 3)), s
        if n:
            np.testing.assert_allclose(res.X[o:o + n].cpu().numpy(), np.stack(X), rtol=1e-10, atol=1e-9)
    k = min(args.cpu_sample, args.captures)
    t1 = time.perf_counter()
    for s in range(k):
        cpu_chain(b, s)
    cpu = k / (time.perf_counter() - t1)
    print(json.dumps({
        "metric": "captures matched/sec (detect-pack + cube + LSAP + select + DLT)",
        "value": args.captures / dt, "unit": "captures/s", "ms_per_batch": dt * 1e3,
        "config": {"captures": args.captures, "dets_per_view": args.dets, "cams": 3, "keep_cube": args.keep_cube,
                   "captures_per_rig": args.rig_group, "rig": args.rig},
        "matches": int(res.count.sum()), "parity_checked": len(check),
        "stage_ms_synchronised": stages,
        "stream": {"value": args.captures / dt_stream, "ms_per_batch": dt_stream * 1e3,
                   "inline_ms_per_batch": dt_inline * 1e3,
                   "note": "match_capture_stream: host F/P of the next batch computed by 3 worker "
                           "processes (shared memory) while this batch's device chain runs; "
                           "inline: the same stream with F/P in the main process"},
        "static_rig": {"value": args.captures / dt_cached, "ms_per_batch": dt_cached * 1e3,
                       "note": "F and P computed once and passed in (fixed camera rig)"},
        "cpu_chain": {"value": cpu, "unit": "captures/s", "cores": 1, "kind": "port",
                      "sample": f"first {k} captures, oracle C cube + scipy LSA + numpy SVD"},
    }))


if __name__ == "__main__":
    main()
