"""Rank-sharded capture matching (distributed.match_captures_sharded): every
rank runs match_captures on its contiguous shard of make_detector_batch
captures, compacts the result into a MatchTable and the tables are gathered
to rank 0.

python tools/bench_sharded_match.py [--captures 1000 --dets 24 --steps 3 --cams C]
torchrun --nproc-per-node N tools/bench_sharded_match.py ...   (one GPU per rank;
    MVM_DIST_BACKEND=gloo lets several ranks share one GPU: a rehearsal, not a measurement)

Rank 0 prints one JSON line: captures/s, each rank's split of chain, table and
gather time, the process group.  At one rank it also sets the table next to
the path it replaces: the compaction kernel's time and table().host() against
MatchBatch.host() (the D2H copy of the whole capacity).  A few steps, no retry.

--cams C (4..8): captures of C cameras from make_capture through
match_captures(n_cams=C); the table then comes from mvm_compact_matches_views
(all C view slots + reprojection residuals), and the path it is set against
is MatchBatch.host() plus the predictions() loop over every capture, the only
way out of such a batch without the table.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bpc_baseline_amd.distributed import (gather_rows, init_from_env, match_captures_sharded,  # noqa: E402
                                          shard_range)
from bpc_baseline_amd.inference.batch_match import match_captures  # noqa: E402
from bpc_baseline_amd.synth import make_detector_batch  # noqa: E402


def wide_shard(a, b, dets, C, seed=5):
    """Detector outputs of the C-camera captures [a, b) (make_capture, capture s
    from default_rng(seed + s), as tools/bench_pipeline.py --cams)
    -> (boxes f32 [n, 4], conf, cls, img_offs i64 [C S + 1], Ks, RTs)."""
    from bpc_baseline_amd.synth import make_capture
    S = b - a
    boxes, counts = [np.zeros((0, 4), np.float32)], []
    Ks, RTs = np.empty((S, C, 3, 3), np.float32), np.empty((S, C, 4, 4))
    for s in range(S):
        k, rt, det = make_capture(np.random.default_rng(seed + a + s), C, dets)
        Ks[s], RTs[s] = np.stack(k), np.stack(rt)
        for c in range(C):
            boxes.append(np.array([d["bbox"] for d in det[c]], np.float32).reshape(-1, 4))
            counts.append(len(det[c]))
    offs = np.zeros(S * C + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    boxes = np.concatenate(boxes)
    return boxes, np.full(len(boxes), 0.9, np.float32), np.zeros(len(boxes), np.float32), offs, Ks, RTs


def table_against_host(args_dev, kw, steps):
    """One rank: ms of the compaction alone (device events), of table() +
    MatchTable.host(), and of MatchBatch.host() on the same batch -- for a
    batch of n_cams > 3 also of MatchBatch.host() + the predictions() loop over
    every capture, and of the table's own predictions() loop."""
    res = match_captures(*args_dev, **kw)
    tab_kw = {"reproj": True} if res.n_cams > 3 else {}
    res.table(**tab_kw)                                       # first launch
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kernel, table_host, batch_host = [], [], []
    h = None
    for _ in range(steps):
        ev[0].record()
        tab = res.table(**tab_kw)
        ev[1].record()
        torch.cuda.synchronize()
        kernel.append(ev[0].elapsed_time(ev[1]))
        # each host copy is timed with the other one, and its own earlier one, released
        vars(res).pop("_host", None)                   # host() keeps its copy
        h = None
        t0 = time.perf_counter()
        h = res.table(**tab_kw).host()
        table_host.append((time.perf_counter() - t0) * 1e3)
        h = None
        t0 = time.perf_counter()
        res.host()
        batch_host.append((time.perf_counter() - t0) * 1e3)
    wide = {}
    if res.n_cams > 3:
        S = int(res.count.size)
        loop, table_loop = [], []
        for _ in range(steps):
            vars(res).pop("_host", None)
            t0 = time.perf_counter()
            for s in range(S):
                res.predictions(s)
            loop.append((time.perf_counter() - t0) * 1e3)
            tab = res.table(**tab_kw)
            t0 = time.perf_counter()
            for s in range(S):
                tab.predictions(s)
            table_loop.append((time.perf_counter() - t0) * 1e3)
        wide = {"batch_host_predictions_ms": min(loop), "table_host_predictions_ms": min(table_loop),
                "wide_note": "batch_host_predictions_ms: MatchBatch.host() + predictions(s) for every capture; "
                             "table_host_predictions_ms: MatchTable.host() + its predictions(s) for every "
                             "capture (table() itself not included: compact_ms)"}
    h = res.table(**tab_kw).host()
    rows = int(tab.scene.shape[0])
    return {**wide, "matches": rows, "capacity_rows": int(res.match.shape[0]), "packed_rows": int(res.pts.shape[0]),
            "table_bytes": int(sum(v.nbytes for v in h.values())),
            "batch_host_bytes": int(sum(v.nbytes for v in res.host().values())),
            "compact_ms": min(kernel), "table_host_ms": min(table_host), "batch_host_ms": min(batch_host),
            "note": "best of the steps; compact_ms: table() between two events (the zero fill of the offsets, "
                    "the prefix sum and the copy kernel); table_host_ms: table() + one D2H of its rows; "
                    "batch_host_ms: MatchBatch.host(), the D2H of the whole capacity that predictions() read"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=1000, help="captures over all ranks")
    ap.add_argument("--dets", type=int, default=24, help="detections per view")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--keep-cube", action="store_true")
    ap.add_argument("--cams", type=int, default=3, choices=range(3, 9),
                    help="cameras per capture; above 3: make_capture captures through "
                         "match_captures(n_cams=C), the table with reprojection residuals")
    args = ap.parse_args()
    env = init_from_env()
    a, b = shard_range(args.captures, env.rank, env.world)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(env.device)
    kw = {"keep_cube": args.keep_cube}
    if args.cams > 3:
        w = wide_shard(a, b, args.dets, args.cams)
        args_dev = (t(w[0]), t(w[1]), t(w[2]), t(w[3]), w[4], w[5])
        kw["n_cams"] = args.cams
    else:
        d = make_detector_batch(b - a, args.dets, seed=5, first_capture=a)
        args_dev = (t(d.boxes), t(d.conf), t(d.cls), t(d.img_offs), d.Ks, d.RTs)
    table = match_captures_sharded(env, *args_dev, **kw)              # warm-up
    torch.cuda.synchronize()
    env.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        table = match_captures_sharded(env, *args_dev, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps        # rank 0 holds the tables last
    split = {}
    for _ in range(args.steps):
        match_captures_sharded(env, *args_dev, split=split, **kw)
    mine = torch.tensor([split[k] / args.steps * 1e3 for k in ("chain", "table", "gather")],
                        dtype=torch.float64, device=env.device)
    per_rank = gather_rows(env, mine)
    if env.is_root:
        per_rank = per_rank[0].cpu().numpy().reshape(env.world, 3)
        line = {
            "metric": "captures matched/sec, rank-sharded (chain + match table + gather to rank 0)",
            "value": args.captures / dt, "unit": "captures/s", "ms_per_step": dt * 1e3,
            "config": {"captures": args.captures, "dets_per_view": args.dets, "cams": args.cams,
                       "keep_cube": args.keep_cube, "steps": args.steps},
            "process_group": {"world_size": env.world, "backend": env.backend if env.initialised else None},
            "matches": int(table.scene.shape[0]),
            "rank_split_ms_synchronised": [
                {"rank": r, "captures": int(np.diff(shard_range(args.captures, r, env.world))[0]),
                 "chain": round(float(c), 3), "table": round(float(tb), 3), "gather": round(float(g), 3)}
                for r, (c, tb, g) in enumerate(per_rank)],
        }
        if env.world == 1:
            line["table_vs_host"] = table_against_host(args_dev, kw, args.steps)
        print(json.dumps(line))
    env.barrier()
    if env.initialised:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
