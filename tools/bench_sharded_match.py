"""Rank-sharded capture matching (distributed.match_captures_sharded): every
rank runs match_captures on its contiguous shard of make_detector_batch
captures, compacts the result into a MatchTable and the tables are gathered
to rank 0.

python tools/bench_sharded_match.py [--captures 1000 --dets 24 --steps 3]
torchrun --nproc-per-node N tools/bench_sharded_match.py ...   (one GPU per rank;
    MVM_DIST_BACKEND=gloo lets several ranks share one GPU: a rehearsal, not a measurement)

Rank 0 prints one JSON line: captures/s, each rank's split of chain, table and
gather time, the process group.  At one rank it also sets the table next to
the path it replaces: the compaction kernel's time and table().host() against
MatchBatch.host() (the D2H copy of the whole capacity).  A few steps, no retry.
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


def table_against_host(args_dev, kw, steps):
    """One rank: ms of the compaction alone (device events), of table() +
    MatchTable.host(), and of MatchBatch.host() on the same batch."""
    res = match_captures(*args_dev, **kw)
    res.table()                                        # first launch
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kernel, table_host, batch_host = [], [], []
    h = None
    for _ in range(steps):
        ev[0].record()
        tab = res.table()
        ev[1].record()
        torch.cuda.synchronize()
        kernel.append(ev[0].elapsed_time(ev[1]))
        # each host copy is timed with the other one, and its own earlier one, released
        vars(res).pop("_host", None)                   # host() keeps its copy
        h = None
        t0 = time.perf_counter()
        h = res.table().host()
        table_host.append((time.perf_counter() - t0) * 1e3)
        h = None
        t0 = time.perf_counter()
        res.host()
        batch_host.append((time.perf_counter() - t0) * 1e3)
    h = res.table().host()
    rows = int(tab.scene.shape[0])
    return {"matches": rows, "capacity_rows": int(res.match.shape[0]), "packed_rows": int(res.pts.shape[0]),
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
    args = ap.parse_args()
    env = init_from_env()
    a, b = shard_range(args.captures, env.rank, env.world)
    d = make_detector_batch(b - a, args.dets, seed=5, first_capture=a)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(env.device)
    args_dev = (t(d.boxes), t(d.conf), t(d.cls), t(d.img_offs), d.Ks, d.RTs)
    kw = {"keep_cube": args.keep_cube}
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
            "config": {"captures": args.captures, "dets_per_view": args.dets, "cams": 3,
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
