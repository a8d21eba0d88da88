"""The full-pose form of the scorer (ops_views.score_poses + match_scores,
DESIGN §3.20) on synthetic poses, beside two baselines on the same inputs: a
plain batched torch statement of BOP's direct form on the same device (the
yardstick) and the numpy model of tests/score_model.py on the host.

python tools/bench_score.py [--captures 1000 --rows 24 --objects 24 --verts 1024 --syms 8 --steps 5]
Every capture holds --rows estimates and --objects ground-truth poses; an
estimate is a ground-truth pose of its capture turned and moved a little.
Times are a host clock around the launches and one synchronise, the median of
--steps; the numpy model is timed on --cpu-captures captures and scaled.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import score_model as M  # noqa: E402
from bpc_baseline_amd import ops_views  # noqa: E402


def torch_direct(pose, gt, verts, syms, S, R, G, chunk):
    """min_k max_v |(Rp v + tp) - (Rg (Sk v + sk) + tg)| of every (row, object)
    pair of a capture, `chunk` captures at a time -> f64 [S R, G]."""
    out = torch.empty((S * R, G), dtype=torch.float64, device=pose.device)
    for s0 in range(0, S, chunk):
        s1 = min(s0 + chunk, S)
        P, Q = pose[s0 * R:s1 * R], gt[s0 * G:s1 * G]
        est = (verts @ P[:, :3, :3].transpose(1, 2) + P[:, None, :3, 3]).reshape(s1 - s0, R, 1, -1, 3)
        best = None
        for Sk in syms:
            vk = verts @ Sk[:3, :3].T + Sk[:3, 3]
            gtp = (vk @ Q[:, :3, :3].transpose(1, 2) + Q[:, None, :3, 3]).reshape(s1 - s0, 1, G, -1, 3)
            d = (est - gtp).square().sum(dim=-1).amax(dim=-1).sqrt()
            best = d if best is None else torch.minimum(best, d)
        out[s0 * R:s1 * R] = best.reshape(-1, G)
    return out


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return got, float(np.median(times)) * 1e3, [round(t * 1e3, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=24)
    ap.add_argument("--objects", type=int, default=24)
    ap.add_argument("--verts", type=int, default=1024)
    ap.add_argument("--syms", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=50, help="captures per batched torch step")
    ap.add_argument("--cpu-captures", type=int, default=2)
    args = ap.parse_args()
    S, R, G, V, K = args.captures, args.rows, args.objects, args.verts, args.syms
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(320)
    gt = M.random_poses(rng, S * G, t_max=300.0)
    pick = (np.arange(S)[:, None] * G + rng.integers(0, G, (S, R))).reshape(-1)
    pose = gt[pick].copy()
    turn = M.random_poses(rng, S * R, t_max=3.0)
    small = 0.02 * (turn[:, :3, :3] - np.eye(3)) + np.eye(3)            # near a rotation: a head's error
    pose[:, :3, :3] = pose[:, :3, :3] @ small
    pose[:, :3, 3] += turn[:, :3, 3]
    scene = np.repeat(np.arange(S), R).astype(np.int32)
    row_offs, gt_offs = np.arange(S + 1, dtype=np.int64) * R, np.arange(S + 1, dtype=np.int64) * G
    verts, syms = rng.uniform(-60, 60, (V, 3)), M.z_symmetries(K)
    thresholds = [2.0, 5.0, 10.0, 20.0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(pose=t(pose), scene=t(scene), gt=t(gt), gt_offs=t(gt_offs), verts=t(verts), syms=t(syms))

    def kernel():
        res = ops_views.score_poses(d["pose"], d["scene"], d["gt"], gt_offs, d["verts"], d["syms"])
        return res, ops_views.match_scores(res.err, row_offs, gt_offs, thresholds)

    def score_only():
        return ops_views.score_poses(d["pose"], d["scene"], d["gt"], gt_offs, d["verts"], d["syms"])

    (res, (gi, tp)), ms, all_ms = timed(kernel, args.steps)
    _, ms_score, _ = timed(score_only, args.steps)
    ref, ms_torch, all_torch = timed(lambda: torch_direct(d["pose"], d["gt"], d["verts"], d["syms"], S, R, G,
                                                          args.torch_chunk), args.steps)
    rel = ((res.err - ref).abs() / ref.clamp_min(1e-300)).max().item()
    c = max(1, min(args.cpu_captures, S))
    t0 = time.perf_counter()
    want = M.score_poses(pose[:c * R], scene[:c * R], gt, gt_offs, verts, syms)
    M.match_scores(want["err"], row_offs[:c + 1], gt_offs[:c + 1], thresholds)
    ms_numpy = (time.perf_counter() - t0) / c * S * 1e3
    assert M.same(res.err[:c * R].cpu().numpy(), want["err"]) and M.same(res.sym[:c * R].cpu().numpy(), want["sym"])
    recall, precision = ops_views.recall_precision(tp, row_offs, gt_offs)
    print(json.dumps({
        "config": {"captures": S, "rows_per_capture": R, "objects_per_capture": G, "verts": V, "syms": K,
                   "transformed_vertices": S * R * G * K * V, "thresholds_mm": thresholds},
        "kernels_ms": ms, "kernels_ms_all_steps": all_ms, "score_poses_ms": ms_score,
        "torch_direct_ms": ms_torch, "torch_direct_ms_all_steps": all_torch, "torch_chunk_captures": args.torch_chunk,
        "numpy_model_ms_scaled": ms_numpy, "numpy_captures_timed": c,
        "largest_relative_difference_to_torch_direct": rel,
        "recall": recall.tolist(), "precision": precision.tolist(),
        "note": "host clock around the launches and one device synchronise, median of the steps; kernels_ms is "
                "score_poses + match_scores through the wrappers (allocation of the outputs inside); the numpy "
                "model is timed on numpy_captures_timed captures and scaled"}))


if __name__ == "__main__":
    main()
