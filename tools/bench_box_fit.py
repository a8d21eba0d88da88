"""Timing of the box fit: 1000 captures x 24 rows x 4 cameras,
every row keeping all four views, a model of V = 64 and of V = 1024 vertices;
the kernel against a batched torch statement of one evaluation (projection,
extremes, residuals, A and g) times the kernel's mean number of evaluations.
Each a median of 5 with the host clock around the launch and one synchronise.
There is no bit equality here: torch orders its sums as it likes.  Prints one
JSON line.  Run from the repository root."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import box_fit_inputs as I                      # noqa: E402
from bpc_baseline_amd import ops_views          # noqa: E402
from bpc_baseline_amd.inference.utils.camera_utils import projection_matrices   # noqa: E402
from bpc_baseline_amd.synth import make_rig     # noqa: E402
from score_model import random_rotations        # noqa: E402

dev = torch.device("cuda", 0)
S, per, C = 1000, 24, 4
n = S * per


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), [round(v, 4) for v in out]


def inputs(V, seed=1):
    """One rig for all captures; true poses, truncated exact boxes, and a start
    some 30 mm off the truth (what the triangulated box centres are)."""
    rng = np.random.default_rng(seed)
    Ks, RTs = make_rig(rng, C)
    P = projection_matrices(np.stack(Ks)[None], np.stack(RTs)[None])[0]
    verts = I.cloud(rng, V)
    R = random_rotations(rng, n)
    t = np.stack([rng.uniform(-250, 250, n), rng.uniform(-250, 250, n), rng.uniform(-80, 80, n)], 1)
    boxes = np.zeros((n, C, 4), np.int32)
    for b in range(0, n, 1000):                        # in pieces: [rows, C, V, 3] is large at V = 1024
        X = np.einsum("nij,vj->nvi", R[b:b + 1000], verts) + t[b:b + 1000, None]
        h = np.einsum("cij,nvj->ncvi", P[:, :, :3], X) + P[None, :, None, :, 3]
        u, v = h[..., 0] / h[..., 2], h[..., 1] / h[..., 2]
        boxes[b:b + 1000] = np.trunc(np.stack([u.min(2), v.min(2), u.max(2), v.max(2)], 2))
    pose = np.tile(np.eye(4), (n, 1, 1))
    pose[:, :3, :3], pose[:, :3, 3] = R, t + rng.normal(0.0, 17.0, (n, 3))
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(pose=to(pose), scene=to(np.repeat(np.arange(S), per).astype(np.int32)),
                views=torch.zeros((n, C), dtype=torch.int32, device=dev), boxes=to(boxes),
                proj=to(np.tile(P[None], (S, 1, 1, 1))), verts=to(verts), truth=to(t))


def torch_evaluation(a):
    """One evaluation at the start, batched: cost [n], A [n, 3, 3], g [n, 3]."""
    P = a["proj"][a["scene"].long()]                                          # [n, C, 3, 4]
    X = a["verts"] @ a["pose"][:, :3, :3].transpose(-1, -2) + a["pose"][:, None, :3, 3]    # [n, V, 3]
    h = torch.einsum("ncij,nvj->ncvi", P[..., :3], X) + P[:, :, None, :, 3]
    uv = h[..., :2] / h[..., 2:3]                                             # [n, C, V, 2]
    lo, ilo = uv.min(dim=2)
    hi, ihi = uv.max(dim=2)
    p = torch.cat([lo, hi], -1)                                               # umin vmin umax vmax
    h2 = torch.gather(h[..., 2], 2, torch.cat([ilo, ihi], -1))
    r = p - a["boxes"].double()
    rows = P[:, :, [0, 1, 0, 1], :3]                                          # [n, C, 4, 3]
    J = (rows - p[..., None] * P[:, :, 2:3, :3]) / h2[..., None]
    J, r = J.reshape(n, -1, 3), r.reshape(n, -1)
    return (r * r).sum(-1), J.transpose(-1, -2) @ J, (J * r[..., None]).sum(1)


res = {"rows": n, "cams": C}
for V in (64, 1024):
    a = inputs(V)
    fit = ops_views.fit_boxes(a["pose"], a["scene"], a["views"], a["boxes"], a["proj"], C, a["verts"])
    info = fit.info.cpu().numpy()
    evals = float(info[:, 1].mean()) + 2.0             # the start, the trials, and the one at the result
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    outs = [e((n, 4, 4), torch.float64), e((n, 2), torch.float64), e((n, 2), torch.int32), e((n, 6), torch.float64),
            e((n, C, 4), torch.float64)]
    args = [a[k] for k in ("pose", "scene", "views", "boxes", "proj", "verts")]
    ms, runs = timed(lambda: torch.ops.mvmatch_views.fit_boxes_out(*args, C, 0, 10, *outs))
    ms_bare, _ = timed(lambda: torch.ops.mvmatch_views.fit_boxes_out(*args, C, 0, 10, *outs[:3], None, None))
    t_ms, t_runs = timed(lambda: torch_evaluation(a))
    before = (a["pose"][:, :3, 3] - a["truth"]).norm(dim=1).mean().item()
    after = (fit.pose[:, :3, 3] - a["truth"]).norm(dim=1).mean().item()
    res[f"V{V}"] = dict(ms=round(ms, 4), runs=runs, rows_per_s=round(n / ms * 1e3), ms_no_cov_resid=round(ms_bare, 4),
                        mean_evaluations=round(evals, 3), status=np.bincount(info[:, 0], minlength=4).tolist(),
                        torch_one_evaluation_ms=round(t_ms, 4), torch_runs=t_runs,
                        torch_times_evaluations_ms=round(t_ms * evals, 3),
                        t_err_mm_before=round(before, 3), t_err_mm_after=round(after, 3))
print(json.dumps(res))
