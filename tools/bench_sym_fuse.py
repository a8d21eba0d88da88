"""Timing of the mean under symmetries: 1000 captures x 24 rows x 4
cameras, quaternions; the existing fuse="mean" stage, the new stage for K = 1, 8
and 64 at one and two rounds, and a batched torch statement of the same
algorithm, each a median of 5 with the host clock around the launch and one
synchronise.  Prints one JSON line.  Run from the repository root."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_sym_model as M                      # noqa: E402
from bpc_baseline_amd import ops_views          # noqa: E402
from bpc_baseline_amd.synth import make_rig     # noqa: E402

dev = torch.device("cuda", 0)
S, per, C = 1000, 24, 4
n = S * per
rng = np.random.default_rng(1)
raw = torch.from_numpy(rng.standard_normal((n, C, 4)).astype(np.float32)).to(dev)
scene = torch.from_numpy(np.repeat(np.arange(S), per).astype(np.int32)).to(dev)
views = torch.zeros((n, C), dtype=torch.int32, device=dev)
X = torch.from_numpy(rng.uniform(-300, 300, (n, 3))).to(dev)
rig = np.stack(make_rig(rng, C)[1]).astype(np.float64)
RTs = torch.from_numpy(np.tile(rig[None], (S, 1, 1, 1))).to(dev)


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


def torch_statement(syms, rounds=2):
    q = raw.double()
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    Mx = torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
                      2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
                      2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y], -1).reshape(n, C, 3, 3)
    W = RTs[scene.long(), :, :3, :3].transpose(-1, -2) @ Mx
    Sk = syms[:, :3, :3]
    ref = W[:, 0]
    for _ in range(rounds):
        B = ref.transpose(-1, -2)[:, None] @ W                       # [n, C, 3, 3]
        score = torch.einsum("ncij,kji->nck", B, Sk)
        Wp = W @ Sk[score.argmax(-1)]
        U, _, Vt = torch.linalg.svd(Wp.sum(1))
        d = torch.det(U @ Vt)
        ref = U @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1)) @ Vt
    return ref


res = {}
e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
outs = dict(rot_views=e((n, C, 3, 3), torch.float64), R=e((n, 3, 3), torch.float64), pose=e((n, 4, 4), torch.float64),
            spread=e((n, C), torch.float64), slot_status=e((n, C), torch.int32), row_status=e(n, torch.int32))
extra = dict(sym_index=e((n, C), torch.int32), sym_margin=e((n, C), torch.float64), n_changed=e(n, torch.int32))
plain = lambda: torch.ops.mvmatch_views.fuse_rotations_out(raw, scene, views, X, RTs, C, 0, 0, n, list(range(C)), "quat",
                                                           "mean", 2, *outs.values())
res["plain_mean_ms"] = timed(plain)
for K in (1, 8, 64):
    syms = torch.from_numpy(M.z_fold(K)).to(dev)
    for rounds in (1, 2):
        f = lambda: torch.ops.mvmatch_views.fuse_rotations_sym_out(raw, scene, views, X, RTs, syms, C, 0, 0, n,
                                                                   list(range(C)), "quat", rounds, *outs.values(),
                                                                   *extra.values())
        res[f"sym_K{K}_rounds{rounds}_ms"] = timed(f)
    res[f"torch_K{K}_rounds2_ms"] = timed(lambda: torch_statement(syms))
    if K == 8:
        f()
        got = outs["R"].clone()
        ref = torch_statement(syms)
        d = (got[:, None] - ref[:, None] @ syms[None, :, :3, :3]).abs().amax(dim=(-1, -2)).amin(dim=1)
        res["torch_vs_kernel_median_diff"] = float(d.median())
res["plain_mean_ms_again"] = timed(plain)
print(json.dumps(res))
