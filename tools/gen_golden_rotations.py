"""Writes tests/golden/rot_decode.npz: raw rotation-head outputs and what the
reference's rotation step makes of them.

Run on a build machine that has the reference checked out:

    python tools/gen_golden_rotations.py --reference /path/to/reference

The reference's decoders (``bpc.pose.models.losses``) are imported and called
with a batch of 1, as its ``_estimate_rotation`` calls them; the wrap of the
Euler angles, the ``+ eps`` normalisation of the quaternion, the product with
the transposed extrinsic rotation and the 4 x 4 layout are applied here the way
that function applies them.  The file holds inputs and outputs only:

  rts           f64 [3, 4, 4]      ``synth.make_rig`` extrinsics
  <mode>_raw    float32 [n, D]     random vectors, then the edge rows
  <mode>_cam    int64 [n]          the camera whose extrinsics the row uses
  <mode>_rot    float32 [n, 3, 3]  the decoded matrix
  <mode>_world  f64 [n, 3, 3]      RT[:3, :3].T @ rot
  <mode>_n_edge int64              how many of the last rows are edge rows
  t / pose      f64 [n, 3] / [n, 4, 4]  (quat rows) the 4 x 4 layout
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 300


def edge_rows(mode):
    pi = np.pi
    if mode == "euler":
        rows = [(0, 0, 0), (pi / 2, 0, 0), (0, pi / 2, 0), (0, 0, pi / 2), (-pi / 2, pi / 2, -pi / 2),
                (pi, 0, 0), (-pi, 0, 0), (0, pi, -pi), (pi / 2, pi / 2, pi / 2)]
        for turns in (1, 3, 7, -2, -5):
            rows += [(2 * pi * turns + 0.3, -2 * pi * turns - 1.1, 2 * pi * turns + 2.9)]
        one = np.float32(pi)
        lo, hi = np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(4))
        rows += [(lo, hi, -lo), (-hi, lo, hi), (3 * pi, -3 * pi, 5 * pi), (1e-30, -1e-30, 1e-7)]
    elif mode == "quat":
        h = np.sqrt(0.5)
        rows = [(0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (h, 0, 0, h), (0, h, 0, h), (0, 0, h, h),
                (0.5, 0.5, 0.5, 0.5), (0.2, -0.4, 1.3, 2.0), (-0.2, 0.4, -1.3, -2.0), (300, -400, 1200, 0),
                (1e-6, 2e-6, -3e-6, 1e-6), (1e-20, 0, 0, 1e-20), (0, 0, 0, 0)]
    else:
        rows = [(1, 0, 0, 0, 1, 0), (0, 1, 0, -1, 0, 0), (0, 0, 1, 0, 1, 0), (1, 0, 0, 0, 0, 1),
                (2, 0, 0, 0, 0, -5), (1, 2, 3, 1, 2, 3.001), (1, 2, 3, 1.0001, 2, 3), (1, 1, 1, -1, -1, -1.01),
                (1e-3, 2e-3, -1e-3, 5, 4, 3), (100, 200, -50, 0.1, 0.2, 0.3)]
    return np.asarray(rows, np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="the reference's checkout (the directory that holds bpc/)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "rot_decode.npz"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, args.reference)
    import torch
    from bpc.pose.models import losses as L
    from bpc_baseline_amd.synth import make_rig

    rng = np.random.default_rng(319)
    _, RTs = make_rig(rng, 3)
    rts = np.stack(RTs).astype(np.float64)
    out = {"rts": rts}
    for mode, D in (("euler", 3), ("quat", 4), ("6d", 6)):
        rand = rng.uniform(-6 * np.pi, 6 * np.pi, (N_RANDOM, 3)) if mode == "euler" else rng.standard_normal((N_RANDOM, D))
        edge = edge_rows(mode)
        raw = np.concatenate([rand.astype(np.float32), edge])
        cam = np.arange(len(raw)) % 3
        rot = np.empty((len(raw), 3, 3), np.float32)
        world = np.empty((len(raw), 3, 3), np.float64)
        for i, raw_pred in enumerate(raw):
            with torch.no_grad():
                if mode == "euler":
                    wrapped = np.mod(raw_pred + np.pi, 2 * np.pi) - np.pi      # float32 throughout
                    m = L.rotmat_from_euler(torch.tensor(wrapped, dtype=torch.float32).unsqueeze(0))
                elif mode == "quat":
                    q = torch.tensor(raw_pred, dtype=torch.float32).unsqueeze(0)
                    length = q.norm(dim=1, keepdim=True)
                    q = q / (length + 1e-8)
                    m = L.quat_to_rotmat(q)
                else:
                    m = L.rotmat_from_6d(torch.tensor(raw_pred, dtype=torch.float32).unsqueeze(0))
            rot[i] = m.squeeze(0).numpy()
            with np.errstate(all="ignore"):
                world[i] = rts[cam[i]][:3, :3].T @ rot[i]
        out.update({f"{mode}_raw": raw, f"{mode}_cam": cam, f"{mode}_rot": rot, f"{mode}_world": world,
                    f"{mode}_n_edge": np.int64(len(edge))})
    n = len(out["quat_raw"])
    t = rng.uniform(-300, 300, (n, 3))
    pose = np.tile(np.eye(4), (n, 1, 1))
    pose[:, :3, :3] = out["quat_world"]
    pose[:, :3, 3] = t
    out.update(t=t, pose=pose)
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
