"""One rank of tests/test_sharded_views.py's GPU test, and the captures it
shares with the single-process reference.

    RANK=r WORLD_SIZE=w MASTER_ADDR=.. MASTER_PORT=.. MVM_DIST_BACKEND=gloo \
        python tests/sharded_views_worker.py OUT_DIR

Each rank builds the same four-camera captures, keeps its ``shard_range`` of
them, runs ``match_captures_sharded(n_cams=4)`` and rank 0 saves the gathered
table to OUT_DIR as one .npy per field.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N_CAMS, N_CAPTURES = 4, 7


def captures():
    """The first seven captures of tests/test_extend_gpu.py's four-camera
    fixture (capture 2 has an empty extra view, capture 5 no match).
    -> dict(boxes, conf, cls, img_offs, Ks, RTs) of host arrays."""
    import test_extend_gpu as TE
    f = TE.fixture(N_CAMS)
    end = int(f.img_offs[N_CAMS * N_CAPTURES])
    return dict(boxes=f.boxes[:end], conf=f.conf[:end], cls=f.cls[:end],
                img_offs=f.img_offs[:N_CAMS * N_CAPTURES + 1], Ks=f.Ks[:N_CAPTURES], RTs=f.RTs[:N_CAPTURES])


def capture_range(c, a, b):
    """Captures [a, b) of a ``captures`` dict (its own img_offs from 0)."""
    o = c["img_offs"]
    lo, hi = int(o[N_CAMS * a]), int(o[N_CAMS * b])
    return dict(boxes=c["boxes"][lo:hi], conf=c["conf"][lo:hi], cls=c["cls"][lo:hi],
                img_offs=o[N_CAMS * a:N_CAMS * b + 1] - lo, Ks=c["Ks"][a:b], RTs=c["RTs"][a:b])


def to_device(c, dev):
    """-> the positional arguments of match_captures."""
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t(c["boxes"]), t(c["conf"]), t(c["cls"]), t(c["img_offs"]), c["Ks"], c["RTs"]


def main(out_dir):
    import torch
    from bpc_baseline_amd.distributed import init_from_env, match_captures_sharded, shard_range
    env = init_from_env()
    a, b = shard_range(N_CAPTURES, env.rank, env.world)
    shard = capture_range(captures(), a, b)
    table = match_captures_sharded(env, *to_device(shard, env.device), n_cams=N_CAMS)
    assert (table is not None) == env.is_root
    if env.is_root:
        assert table.n_cams == N_CAMS
        for k in table.fields():
            np.save(os.path.join(out_dir, k + ".npy"), getattr(table, k).cpu().numpy())
        np.save(os.path.join(out_dir, "offs.npy"), table.offs)
    env.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
