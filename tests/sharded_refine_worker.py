"""One rank of tests/test_sharded_refine.py's GPU test.

    RANK=r WORLD_SIZE=w MASTER_ADDR=.. MASTER_PORT=.. MVM_DIST_BACKEND=gloo \
        python tests/sharded_refine_worker.py OUT_DIR

Each rank builds the seven four-camera captures of
tests/sharded_prune_worker.py, keeps its ``shard_range`` of them, runs
``match_captures_sharded(n_cams=4, reproj_gate=GATE, refine=True)`` and rank 0
saves the gathered table to OUT_DIR as one .npy per field.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from sharded_prune_worker import GATE, captures  # noqa: E402
from sharded_views_worker import N_CAMS, N_CAPTURES, capture_range, to_device  # noqa: E402


def main(out_dir):
    import torch
    from bpc_baseline_amd.distributed import init_from_env, match_captures_sharded, shard_range
    env = init_from_env()
    a, b = shard_range(N_CAPTURES, env.rank, env.world)
    shard = capture_range(captures(), a, b)
    table = match_captures_sharded(env, *to_device(shard, env.device), n_cams=N_CAMS, reproj_gate=GATE,
                                   refine=True)
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
