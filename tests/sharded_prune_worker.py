"""One rank of tests/test_sharded_prune.py's GPU test, and the captures it
shares with the single-process reference.

    RANK=r WORLD_SIZE=w MASTER_ADDR=.. MASTER_PORT=.. MVM_DIST_BACKEND=gloo \
        python tests/sharded_prune_worker.py OUT_DIR

Each rank builds the same four-camera captures (the seven of
tests/sharded_views_worker.py with extra-view detections moved by 6-12 px),
keeps its ``shard_range`` of them, runs
``match_captures_sharded(n_cams=4, reproj_gate=GATE)`` and rank 0 saves the
gathered table to OUT_DIR as one .npy per field.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from sharded_views_worker import N_CAMS, N_CAPTURES, capture_range, to_device  # noqa: E402

GATE = 3.0


def captures():
    """The first seven captures of tests/test_view_prune_gpu.py's shifted
    four-camera fixture -> dict(boxes, conf, cls, img_offs, Ks, RTs)."""
    import test_extend_gpu as TE
    import view_prune_model as M
    f = TE.fixture(N_CAMS)
    boxes = M.shift_extra_boxes(f, seed=900 + N_CAMS)
    end = int(f.img_offs[N_CAMS * N_CAPTURES])
    return dict(boxes=boxes[:end], conf=f.conf[:end], cls=f.cls[:end],
                img_offs=f.img_offs[:N_CAMS * N_CAPTURES + 1], Ks=f.Ks[:N_CAPTURES], RTs=f.RTs[:N_CAPTURES])


def main(out_dir):
    import torch
    from bpc_baseline_amd.distributed import init_from_env, match_captures_sharded, shard_range
    env = init_from_env()
    a, b = shard_range(N_CAPTURES, env.rank, env.world)
    shard = capture_range(captures(), a, b)
    table = match_captures_sharded(env, *to_device(shard, env.device), n_cams=N_CAMS, reproj_gate=GATE)
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
