"""One rank of tests/test_sharded_match.py's GPU test, and the captures it and
tests/test_match_table_gpu.py share.

    RANK=r WORLD_SIZE=w MASTER_ADDR=.. MASTER_PORT=.. MVM_DIST_BACKEND=gloo \
        python tests/sharded_match_worker.py OUT_DIR

Each rank builds the same captures, keeps its ``shard_range`` of them, runs
``match_captures_sharded`` and rank 0 saves the gathered table to OUT_DIR as
one .npy per field.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# detections per view of the seven captures (64 x 64 >= 4096: the
# candidate-list class, so the batch is a mixed one); capture NO_MATCHES has
# its first view emptied, so nothing can match in it
SIZES = (8, 64, 24, 8, 24, 64, 8)
NO_MATCHES = 3
CONF_THRESH, MATCH_THRESH = 0.1, 30


def mixed_captures(sizes=SIZES, empty_first_view=NO_MATCHES, seed=40):
    """``make_detector_batch`` captures of ``sizes[i]`` detections per view,
    concatenated; the first view of capture ``empty_first_view`` gets
    confidences below every threshold, so the packer keeps none of it.
    -> dict(boxes, conf, cls, img_offs, Ks, RTs) of host arrays."""
    from bpc_baseline_amd.synth import make_detector_batch
    parts = [make_detector_batch(1, n, seed=seed, first_capture=i) for i, n in enumerate(sizes)]
    counts = np.concatenate([np.diff(p.img_offs) for p in parts])
    img_offs = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=img_offs[1:])
    conf = np.concatenate([p.conf for p in parts])
    if empty_first_view is not None:
        a, b = img_offs[3 * empty_first_view], img_offs[3 * empty_first_view + 1]
        conf[a:b] = 0.0
    return dict(boxes=np.concatenate([p.boxes for p in parts]), conf=conf,
                cls=np.concatenate([p.cls for p in parts]), img_offs=img_offs,
                Ks=np.concatenate([p.Ks for p in parts]), RTs=np.concatenate([p.RTs for p in parts]))


def capture_range(c, a, b):
    """Captures [a, b) of a ``mixed_captures`` dict (its own img_offs from 0)."""
    o = c["img_offs"]
    lo, hi = int(o[3 * a]), int(o[3 * b])
    return dict(boxes=c["boxes"][lo:hi], conf=c["conf"][lo:hi], cls=c["cls"][lo:hi],
                img_offs=o[3 * a:3 * b + 1] - lo, Ks=c["Ks"][a:b], RTs=c["RTs"][a:b])


def to_device(c, dev):
    """-> the positional arguments of match_captures."""
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t(c["boxes"]), t(c["conf"]), t(c["cls"]), t(c["img_offs"]), c["Ks"], c["RTs"]


def main(out_dir):
    import torch
    from bpc_baseline_amd.distributed import init_from_env, match_captures_sharded, shard_range
    from bpc_baseline_amd.inference.batch_match import MatchTable
    env = init_from_env()
    a, b = shard_range(len(SIZES), env.rank, env.world)
    shard = capture_range(mixed_captures(), a, b)
    table = match_captures_sharded(env, *to_device(shard, env.device), conf_thresh=CONF_THRESH,
                                   matching_threshold=MATCH_THRESH)
    assert (table is not None) == env.is_root
    if env.is_root:
        for k in MatchTable.FIELDS:
            np.save(os.path.join(out_dir, k + ".npy"), getattr(table, k).cpu().numpy())
        np.save(os.path.join(out_dir, "offs.npy"), table.offs)
    env.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
