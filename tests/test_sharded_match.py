"""Rank-sharded capture matching: gather_tables on fabricated host tables over
gloo (CPU), and match_captures_sharded with 2 and 3 ranks sharing the one GPU
against the single-process table and the CPU oracle chain."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("scene", "match", "cost", "X", "boxes", "centroids")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ---- gather_tables on host tables -------------------------------------------
def _fabricated(counts, seed):
    """A host MatchTable of len(counts) captures with counts[s] rows each,
    scene ids from 0, every other value random."""
    from bpc_baseline_amd.inference.batch_match import MatchTable
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    offs = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    t = torch.from_numpy
    return MatchTable(scene=t(np.repeat(np.arange(counts.size), counts).astype(np.int32)),
                      match=t(rng.integers(0, 99, (n, 3)).astype(np.int32)),
                      cost=t(rng.uniform(0, 30, n).astype(np.float32)), X=t(rng.normal(size=(n, 3))),
                      boxes=t(rng.integers(0, 2000, (n, 3, 4)).astype(np.int32)),
                      centroids=t(rng.integers(0, 4000, (n, 3, 2)) * 0.5), offs=offs)


def _layout(world, variant):
    """Per-rank per-capture row counts.  "uneven": one rank whose captures
    have no rows; "few": 2 captures over the ranks (``shard_range``), so from
    world 3 on some rank has no captures at all; "none": no rank has a row."""
    from bpc_baseline_amd.distributed import shard_range
    if variant == "uneven":
        return [[3, 0, 5][:1 + r % 3] if r != 1 else [0, 0] for r in range(world)]
    per = [0, 4] if variant == "few" else [0, 0]
    return [per[slice(*shard_range(2, r, world))] for r in range(world)]


def _gather_worker(rank, world, port, variant, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, REPO)
    from bpc_baseline_amd.distributed import gather_tables, init_from_env
    env = init_from_env(backend="gloo", use_gpu=False)
    counts = _layout(world, variant)[rank]
    got = gather_tables(env, _fabricated(counts, seed=100 + rank), len(counts))
    assert (got is not None) == env.is_root
    if env.is_root:
        for k in FIELDS:
            np.save(os.path.join(out_dir, k + ".npy"), getattr(got, k).numpy())
        np.save(os.path.join(out_dir, "offs.npy"), got.offs)
    env.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world,variant", [(2, "uneven"), (3, "uneven"), (4, "uneven"), (2, "few"),
                                           (3, "few"), (4, "few"), (2, "none")])
def test_gather_tables_gloo(tmp_path, world, variant):
    """Rank 0's table is the concatenation of the ranks' tables in rank order,
    scenes renumbered by each rank's first global capture, offs rebuilt."""
    layout = _layout(world, variant)
    assert any(sum(c) == 0 for c in layout)                       # a rank with no rows
    assert variant != "few" or world == 2 or any(len(c) == 0 for c in layout)
    mp.spawn(_gather_worker, args=(world, _free_port(), variant, str(tmp_path)), nprocs=world, join=True)
    parts = [_fabricated(c, seed=100 + r) for r, c in enumerate(layout)]
    first = np.cumsum([0] + [len(c) for c in layout])
    for k in FIELDS:
        ref = [getattr(p, k).numpy() for p in parts]
        if k == "scene":
            ref = [a + np.int32(first[r]) for r, a in enumerate(ref)]
        ref = np.concatenate(ref)
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == ref.dtype and got.shape == ref.shape, k
        assert np.array_equal(_bits(got), _bits(ref)), k
    all_counts = np.concatenate([np.asarray(c, np.int64) for c in layout])
    offs = np.load(tmp_path / "offs.npy")
    assert offs.dtype == np.int64 and offs[0] == 0 and np.array_equal(np.diff(offs), all_counts)
    assert np.array_equal(np.load(tmp_path / "scene.npy"),
                          np.repeat(np.arange(all_counts.size), all_counts))


def test_gather_tables_without_a_group():
    """No process group: the table itself."""
    from bpc_baseline_amd.distributed import DistEnv, gather_tables
    env = DistEnv(0, 1, 0, torch.device("cpu"), False)
    tab = _fabricated([2, 0, 1], seed=1)
    assert gather_tables(env, tab, 3) is tab
    with pytest.raises(ValueError):
        gather_tables(env, tab, 2)


# ---- match_captures_sharded on the GPU --------------------------------------
@pytest.fixture(scope="module")
def single(cuda):
    """The seven captures in one process: the table every sharded run must
    reproduce, computed once."""
    from bpc_baseline_amd.inference.batch_match import match_captures
    from sharded_match_worker import CONF_THRESH, MATCH_THRESH, mixed_captures, to_device
    tab = match_captures(*to_device(mixed_captures(), cuda), conf_thresh=CONF_THRESH,
                         matching_threshold=MATCH_THRESH).table()
    return dict(tab.host(), offs=tab.offs)


@pytest.fixture(scope="module")
def oracle_chain():
    """Per capture, on the CPU restatements: packing, F, oracle.cube ->
    oracle.lsap -> pipeline.select_sort -> pipeline.triangulate.
    -> list of (match int32 [k, 3], cost f32 [k], X f64 [k, 3])."""
    from bpc_baseline_amd.inference.utils.camera_utils import camera_pairs, fundamental_matrices
    from oracle import lsap, pipeline
    from oracle import oracle as cube_oracle
    from sharded_match_worker import CONF_THRESH, MATCH_THRESH, SIZES, capture_range, mixed_captures
    full, out = mixed_captures(), []
    for s in range(len(SIZES)):
        c = capture_range(full, s, s + 1)
        K, RT = c["Ks"][0], c["RTs"][0]
        _, cent, o = pipeline.detect_pack(c["boxes"], c["conf"], c["cls"], c["img_offs"], CONF_THRESH)
        N, M, P = np.diff(o)
        if min(N, M, P) == 0:
            out.append((np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros((0, 3))))
            continue
        F = fundamental_matrices(list(K), list(RT), camera_pairs(3))
        cube = cube_oracle.cube(cent, o, F, 1)[0].reshape(-1)
        rr, rc = lsap.linear_sum_assignment(cube.reshape(N * M, P))
        m, cost = pipeline.select_sort(cube, M, P, rr, rc, MATCH_THRESH)
        proj = np.stack([K[v] @ RT[v][:3] for v in range(3)])
        X = pipeline.triangulate(np.repeat(proj[None], len(m), 0), cent[o[:3][None, :] + m])
        out.append((m, cost, X))
    return out


def _run_ranks(world, out_dir, timeout=240):
    """One fresh child process per rank (gloo group, the one GPU shared), each
    waited for with its own time limit; on a failure the others are killed
    and nothing more is started."""
    env = dict(os.environ, MVM_DIST_BACKEND="gloo", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()))
    env.pop("MVM_DIST_FORCE", None)
    worker = os.path.join(REPO, "tests", "sharded_match_worker.py")
    procs = []
    try:
        for r in range(world):
            log = open(os.path.join(out_dir, f"rank{r}.log"), "w")
            procs.append(subprocess.Popen([sys.executable, worker, str(out_dir)],
                                          env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), cwd=REPO,
                                          stdout=log, stderr=subprocess.STDOUT))
        for r, p in enumerate(procs):
            rc = p.wait(timeout=timeout)
            if rc != 0:
                with open(os.path.join(out_dir, f"rank{r}.log")) as fh:
                    raise AssertionError(f"rank {r} of {world}: exit status {rc}\n{fh.read()[-3000:]}")
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_match_equals_single_process_and_oracle(tmp_path, world, single, oracle_chain):
    """7 captures (8 / 24 / 64 detections per view, one without matches) over
    2 ranks (4 + 3) and 3 ranks (3 + 2 + 2).  Rank 0's gathered table equals
    the single-process table bit for bit, X included (the same kernels on the
    same per-capture inputs), and per capture the CPU oracle chain: matches,
    order and cost exactly, X within the DLT's bound (rtol 1e-10, atol 1e-9)."""
    from sharded_match_worker import NO_MATCHES, SIZES
    assert world + 1 <= 4                        # processes holding the GPU at once, this one included
    _run_ranks(world, str(tmp_path))
    got = {k: np.load(tmp_path / (k + ".npy")) for k in FIELDS + ("offs",)}
    for k in FIELDS + ("offs",):
        assert got[k].dtype == single[k].dtype and got[k].shape == single[k].shape, k
        assert np.array_equal(_bits(got[k]), _bits(single[k])), k
    offs = got["offs"]
    assert offs.size == len(SIZES) + 1 and offs[NO_MATCHES] == offs[NO_MATCHES + 1]
    assert offs[-1] > 2 * len(SIZES)             # the synthetic objects are recovered
    for s, (m, cost, X) in enumerate(oracle_chain):
        rows = slice(int(offs[s]), int(offs[s + 1]))
        assert (got["scene"][rows] == s).all()
        assert np.array_equal(got["match"][rows], m), s
        assert np.array_equal(_bits(got["cost"][rows]), _bits(cost)), s
        np.testing.assert_allclose(got["X"][rows], X, rtol=1e-10, atol=1e-9)
