"""Rank-sharded matching of four-camera captures: gather_tables on fabricated
C = 4 host tables over gloo (CPU), the ranks' agreement on the field set, and
match_captures_sharded(n_cams=4) with 2 ranks sharing the one GPU against the
single-process table."""
import os
import signal
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("scene", "match", "cost", "X", "boxes", "centroids", "views", "n_views", "ext_cost", "reproj")
C = 4


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
def _fabricated(counts, seed, n_cams=C):
    """A host MatchTable of len(counts) captures of ``n_cams`` cameras with
    counts[s] rows each, scene ids from 0, every other value random (NaN and
    -1 in the slots of views a row did not keep, as the kernel leaves them)."""
    from bpc_baseline_amd.inference.batch_match import MatchTable
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    offs = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    views = rng.integers(0, 99, (n, n_cams)).astype(np.int32)
    views[:, 3:][rng.random((n, n_cams - 3)) < 0.5] = -1
    keep = views >= 0
    t = torch.from_numpy
    return MatchTable(
        scene=t(np.repeat(np.arange(counts.size), counts).astype(np.int32)),
        match=t(views[:, :3].copy()), cost=t(rng.uniform(0, 30, n).astype(np.float32)),
        X=t(rng.normal(size=(n, 3))),
        boxes=t(np.where(keep[..., None], rng.integers(0, 2000, (n, n_cams, 4)), -1).astype(np.int32)),
        centroids=t(np.where(keep[..., None], rng.integers(0, 4000, (n, n_cams, 2)) * 0.5, np.nan)),
        offs=offs, views=t(views), n_views=t(keep.sum(axis=1).astype(np.int32)),
        ext_cost=t(np.where(keep[:, 3:], rng.uniform(0, 30, (n, n_cams - 3)), np.inf).astype(np.float32)),
        reproj=t(np.where(keep, rng.uniform(0, 3, (n, n_cams)), np.nan)), n_cams=n_cams)


def _layout(world, variant):
    """Per-rank per-capture row counts.  "uneven": one rank whose captures
    have no rows; "few": 2 captures over the ranks (``shard_range``), so from
    world 3 on some rank has no captures at all."""
    from bpc_baseline_amd.distributed import shard_range
    if variant == "uneven":
        return [[3, 0, 5][:1 + r % 3] if r != 1 else [0, 0] for r in range(world)]
    return [[0, 4][slice(*shard_range(2, r, world))] for r in range(world)]


def _gather_worker(rank, world, port, variant, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, REPO)
    from bpc_baseline_amd.distributed import gather_tables, init_from_env
    from bpc_baseline_amd.inference.batch_match import MatchTable
    env = init_from_env(backend="gloo", use_gpu=False)
    if variant == "disagree":
        # rank 1 brings a three-camera table: every rank raises, none hangs
        tab = _fabricated([2], seed=rank) if rank != 1 else MatchTable.empty(torch.device("cpu"),
                                                                             np.zeros(2, np.int64))
        with pytest.raises(ValueError, match="n_cams"):
            gather_tables(env, tab, 1)
        open(os.path.join(out_dir, f"raised{rank}"), "w").close()
    else:
        counts = _layout(world, variant)[rank]
        if counts:
            tab = _fabricated(counts, seed=100 + rank)
        else:       # a rank without captures: the empty table of its own keywords
            tab = MatchTable.empty(torch.device("cpu"), n_cams=C, reproj=True)
        got = gather_tables(env, tab, len(counts))
        assert (got is not None) == env.is_root
        if env.is_root:
            assert got.n_cams == C and got.fields() == FIELDS
            for k in FIELDS:
                np.save(os.path.join(out_dir, k + ".npy"), getattr(got, k).numpy())
            np.save(os.path.join(out_dir, "offs.npy"), got.offs)
    env.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world,variant", [(2, "uneven"), (3, "uneven"), (2, "few"), (3, "few")])
def test_gather_view_tables_gloo(tmp_path, world, variant):
    """Rank 0's table is the concatenation of the ranks' C = 4 tables in rank
    order, every field bit-equal (the NaN / -1 slots included), scenes
    renumbered by each rank's first global capture, offs rebuilt."""
    layout = _layout(world, variant)
    assert any(sum(c) == 0 for c in layout)                       # a rank with no rows
    assert variant != "few" or world == 2 or any(len(c) == 0 for c in layout)   # ... with no captures
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
    assert np.array_equal(np.load(tmp_path / "scene.npy"), np.repeat(np.arange(all_counts.size), all_counts))


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_that_disagree_on_n_cams_all_raise(tmp_path, world):
    mp.spawn(_gather_worker, args=(world, _free_port(), "disagree", str(tmp_path)), nprocs=world, join=True)
    assert sorted(os.listdir(tmp_path)) == [f"raised{r}" for r in range(world)]


def test_fields_and_empty_shapes():
    """fields() lists what a table holds; FIELDS keeps its value; empty()
    gives the shapes of each kind of table."""
    from bpc_baseline_amd.distributed import DistEnv, gather_tables
    from bpc_baseline_amd.inference.batch_match import MatchTable
    assert MatchTable.FIELDS == ("scene", "match", "cost", "X", "boxes", "centroids")
    cpu = torch.device("cpu")
    e3, e3r, e5 = MatchTable.empty(cpu), MatchTable.empty(cpu, reproj=True), MatchTable.empty(cpu, n_cams=5)
    assert e3.fields() == MatchTable.FIELDS and e3.n_cams == 3 and e3.reproj is None
    assert e3r.fields() == e5.fields() == FIELDS
    assert tuple(e3r.views.shape) == (0, 3) and tuple(e3r.ext_cost.shape) == (0, 0)
    assert tuple(e5.boxes.shape) == (0, 5, 4) and tuple(e5.centroids.shape) == (0, 5, 2)
    assert tuple(e5.reproj.shape) == (0, 5) and tuple(e5.ext_cost.shape) == (0, 2) and e5.n_cams == 5
    tab = _fabricated([2, 0, 1], seed=1)
    assert tab.fields() == FIELDS
    env = DistEnv(0, 1, 0, cpu, False)
    assert gather_tables(env, tab, 3) is tab                     # no process group: the table itself
    # predictions / reprojection mask the row on views >= 0
    h = tab.host()
    pred, rep = tab.predictions(0), tab.reprojection(0)
    assert len(pred) == len(rep) == 2
    for r, ((b, c, X, cams), q) in enumerate(zip(pred, rep)):
        assert np.array_equal(cams, np.nonzero(h["views"][r] >= 0)[0]) and len(cams) == h["n_views"][r]
        assert b.shape == (len(cams), 4) and (b >= 0).all() and not np.isnan(c).any()
        assert np.array_equal(q, h["reproj"][r][cams]) and np.array_equal(X, h["X"][r])


def test_sharded_validates_img_offs_against_n_cams():
    from bpc_baseline_amd.distributed import DistEnv, match_captures_sharded
    env = DistEnv(0, 1, 0, torch.device("cpu"), False)
    z = torch.zeros(0)
    with pytest.raises(ValueError, match="4 images per capture"):
        match_captures_sharded(env, z, z, z, torch.zeros(7, dtype=torch.int64), None, None, n_cams=4)
    with pytest.raises(ValueError, match="n_cams"):
        match_captures_sharded(env, z, z, z, torch.zeros(7, dtype=torch.int64), None, None, n_cams=9)
    # no captures: the empty table of the keywords, without a device
    tab = match_captures_sharded(env, z, z, z, torch.zeros(1, dtype=torch.int64), None, None, n_cams=4)
    assert tab.n_cams == 4 and tab.fields() == FIELDS and tab.offs.tolist() == [0]
    tab = match_captures_sharded(env, z, z, z, torch.zeros(1, dtype=torch.int64), None, None, reproj=True)
    assert tab.n_cams == 3 and tab.fields() == FIELDS


# ---- match_captures_sharded(n_cams=4) on the GPU ----------------------------
def _run_ranks(world, out_dir, timeout=240):
    """One fresh child process per rank (gloo group, the one GPU shared), each
    under its own time limit; every exit status is checked, and on a failure
    the others are killed and nothing more is started."""
    env = dict(os.environ, MVM_DIST_BACKEND="gloo", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()))
    env.pop("MVM_DIST_FORCE", None)
    worker = os.path.join(REPO, "tests", "sharded_views_worker.py")
    procs = []
    try:
        for r in range(world):
            log = open(os.path.join(out_dir, f"rank{r}.log"), "w")
            procs.append(subprocess.Popen(["timeout", "-k", "10", str(timeout), sys.executable, worker,
                                           str(out_dir)],
                                          env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), cwd=REPO,
                                          stdout=log, stderr=subprocess.STDOUT, start_new_session=True))
        for r, p in enumerate(procs):
            rc = p.wait(timeout=timeout + 20)
            if rc != 0:
                with open(os.path.join(out_dir, f"rank{r}.log")) as fh:
                    raise AssertionError(f"rank {r} of {world}: exit status {rc}\n{fh.read()[-3000:]}")
    finally:
        for p in procs:
            if p.poll() is None:
                os.killpg(p.pid, signal.SIGKILL)     # the time limit's process and the rank under it
                p.wait()


@pytest.mark.gpu
def test_sharded_four_camera_match_equals_single_process(tmp_path, cuda):
    """7 four-camera captures (an empty extra view, one capture without a
    match) over 2 ranks (4 + 3): rank 0's gathered table equals the
    single-process table(reproj=True) bit for bit, reproj included (the same kernels on
    the same per-capture inputs)."""
    from bpc_baseline_amd.inference.batch_match import match_captures
    from sharded_views_worker import N_CAMS, N_CAPTURES, captures, to_device
    tab = match_captures(*to_device(captures(), cuda), n_cams=N_CAMS).table(reproj=True)
    single = dict(tab.host(), offs=tab.offs)
    assert tab.fields() == FIELDS and tab.offs.size == N_CAPTURES + 1
    assert tab.offs[-1] > 2 * N_CAPTURES and (np.diff(tab.offs) == 0).any()
    assert (single["n_views"] > 3).any() and (single["n_views"] == 3).any()
    _run_ranks(2, str(tmp_path))                 # 3 processes hold the GPU at once, this one included
    for k in FIELDS + ("offs",):
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == single[k].dtype and got.shape == single[k].shape, k
        assert np.array_equal(_bits(got), _bits(single[k])), k
