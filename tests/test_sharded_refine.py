"""Rank-sharded matching with the point refinement: seven four-camera captures
over 2 gloo ranks sharing the one GPU,
``match_captures_sharded(n_cams=4, reproj_gate=3, refine=True)``, against the
single-process table."""
import os
import signal
import socket
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("scene", "match", "cost", "X", "boxes", "centroids", "views", "n_views", "ext_cost", "reproj")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _run_ranks(world, out_dir, timeout=240):
    """One fresh child process per rank (gloo group, the one GPU shared), each
    under its own time limit; every exit status is checked, and on a failure
    the others are killed and nothing more is started."""
    env = dict(os.environ, MVM_DIST_BACKEND="gloo", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()))
    env.pop("MVM_DIST_FORCE", None)
    worker = os.path.join(REPO, "tests", "sharded_refine_worker.py")
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
def test_sharded_refined_match_equals_single_process(tmp_path, cuda):
    """Rank 0's gathered table equals the single-process
    ``match_captures(reproj_gate=3, refine=True).table(reproj=True)`` bit for
    bit, and its X is the refined one (it differs from the unrefined table's)."""
    from bpc_baseline_amd.inference.batch_match import match_captures
    from sharded_prune_worker import GATE, captures
    from sharded_views_worker import N_CAMS, N_CAPTURES, to_device
    args = to_device(captures(), cuda)
    tab = match_captures(*args, n_cams=N_CAMS, reproj_gate=GATE, refine=True).table(reproj=True)
    dlt = match_captures(*args, n_cams=N_CAMS, reproj_gate=GATE).table(reproj=True)
    single = dict(tab.host(), offs=tab.offs)
    assert tab.fields() == FIELDS and tab.offs.size == N_CAPTURES + 1
    assert np.array_equal(tab.offs, dlt.offs)
    assert (_bits(single["X"]) != _bits(dlt.host()["X"])).any(axis=1).sum() >= 10
    _run_ranks(2, str(tmp_path))                 # 3 processes hold the GPU at once, this one included
    for k in FIELDS + ("offs",):
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == single[k].dtype and got.shape == single[k].shape, k
        assert np.array_equal(_bits(got), _bits(single[k])), k
