"""Host side of the extension into extra cameras: the pair
list, the batched host F over it, and the n_cams validation -- no GPU."""
import numpy as np
import pytest
import torch

from bpc_baseline_amd.inference import batch_match
from bpc_baseline_amd.inference.batch_match import extension_pairs, match_captures
from bpc_baseline_amd.inference.utils.camera_utils import (compute_fundamental_matrix,
                                                           fundamental_matrices_batched)
from bpc_baseline_amd.synth import make_rig


@pytest.mark.parametrize("C", range(3, 9))
def test_extension_pairs(C):
    p = extension_pairs(C)
    assert p.dtype == np.int32 and p.shape == (3 + 3 * (C - 3), 2)
    want = [(0, 1), (0, 2), (1, 2)]
    for d in range(3, C):
        want += [(0, d), (1, d), (2, d)]
    assert p.tolist() == [list(w) for w in want]


@pytest.mark.parametrize("C", (2, 9, 0, -1))
def test_extension_pairs_range(C):
    with pytest.raises(ValueError):
        extension_pairs(C)


@pytest.mark.parametrize("C", range(3, 9))
def test_batched_host_F_equals_per_pair(C):
    rng = np.random.default_rng(40 + C)
    rigs = [make_rig(rng, C) for _ in range(3)]
    Ks = np.stack([np.stack(k) for k, _ in rigs])
    RTs = np.stack([np.stack(r) for _, r in rigs])
    pairs = extension_pairs(C)
    F = fundamental_matrices_batched(Ks, RTs, pairs).reshape(3, len(pairs), 9)
    for s in range(3):
        for p, (a, b) in enumerate(pairs):
            ref = compute_fundamental_matrix(Ks[s, a], RTs[s, a, :3, :3], RTs[s, a, :3, 3],
                                             Ks[s, b], RTs[s, b, :3, :3], RTs[s, b, :3, 3])
            assert np.array_equal(np.asarray(ref, np.float64).reshape(9).view(np.uint64),
                                  F[s, p].view(np.uint64)), (s, a, b)
    Fh, Ph = batch_match._host_rig(Ks, RTs, C)
    assert np.array_equal(Fh.view(np.uint64), F.reshape(-1, 9).view(np.uint64))
    assert Ph.shape == (3, C, 3, 4)


@pytest.mark.parametrize("C", (2, 9, 0, -3))
def test_n_cams_out_of_range_raises_before_any_device_call(C, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device call before the n_cams check")
    monkeypatch.setattr(batch_match.ops, "pack_detections", boom)
    monkeypatch.setattr(batch_match.ops, "rig_matrices", boom)
    e = torch.zeros(0)
    with pytest.raises(ValueError, match="n_cams"):
        match_captures(e.reshape(0, 4), e, e, torch.zeros(1, dtype=torch.int64), np.zeros((0, 3, 3, 3)),
                       np.zeros((0, 3, 4, 4)), n_cams=C)


def test_table_of_a_wide_batch_is_not_implemented():
    z = np.zeros(1, np.int64)
    b = batch_match.MatchBatch(match=torch.zeros((0, 3), dtype=torch.int32), cost=torch.zeros(0),
                               X=torch.zeros((0, 3), dtype=torch.float64), count=np.zeros(0, np.int32),
                               offs=z, pts=torch.zeros((0, 2), dtype=torch.float64),
                               boxes=torch.zeros((0, 4), dtype=torch.int32), cam_offs=z, n_cams=4)
    with pytest.raises(NotImplementedError):
        b.table()
