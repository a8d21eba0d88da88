"""The mean under symmetries on the GPU (mvm_fuse_rotations_sym,
ops_views.fuse_rotations_sym) against tests/pose_sym_model.py.

The op writes into slices of sentinel-filled outputs with a guard row on either
side; every output is compared whole and bit for bit with the model (NaN equal
to NaN; a zero of either sign is the same number), the guards with the
sentinel, and the inputs with what was uploaded."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import pose_edges as E
import pose_sym_edges as SE
import pose_sym_model as M
from bpc_baseline_amd import ops_views       # registers torch.ops.mvmatch_views.*
from test_crop_gpu import _graph_shape
from test_pose_gpu import SENT_F, SENT_I, case

pytestmark = pytest.mark.gpu
OUTS = (("rot_views", (3, 3), torch.float64, True), ("R", (3, 3), torch.float64, False),
        ("pose", (4, 4), torch.float64, False), ("spread", (), torch.float64, True),
        ("slot_status", (), torch.int32, True), ("row_status", (), torch.int32, False),
        ("sym_index", (), torch.int32, True), ("sym_margin", (), torch.float64, True),
        ("n_changed", (), torch.int32, False))
OPTIONAL = ("rot_views", "spread", "sym_margin", "n_changed")


@lru_cache(maxsize=None)
def group(K):
    """K symmetry transforms: the identity, the z folds, the cube group, and
    for 64 and 1,024 a discretised turn about z."""
    if K == 24:
        return M.with_blocks(E.cube_group())
    return M.z_fold(K)


def run_op(c, dev, rows, cams, syms, rounds=2, omit=()):
    b, e = rows
    m, K = e - b, len(cams)
    raw = torch.from_numpy(np.ascontiguousarray(c.raw[b:e][:, list(cams)])).to(dev)
    args = c.device(dev) + (torch.from_numpy(np.ascontiguousarray(syms)).to(dev),)
    keep = [a.clone() for a in (raw,) + args]
    bufs = {}
    for name, tail, dt, per_slot in OUTS:
        shape = (m + 2,) + ((K,) if per_slot else ()) + tail
        bufs[name] = torch.full(shape, SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=dev)
    out = {k: (None if k in omit else v[1:m + 1]) for k, v in bufs.items()}
    torch.ops.mvmatch_views.fuse_rotations_sym_out(raw, *args, c.C, c.scene_base, b, m, list(cams), c.mode, rounds,
                                                   *(out[k] for k, *_ in OUTS))
    torch.cuda.synchronize(dev)
    for got, was in zip((raw,) + args, keep):
        assert bool(((got == was) | ((got != got) & (was != was))).all())     # NaN stays NaN
    for name, _, dt, _ in OUTS:
        sent = SENT_I if dt == torch.int32 else SENT_F
        assert (bufs[name][0] == sent).all() and (bufs[name][-1] == sent).all(), name
        if name in omit:
            assert (bufs[name] == sent).all(), name
    return {k: v[1:m + 1].cpu().numpy() for k, v in bufs.items() if k not in omit}


# every case(n, C, "euler") below, SE.GPU_SIZES apart, is listed in SE.EULER_CASES: tests/test_pose_sym_model.py
# checks the share euler_filter drops for exactly those draws
def check(c, dev, rows, cams, syms, rounds=2, omit=()):
    b, e = rows
    got = run_op(c, dev, rows, cams, syms, rounds, omit)
    want = M.fuse_rotations_sym(c.raw[b:e][:, list(cams)], c.scene, c.views, c.X, c.RTs, c.mode, syms, rows=rows,
                                cams=list(cams), rounds=rounds, scene_base=c.scene_base)
    for k, v in got.items():
        assert M.same(v, want[k]), (k, np.argwhere(~((v == want[k]) | ((v != v) & (want[k] != want[k]))))[:5])
    M.invariants(got)
    return want


@pytest.mark.parametrize("mode", ("euler", "quat", "6d"))
@pytest.mark.parametrize("n, C, K, rounds", SE.GPU_SIZES)
def test_rows_cameras_symmetries_rounds_and_modes(cuda, n, C, K, rounds, mode):
    want = check(case(n, C, mode), cuda, (0, n), range(C), group(K), rounds)
    if n >= 255:
        assert {0, M.NO_VIEW, M.NO_CAPTURE, M.DEGENERATE} <= set(want["slot_status"].reshape(-1))
        assert K == 1 or len(set(want["sym_index"].reshape(-1))) > 2


def test_no_rows(cuda):
    check(case(257, 4, "quat"), cuda, (0, 0), range(4), group(4))
    check(case(257, 4, "quat"), cuda, (9, 9), (2,), group(1))


def test_the_identity_alone_gives_the_plain_kernel(cuda):
    """Every output shared with fuse="mean", as numbers, from the existing kernel."""
    from test_pose_gpu import run_op as run_plain
    for mode in M.P.MODES:
        c = case(257, 4, mode)
        plain = run_plain(c, cuda, (0, c.n), range(4), "mean")
        for rounds in (1, 2):
            got = run_op(c, cuda, (0, c.n), range(4), group(1), rounds)
            for k in plain:
                assert M.same(got[k], plain[k]), (mode, k)


def test_scene_base(cuda):
    c = case(257, 4, "quat", scene_base=7)
    want = check(c, cuda, (0, c.n), range(4), group(4))
    for r in c.bad[:2]:                                               # ids outside on either side
        assert (want["slot_status"][r] == M.NO_CAPTURE).all() and want["row_status"][r] == M.NO_ROTATION


@pytest.mark.parametrize("cams", ((2,), (0, 2), (3, 0, 2, 1), (2, 1, 1, 2)))
def test_camera_subsets_and_orders(cuda, cams):
    for mode in M.P.MODES:
        check(case(257, 4, mode), cuda, (1, 200), cams, group(4))
    check(case(513, 5, "6d"), cuda, (0, 513), (4, 1, 3), group(24), 4)


@pytest.mark.parametrize("rows", ((0, 1), (4, 9), (256, 257), (250, 513)))
def test_row_ranges(cuda, rows):
    check(case(513, 5, "6d"), cuda, rows, range(5), group(24))


@pytest.mark.parametrize("omit", (("sym_margin",), ("n_changed",), ("rot_views",), ("spread",), OPTIONAL))
def test_optional_outputs(cuda, omit):
    check(case(257, 4, "euler"), cuda, (0, 257), range(4), group(4), omit=omit)
    check(case(257, 4, "quat"), cuda, (3, 40), (1, 2), group(2), 1, omit=omit)


@pytest.mark.parametrize("name", sorted(SE.families()))
def test_edge_families(cuda, name):
    t, syms = SE.families()[name]
    for rounds in (1, 2, 3):
        want = check(t, cuda, (0, t.n), range(t.C), syms, rounds)
    if name == "round_two":
        assert (want["n_changed"] == 0).all() and (check(t, cuda, (0, t.n), range(4), syms, 2)["n_changed"] == 1).all()
    if name == "lost_reference":
        check(t, cuda, (0, t.n), (4, 0, 3, 2), syms)


def test_op_captures_into_a_graph(cuda):
    """One kernel node and no edge; the replay gives the eager bytes."""
    c, syms = case(257, 4, "6d"), group(24)
    eager = run_op(c, cuda, (0, c.n), (0, 2, 3), syms)
    raw = torch.from_numpy(np.ascontiguousarray(c.raw[:, [0, 2, 3]])).to(cuda)
    args = c.device(cuda) + (torch.from_numpy(syms).to(cuda),)
    out = {}
    for name, tail, dt, per_slot in OUTS:
        shape = (c.n,) + ((3,) if per_slot else ()) + tail
        out[name] = torch.full(shape, SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=cuda)
    torch.cuda.synchronize(cuda)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        torch.ops.mvmatch_views.fuse_rotations_sym_out(raw, *args, 4, 0, 0, c.n, [0, 2, 3], "6d", 2,
                                                       *(out[k] for k, *_ in OUTS))
    assert all((v == (SENT_I if v.dtype == torch.int32 else SENT_F)).all() for v in out.values())   # captured, not run
    assert _graph_shape(g.raw_cuda_graph()) == (1, 0, 0)             # hipGraphNodeTypeKernel == 0
    g.replay()
    torch.cuda.synchronize(cuda)
    for k, v in out.items():
        assert M.same(v.cpu().numpy(), eager[k]), k


def test_the_wrapper_and_argument_errors(cuda):
    c, syms = case(257, 4, "quat"), group(4)
    scene, views, X, RTs = c.device(cuda)
    raw = torch.from_numpy(c.raw).to(cuda)
    f = ops_views.fuse_rotations_sym
    res = f(raw, scene, views, X, c.RTs, 4, "quat", syms)                        # host RTs and syms, two rounds
    want = M.fuse_rotations_sym(c.raw, c.scene, c.views, c.X, c.RTs, "quat", syms)
    for k, *_ in OUTS:
        assert M.same(getattr(res, k).cpu().numpy(), want[k]), k
    assert isinstance(res, ops_views.FusedRotations) and ops_views.SLOT_NO_SYM == M.NO_SYM
    res = f(raw[5:9, [3, 1]].contiguous(), scene, views, X, RTs, 4, "quat", torch.from_numpy(syms).to(cuda),
            rows=(5, 9), cams=(3, 1), rounds=1)
    want = M.fuse_rotations_sym(c.raw[5:9][:, [3, 1]], c.scene, c.views, c.X, c.RTs, "quat", syms, rows=(5, 9),
                                cams=[3, 1], rounds=1)
    for k, *_ in OUTS:
        assert M.same(getattr(res, k).cpu().numpy(), want[k]), k
    for bad in (dict(rounds=0), dict(rounds=5), dict(rounds=2.0), dict(rounds=True), dict(rows=(3, 2)),
                dict(rows=(0, c.n + 1)), dict(cams=()), dict(cams=(4,)), dict(rows=(0, 5))):
        with pytest.raises(ValueError):
            f(raw, scene, views, X, RTs, 4, "quat", syms, **bad)
    nan_syms = syms.copy()
    nan_syms[1, 0, 0] = np.nan
    for bad in (np.eye(4), syms[:0], syms[:, :3, :3], nan_syms):                 # host symmetries are checked
        with pytest.raises(ValueError, match="syms"):
            f(raw, scene, views, X, RTs, 4, "quat", bad)
    dsyms = torch.from_numpy(syms).to(cuda)
    for bad in (dsyms.float(), dsyms.cpu(), dsyms[:, :3]):
        with pytest.raises(ValueError, match="syms"):
            f(raw, scene, views, X, RTs, 4, "quat", bad)
    for mode in ("euler", "6d", "matrix"):
        with pytest.raises(ValueError):
            f(raw, scene, views, X, RTs, 4, mode, syms)
    # the op's own rows: the outputs
    op = torch.ops.mvmatch_views.fuse_rotations_sym_out
    e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=cuda)
    good = dict(rot_views=e((2, 4, 3, 3)), R=e((2, 3, 3)), pose=e((2, 4, 4)), spread=e((2, 4)),
                slot_status=e((2, 4), torch.int32), row_status=e(2, torch.int32), sym_index=e((2, 4), torch.int32),
                sym_margin=e((2, 4)), n_changed=e(2, torch.int32))
    call = lambda rounds=2, **kw: op(raw[:2].contiguous(), scene, views, X, RTs, dsyms, 4, 0, 0, 2, [0, 1, 2, 3],
                                     "quat", rounds, *(dict(good, **kw)[k] for k, *_ in OUTS))
    call()
    for name in good:
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name][:1]})
    with pytest.raises(ValueError, match="sym_index"):
        call(sym_index=good["sym_index"].to(torch.int64))
    with pytest.raises(ValueError, match="rounds"):
        call(rounds=5)
