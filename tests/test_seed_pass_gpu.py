"""match_captures(extra_seeds=[...]) end to end on the GPU, on
the captures of tests/test_seed_pass_model.py: the first pass is the call
without the keyword byte for byte, every later pass is the existing
match_captures(n_cams=C) run on a sub-batch the test builds on the host from
the earlier passes' views -- every field bit for bit, so the leftover kernels
are pinned through the whole path with no tolerance --, and table_all() is the
restatement's merge of the passes' tables."""
import numpy as np
import pytest
import torch

import seed_pass_model as M
from bpc_baseline_amd.inference.batch_match import match_capture_stream, match_captures

pytestmark = pytest.mark.gpu

BATCH_FIELDS = ("match", "cost", "X", "views", "ext_cost", "pts", "boxes", "proj")
HOST_FIELDS = ("count", "offs", "cam_offs")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _match(f, dev, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return match_captures(t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs, n_cams=f.C, **kw)


def _assert_same_batch(got, want, what):
    """Every field of two batches bit for bit over the captures' match rows
    (the rows behind a capture's count are not specified), the rest whole."""
    for k in HOST_FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k)
    rows = np.concatenate([np.arange(o, o + n) for o, n in zip(want.offs[:-1], want.count)] or
                          [np.zeros(0, np.int64)]).astype(np.int64)
    names = BATCH_FIELDS + (("pruned",) if want.pruned is not None else ())
    assert (got.pruned is None) == (want.pruned is None)
    for k in names:
        a, b = getattr(got, k).cpu().numpy(), getattr(want, k).cpu().numpy()
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        if k in ("pts", "boxes", "proj"):
            assert np.array_equal(_bits(a), _bits(b)), (what, k)
        else:
            assert np.array_equal(_bits(a[rows]), _bits(b[rows])), (what, k)


def _mark(used, f, batch, order=None, sub_offs=None, orig=None):
    M.mark_used(used, batch.views.cpu().numpy(), batch.offs, batch.count, f.img_offs, f.C, order, sub_offs,
                orig)


def _check_passes(f, res, seeds, dev, **kw):
    """Every later pass of ``res`` against match_captures on the host-built sub-batch."""
    assert len(res.passes) == len(seeds) and res.cam_order is None and res.orig is None
    used = np.zeros(len(f.cent), np.int32)
    _mark(used, f, res)
    subs = []
    for p, seed in zip(res.passes, seeds):
        order = M.seed_order(seed, f.C)
        g, orig, sub_offs = M.sub_captures(f, used, seed)
        assert p.cam_order == order and np.array_equal(p.orig.cpu().numpy(), orig)
        assert p.passes == () and p.n_cams == f.C
        want = _match(g, dev, **kw)
        _assert_same_batch(p, want, seed)
        _mark(used, f, p, order, sub_offs, orig)
        subs.append((order, orig, sub_offs))
    return subs


@pytest.mark.parametrize("gate", (None, 3.0))
@pytest.mark.parametrize("rig", ("host", "device"))
@pytest.mark.parametrize("C", (5, 6))
def test_extra_pass_is_the_path_on_the_leftovers(cuda, C, rig, gate):
    f = M.captures(C)
    kw = dict(rig=rig, reproj_gate=gate)
    plain = _match(f, cuda, **kw)
    none = _match(f, cuda, extra_seeds=None, **kw)
    res = _match(f, cuda, extra_seeds=[M.SEED], **kw)
    assert plain.passes == () and none.passes == ()
    _assert_same_batch(none, plain, "extra_seeds=None")
    _assert_same_batch(res, plain, "pass 0")
    (order, orig, sub_offs), = _check_passes(f, res, [M.SEED], cuda, **kw)
    # the extra pass finds the objects one of cameras 0-2 misses
    p1 = res.passes[0]
    assert int(p1.count.sum()) >= 6 and int(res.count.sum()) >= 8 * M.N_ALL

    # the merged table is the restatement's merge of the passes' own tables
    tabs = [b.table(reproj=True) for b in (res, p1)]
    hosts = [dict(t.host(), offs=t.offs) for t in tabs]
    want = M.merged_table(hosts, [None, order], [None, orig], [None, sub_offs], C)
    tab = res.table_all()
    assert tab.fields() == tabs[0].fields() + ("seed_pass",) and tab.n_cams == C
    got = dict(tab.host(), offs=tab.offs)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    zero = got["seed_pass"] == 0
    assert np.array_equal(got["views"][zero][:, :3], got["match"][zero])
    assert np.array_equal(got["views"][~zero][:, list(M.SEED)], got["match"][~zero])
    assert (~zero).sum() == p1.count.sum() and zero.sum() == res.count.sum()
    # a batch without extra passes: its own table, pass 0 in every row
    alone = plain.table_all()
    one = plain.table(reproj=True)
    assert not alone.seed_pass.any() and alone.seed_pass.dtype == torch.int32
    for k in one.fields():
        assert np.array_equal(_bits(alone.host()[k]), _bits(one.host()[k])), k


def test_pass_1_finds_the_seed_missed_objects_with_the_right_detections(cuda):
    f = M.captures(5)
    res = _match(f, cuda, extra_seeds=[M.SEED])
    tab = res.table_all().host()
    offs = res.table_all().offs
    for s in range(f.S):
        rows = tab["views"][int(offs[s]):int(offs[s + 1])]
        for o in f.missed[s]:
            want = np.array([(np.nonzero(f.ident[s][c] == o)[0].tolist() or [-1])[0] for c in range(f.C)])
            assert sum(np.array_equal(r, want) for r in rows) == 1, (s, rows, want)


@pytest.mark.parametrize("rig", ("host", "device"))
def test_two_extra_seeds_in_sequence(cuda, rig):
    """The second extra pass sees the first one's matches as used."""
    f = M.captures(5)
    seeds = [M.SEED, (1, 3, 4)]
    res = _match(f, cuda, rig=rig, extra_seeds=seeds, reproj_gate=3.0)
    _check_passes(f, res, seeds, cuda, rig=rig, reproj_gate=3.0)
    one = _match(f, cuda, rig=rig, extra_seeds=seeds[:1], reproj_gate=3.0)
    _assert_same_batch(res.passes[0], one.passes[0], "first of two")
    tab = res.table_all()
    assert np.array_equal(np.bincount(tab.seed_pass.cpu().numpy(), minlength=3),
                          [res.count.sum(), res.passes[0].count.sum(), res.passes[1].count.sum()])
    assert np.array_equal(np.diff(tab.offs), sum(b.count.astype(np.int64) for b in (res,) + res.passes))


def test_argument_errors(cuda):
    f = M.captures(5)
    for bad in ([(2, 2, 4)], [(2, 3, 5)], [(2, 3)], [], [(2, 3, 4)] * 5, [(-1, 3, 4)]):
        with pytest.raises(ValueError):
            _match(f, cuda, extra_seeds=bad)
    import test_extend_gpu as TE
    b3 = TE.three_cam_inputs(TE.fixture(4))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    with pytest.raises(ValueError, match="n_cams"):
        match_captures(t(b3[0]), t(b3[1]), t(b3[2]), t(b3[3]), b3[4], b3[5], extra_seeds=[(0, 1, 2)])
    plain = _match(f, cuda)
    F = torch.zeros((f.S * 9, 9), dtype=torch.float64, device=cuda)
    for kw in (dict(F=F), dict(proj=plain.proj), dict(F=F, proj=plain.proj)):
        with pytest.raises(TypeError, match="extra_seeds"):
            _match(f, cuda, extra_seeds=[M.SEED], **kw)


def test_stream_passes_the_keyword_through(cuda):
    f = M.captures(5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    batch = (t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs)
    one = _match(f, cuda, extra_seeds=[M.SEED])
    got, = list(match_capture_stream([batch], n_cams=5, extra_seeds=[M.SEED]))
    assert len(got.passes) == 1
    _assert_same_batch(got.passes[0], one.passes[0], "stream")


def test_sharded_call_refuses_the_keyword(cuda):
    from bpc_baseline_amd.distributed import DistEnv, match_captures_sharded
    f = M.captures(5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    env = DistEnv(0, 1, 0, cuda, False)
    with pytest.raises(NotImplementedError, match="extra_seeds"):
        match_captures_sharded(env, t(f.boxes), t(f.conf), t(f.cls), t(f.img_offs), f.Ks, f.RTs, n_cams=5,
                               extra_seeds=[M.SEED])
