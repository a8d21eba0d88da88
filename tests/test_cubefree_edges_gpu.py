"""The cube-free association (mvm_triplet_minima -> mvm_lsap_solve_resid ->
mvm_select_triangulate_resid) on the inputs test_cubefree_gpu.py's make_scenes
batches never produce (tests/cubefree_inputs.py builds them, and
tests/test_cubefree_edges_model.py proves on the CPU that they are what they
claim): exact ties and zeros, a fp64 sum on a 16-bit key carry, residuals at
and above 2^64, float32 costs of +inf, non-finite sums, costs below 2^-100,
constant cubes, duplicated detections, infeasible scenes.

References: the CPU oracle (oracle/mvm_oracle.c) for the minima and the
residuals, scipy on the oracle cube for the assignment,
oracle/pipeline.select_sort on the oracle cube for the select tail.  Every
comparison is bit for bit.
"""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

import cubefree_inputs as CI
from oracle import oracle as O
from oracle import pipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def refs():
    """name -> reference of a batch, computed once and left unchanged."""
    return {}


class _Ref:
    pass


def _reference(refs, name, batch):
    if name in refs:
        return refs[name]
    r = _Ref()
    S = len(batch.scenes)
    r.batch = batch
    r.cube, _, _, r.offs, _ = O.cube(batch.pts, batch.co, batch.F, S)
    r.max_n = max(max(c) for c in batch.counts)
    r.resid = O.residuals(batch.pts, batch.co, batch.F, S, r.max_n)
    r.lsa = {}
    refs[name] = r
    return r


def _dev(cuda, batch):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t(batch.pts), t(batch.co), t(batch.F)


# ----------------------------------------------------------------- minima ----
MINIMA = ["coarse", "straddle", "mixed", "two64", "huge", "tiny"]


@pytest.fixture(scope="module")
def minima_batches():
    return CI.minima_cases()


@pytest.mark.parametrize("with_bmin8", [True, False], ids=["bmin8", "blocks_only"])
@pytest.mark.parametrize("name", MINIMA)
def test_minima_edges_equal_oracle(cuda, refs, minima_batches, name, with_bmin8):
    """bm8, bm32 and the fp64 residuals against the oracle, with the 8-row
    minima (the group path) and without (N % 16 == 0: the unrolled whole-chunk
    path; a ragged N: the row loop)."""
    from bpc_baseline_amd import ops
    batch = minima_batches[name]
    ref = _reference(refs, "minima_" + name, batch)
    counts = batch.counts
    assert any(c[0] % 16 == 0 for c in counts) and any(c[0] % 16 for c in counts)
    S = len(counts)
    plan = ops.TripletPlan(batch.co, S, device=cuda)
    P, C, FF = _dev(cuda, batch)
    bm32 = torch.full((max(plan.n_bm32, 8),), 0x5A5A, dtype=torch.int16, device=cuda)
    plan.workspace.fill_(0xFF)                       # NaN everywhere the kernel does not write
    if with_bmin8:
        bm8 = torch.full((max(plan.n_bmin8, 1),), -1, dtype=torch.int16, device=cuda)
        ops.triplet_minima(P, C, FF, plan, bmin8=bm8, bm32=bm32)
        got8 = bm8.cpu().numpy().view(np.uint16)
    else:
        bm8, _ = ops.triplet_minima(P, C, FF, plan, bm32=bm32, with_bmin8=False)
        assert bm8.numel() == 0
    got32 = bm32.cpu().numpy().view(np.uint16)
    ld = (plan.max_n + 3) // 4 * 4
    resid = plan.workspace[:plan.workspace_bytes].view(torch.float64).cpu().numpy().reshape(S, 3, plan.max_n, ld)
    if with_bmin8:                                   # the cube kernel on the same batch: cube and 8-row minima
        ref8 = torch.full_like(bm8, -1)
        cube, _, _ = ops.triplet_cost_argmin(P, C, FF, plan, bmin8=ref8)
        assert np.array_equal(cube.cpu().numpy().view(np.int32), ref.cube.view(np.int32)), (name, "cube")
        dev8 = ref8.cpu().numpy().view(np.uint16)
    for s, (N, M, Pn) in enumerate(counts):
        cs = ref.cube[ref.offs[s]:ref.offs[s + 1]].reshape(N, M, Pn)
        want8 = O.bmin8_keys(cs)
        if with_bmin8:
            o = plan.bmin8_offs_host[s]
            bad = np.nonzero(got8[o:o + want8.size] != want8.reshape(-1))[0]
            assert bad.size == 0, (name, s, "8-row minima", bad[:4], got8[o + bad[:4]], want8.reshape(-1)[bad[:4]])
            assert np.array_equal(dev8[o:o + want8.size], want8.reshape(-1)), (name, s, "cube kernel's minima")
        o32 = plan.bm32_offs_host[s]
        want32 = O.bm32_keys(want8, N, M, Pn).reshape(-1)
        bad = np.nonzero(got32[o32:o32 + want32.size] != want32)[0]
        assert bad.size == 0, (name, s, "block minima", bad[:4], got32[o32 + bad[:4]], want32[bad[:4]])
        for m, (a, b) in enumerate(((N, M), (Pn, N), (Pn, M))):
            g, w = resid[s, m, :a, :b], ref.resid[s, m, :a, :b]
            assert np.array_equal(g.view(np.int64), w.view(np.int64)), (name, s, "residuals", m)
    if name == "straddle":                           # the key the recheck must produce, named
        for s, sc in enumerate(batch.scenes):
            i, j, k, sm = sc.note["straddle"]
            N, M, Pn = counts[s]
            npad, bps = (N + 15) // 16 * 16, (M + 31) // 32
            key = got32[plan.bm32_offs_host[s] + (k * bps + j // 32) * npad + i]
            assert key == CI.key16(np.float32(sm / 3.0).view(np.uint32)), (s, hex(key))
            assert key != CI.key16((np.float32(sm) * np.float32(1.0 / 3.0)).view(np.uint32))


# ------------------------------------------------------------- assignment ----
ASSIGN = ["lists", "overflow", "constant", "f13_zero", "dup10", "dup30", "inf_feasible", "infeasible",
          "min_cols"]
VARIANTS = {"default": (0, True), "blocks1": (1, True), "blocks64": (64, True),
            "no_bmin8": (0, False), "no_bmin8_blocks1": (1, False), "cube_form": (0, None)}


@pytest.fixture(scope="module")
def assign_cases():
    return CI.assign_cases()


def _scipy(ref, s):
    """scipy on the oracle cube of scene s: (rows, cols), or None (infeasible)."""
    if s not in ref.lsa:
        N, M, Pn = ref.batch.counts[s]
        try:
            ref.lsa[s] = scipy_lsa(ref.cube[ref.offs[s]:ref.offs[s + 1]].reshape(N * M, Pn))
        except ValueError as e:
            assert "infeasible" in str(e)
            ref.lsa[s] = None
    return ref.lsa[s]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ASSIGN)
def test_assignment_edges_equal_scipy(cuda, refs, assign_cases, name, variant):
    """linear_sum_assignment_resid (lsap_sparse_blocks default / 1 / 64, with
    and without the 8-row minima) and the cube-form assignment on the same
    batch, against scipy on the oracle cube; the solver's counters say the
    case ran the code it is about."""
    from bpc_baseline_amd import ops
    case = assign_cases[name]
    batch = case.batch
    ref = _reference(refs, "assign_" + name, batch)
    counts = batch.counts
    S = len(counts)
    blocks, with_bmin8 = VARIANTS[variant]
    opts = dict(case.options or {})
    if blocks:
        opts["lsap_sparse_blocks"] = blocks
    opts = opts or None
    plan = ops.TripletPlan(batch.co, S, device=cuda)
    P, C, FF = _dev(cuda, batch)
    c3 = plan.counts
    if with_bmin8 is None:
        bm8 = torch.empty(max(plan.n_bmin8, 1), dtype=torch.int16, device=cuda)
        cube, _, _ = ops.triplet_cost_argmin(P, C, FF, plan, bmin8=bm8)
        lplan = ops.LsapPlan(c3[:, 0] * c3[:, 1], c3[:, 2], device=cuda)
        r, c, st = ops.linear_sum_assignment_batched(cube, plan.cube_offs[:-1].contiguous(), lplan, options=opts,
                                                     bmin8=(bm8, plan.bmin8_offs, plan.segs))
    else:
        lplan = ops.LsapPlan(c3[:, 0] * c3[:, 1], c3[:, 2], device=cuda, resid=True)
        minima = ops.triplet_minima(P, C, FF, plan, with_bmin8=with_bmin8)
        r, c, st = ops.linear_sum_assignment_resid(lplan, plan, minima, options=opts)
    r, c, st = r.cpu().numpy(), c.cpu().numpy(), st.cpu().numpy()
    want_st = case.status or [0] * S
    assert list(st) == want_st, (name, variant, list(st))
    o = lplan.out_offs_host
    for s, (N, M, Pn) in enumerate(counts):
        want = _scipy(ref, s)
        if want_st[s] == 2:
            assert want is None                      # scipy raises on this scene's cube
            continue
        assert np.array_equal(r[o[s]:o[s + 1]], want[0]), (name, variant, s, "rows")
        bad = np.nonzero(c[o[s]:o[s + 1]] != want[1])[0]
        assert bad.size == 0, (name, variant, s, "cols", bad[:4], c[o[s] + bad[:4]], want[1][bad[:4]])
    if variant != "default":
        return
    stats = ops.lsap_sparse_stats(lplan, min_cols=(case.options or {}).get("lsap_sparse_min_cols"))
    print(f"\nlsap_sparse_stats {name}: [dense min scans, dense tie scans, overflowed lists, steps] per scene "
          f"{stats.tolist()}")
    # every scene is of the candidate-list class (an infeasible problem ends
    # before its counters are written)
    assert (stats[np.array(want_st) == 0] >= 0).all()
    for s, regime in enumerate(case.regime):
        if regime == "overflow":
            assert stats[s, 2] > 0 and stats[s, 1] > 0, (name, s, stats[s])
    lists = [s for s, regime in enumerate(case.regime) if regime == "lists"]
    if lists:
        # the bound of test_resid_lists_hold_on_small_rows: dense scans on at
        # most 5% of the short-side rows
        rows = sum(counts[s][2] for s in lists)
        assert stats[lists, 0].sum() <= 0.05 * rows, stats[lists, 0]
        assert stats[lists, 1].sum() <= 0.05 * rows, stats[lists, 1]


# ------------------------------------------------------------ select tail ----
@pytest.fixture(scope="module")
def select_ref(refs):
    batch = CI.select_batch()
    ref = _reference(refs, "select", batch)
    rows, cols, offs = [], [], [0]
    for s in range(len(batch.scenes)):
        rr, cc = _scipy(ref, s)
        rows.append(rr)
        cols.append(cc)
        offs.append(offs[-1] + len(rr))
    ref.row_ind = np.concatenate(rows).astype(np.int64)
    ref.col_ind = np.concatenate(cols).astype(np.int64)
    ref.lsap_offs = np.array(offs, np.int64)
    # an attained cost that several matches of scene 1 share
    N, M, Pn = batch.counts[1]
    v = ref.cube[ref.offs[1]:ref.offs[2]][rows[1] * Pn + cols[1]]
    vals, n = np.unique(v, return_counts=True)
    assert (n >= 2).any()
    ref.attained = np.float32(vals[n >= 2][len(vals[n >= 2]) // 2])
    ref.n_attained = sum(int((ref.cube[ref.offs[s]:ref.offs[s + 1]][rows[s] * batch.counts[s][2] + cols[s]]
                              == ref.attained).sum()) for s in range(len(batch.scenes)))
    assert ref.n_attained >= 2
    return ref


@pytest.mark.parametrize("edge", ["at", "below", "above", "inf"])
def test_select_resid_edges(cuda, select_ref, edge):
    """select_triangulate_resid on rectified scenes whose objects appear twice
    in every view (matches with bit-equal costs: the stable order shows),
    against select_sort on the oracle cube and the cube-form kernel, at a
    threshold that is an attained cost (strict <: dropped), one float32 ulp
    either side of it (as Python floats: the compare is in float64), +inf."""
    from bpc_baseline_amd import ops
    from bpc_baseline_amd.inference.utils.camera_utils import projection_matrices
    from bpc_baseline_amd.synth import make_scenes
    ref = select_ref
    batch = ref.batch
    S = len(batch.scenes)
    a32 = ref.attained
    thr = {"at": float(a32), "below": float(np.nextafter(a32, np.float32(0))),
           "above": float(np.nextafter(a32, np.float32(np.inf))), "inf": float("inf")}[edge]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    P, C, FF = _dev(cuda, batch)
    plan = ops.TripletPlan(batch.co, S, device=cuda)
    ops.triplet_minima(P, C, FF, plan)
    rig = make_scenes(S, 3, 8, seed=3)               # any projection matrices
    proj = t(projection_matrices(rig.meta["Ks"], rig.meta["RTs"]))
    lo, ri, ci = t(ref.lsap_offs), t(ref.row_ind), t(ref.col_ind)
    a = ops.select_triangulate_resid(plan, C, lo, ri, ci, P, proj, thr)
    cube, _, _ = ops.triplet_cost_argmin(P, C, FF, plan)
    b = ops.select_triangulate(cube, plan.cube_offs, C, lo, ri, ci, P, proj, thr)
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    kept_at = 0
    for s, (N, M, Pn) in enumerate(batch.counts):
        o, e = int(ref.lsap_offs[s]), int(ref.lsap_offs[s + 1])
        rm, rv = pipeline.select_sort(ref.cube[ref.offs[s]:ref.offs[s + 1]], M, Pn, ref.row_ind[o:e],
                                      ref.col_ind[o:e], thr)
        k = rm.shape[0]
        assert a[3][s] == k and b[3][s] == k, (edge, s, a[3][s], b[3][s], k)
        np.testing.assert_array_equal(a[0][o:o + k], rm)                       # match and order
        np.testing.assert_array_equal(a[1][o:o + k].view(np.int32), rv.view(np.int32))
        np.testing.assert_array_equal(a[0][o:o + k], b[0][o:o + k])
        np.testing.assert_array_equal(a[1][o:o + k].view(np.int32), b[1][o:o + k].view(np.int32))
        np.testing.assert_array_equal(a[2][o:o + k].view(np.int64), b[2][o:o + k].view(np.int64))
        if edge == "inf":
            assert k == e - o and len(np.unique(rv)) < k                       # bit-equal costs among the matches
        kept_at += int((rv == a32).sum())
    # strict <: the attained cost is dropped at and below it, kept one ulp above
    assert kept_at == (0 if edge in ("at", "below") else ref.n_attained), (edge, kept_at, ref.n_attained)


# ------------------------------------------------------------- end to end ----
@pytest.mark.parametrize("rig", ["host", "device"])
def test_match_captures_with_duplicated_boxes(cuda, rig):
    """match_captures(keep_cube=False) against keep_cube=True on detector
    batches of 80 and 130 detections per view with 20% of each image's boxes
    duplicated."""
    from bpc_baseline_amd import ops
    from bpc_baseline_amd.inference.batch_match import match_captures
    boxes, conf, cls, img_offs, Ks, RTs = CI.dup_detector_batch([(3, 80), (2, 130)], 0.2, 31)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    args = (t(boxes), t(conf), t(cls), t(img_offs), Ks, RTs)
    a = match_captures(*args, keep_cube=False, rig=rig)
    b = match_captures(*args, keep_cube=True, rig=rig)
    assert a.cube is None and b.cube is not None
    assert ops.cube_free_scenes(np.diff(a.cam_offs).reshape(-1, 3)).all()
    assert np.array_equal(a.count, b.count) and np.array_equal(a.offs, b.offs) and (a.count > 0).all()
    for s in range(len(a.count)):
        k = slice(int(a.offs[s]), int(a.offs[s]) + int(a.count[s]))
        assert np.array_equal(a.match[k].cpu().numpy(), b.match[k].cpu().numpy()), s
        assert np.array_equal(a.cost[k].cpu().numpy().view(np.int32), b.cost[k].cpu().numpy().view(np.int32)), s
        assert np.array_equal(a.X[k].cpu().numpy().view(np.int64), b.X[k].cpu().numpy().view(np.int64)), s
