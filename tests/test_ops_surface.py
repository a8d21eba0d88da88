"""The boundary layer of bpc_baseline_amd.ops, without a GPU: the public names
and the schema of every ``torch.ops.mvmatch.*`` op are frozen, every op has a
fake that returns None, ``_check_args`` compares element counts as its three
modes say, and ``sparse_class`` is the candidate-list class predicate that
cube_free_scenes, lsap_sparse_stats and the batch chain used to spell out."""
import numpy as np
import pytest
import torch

from bpc_baseline_amd import ops

ALL = [
    "PairwisePlan", "TripletPlan",
    "pairwise_residual_argmin", "pairwise_residual_f64", "triplet_cost_argmin",
    "hbm_write_probe", "LsapPlan", "linear_sum_assignment_batched",
    "pack_detections", "triangulate_dlt", "select_triangulate",
    "triplet_minima", "linear_sum_assignment_resid", "select_triangulate_resid",
    "cube_free_scenes", "sparse_class_bounds", "lsap_sparse_stats", "compact_matches",
    "rig_matrices", "extend_costs", "extend_select_triangulate", "compact_matches_views",
]

# str(torch.ops.mvmatch.<op>.default._schema) of every op the package registers
SCHEMAS = {
    "pairwise_residual_argmin_out": "mvmatch::pairwise_residual_argmin_out(Tensor pts, Tensor cam_offs, Tensor F, SymInt[] pair_a, SymInt[] pair_b, SymInt n_scenes, SymInt n_cams, SymInt max_n, Tensor dist_offs, Tensor row_offs, Tensor(a10!) dist, Tensor(a11!) argmin, Tensor(a12!) minval, SymInt[]? opts=None, SymInt row_align=1) -> ()",
    "pairwise_residual_f64_out": "mvmatch::pairwise_residual_f64_out(Tensor pts, Tensor cam_offs, Tensor F, SymInt[] pair_a, SymInt[] pair_b, SymInt n_scenes, SymInt n_cams, SymInt max_n, SymInt mat_stride, SymInt ld, Tensor(a10!) e) -> ()",
    "triplet_cost_argmin_out": "mvmatch::triplet_cost_argmin_out(Tensor pts, Tensor cam_offs, Tensor F, SymInt n_scenes, SymInt max_n, Tensor cube_offs, Tensor row_offs, Tensor(a7!) cube, Tensor(a8!) argmin, Tensor(a9!) minval, Tensor(a10!) workspace, SymInt[]? opts=None) -> ()",
    "triplet_cost_bmin8_out": "mvmatch::triplet_cost_bmin8_out(Tensor pts, Tensor cam_offs, Tensor F, SymInt n_scenes, SymInt max_n, Tensor cube_offs, Tensor row_offs, Tensor(a7!) cube, Tensor(a8!) argmin, Tensor(a9!) minval, Tensor(a10!) bmin8, Tensor bmin8_offs, Tensor(a12!) workspace, SymInt[]? opts=None) -> ()",
    "lsap_solve_bmin8_out": "mvmatch::lsap_solve_bmin8_out(Tensor cost, Tensor cost_offs, Tensor dims, Tensor ws_offs, Tensor out_offs, Tensor(a5!) workspace, Tensor(a6!) row_ind, Tensor(a7!) col_ind, Tensor(a8!) status, Tensor bmin8, Tensor bmin8_offs, Tensor segs, SymInt long_min, SymInt long_max, SymInt short_max, SymInt[]? opts=None) -> ()",
    "lsap_solve_out": "mvmatch::lsap_solve_out(Tensor cost, Tensor cost_offs, Tensor dims, Tensor ws_offs, Tensor out_offs, Tensor(a5!) workspace, Tensor(a6!) row_ind, Tensor(a7!) col_ind, Tensor(a8!) status, SymInt long_min=1, SymInt long_max=4611686018427387904, SymInt[]? opts=None, SymInt short_max=-1) -> ()",
    "triplet_minima_out": "mvmatch::triplet_minima_out(Tensor pts, Tensor cam_offs, Tensor F, SymInt n_scenes, SymInt max_n, Tensor(a5!) bmin8, Tensor bmin8_offs, Tensor bm32, Tensor bm32_offs, Tensor(a9!) resid, SymInt[]? opts=None) -> ()",
    "lsap_solve_resid_out": "mvmatch::lsap_solve_resid_out(Tensor dims, Tensor ws_offs, Tensor out_offs, Tensor(a3!) workspace, Tensor(a4!) row_ind, Tensor(a5!) col_ind, Tensor(a6!) status, Tensor bmin8, Tensor bmin8_offs, Tensor bm32, Tensor bm32_offs, Tensor segs, Tensor resid, SymInt max_n, SymInt long_min, SymInt long_max, SymInt short_max, SymInt[]? opts=None) -> ()",
    "pack_detections_out": "mvmatch::pack_detections_out(Tensor boxes, Tensor conf, Tensor cls, Tensor img_offs, float conf_thresh, float class_id, Tensor(a6!) counts, Tensor(a7!) cam_offs, Tensor(a8!) pts, Tensor(a9!) boxes_out, Tensor(a10!) status) -> ()",
    "triangulate_dlt_out": "mvmatch::triangulate_dlt_out(Tensor proj, Tensor? set_of_point, Tensor pts2d, Tensor(a3!) X) -> ()",
    "select_triangulate_out": "mvmatch::select_triangulate_out(Tensor cube, Tensor cube_offs, Tensor cam_offs, Tensor lsap_offs, Tensor row_ind, Tensor col_ind, Tensor pts, Tensor proj, float threshold, Tensor(a9!) match, Tensor(a10!) cost, Tensor(a11!) X, Tensor(a12!) count) -> ()",
    "select_triangulate_resid_out": "mvmatch::select_triangulate_resid_out(Tensor resid, SymInt max_n, Tensor cam_offs, Tensor lsap_offs, Tensor row_ind, Tensor col_ind, Tensor pts, Tensor proj, float threshold, Tensor(a9!) match, Tensor(a10!) cost, Tensor(a11!) X, Tensor(a12!) count) -> ()",
    "compact_matches_out": "mvmatch::compact_matches_out(Tensor match, Tensor cost, Tensor X, Tensor count, Tensor seg_offs, Tensor pts, Tensor boxes, Tensor cam_offs, SymInt scene_base, Tensor(a9!) dense_offs, Tensor(a10!) scene_out, Tensor(a11!) match_out, Tensor(a12!) cost_out, Tensor(a13!) X_out, Tensor(a14!) boxes_out, Tensor(a15!) cent_out) -> ()",
    "compact_matches_views_out": "mvmatch::compact_matches_views_out(Tensor views, Tensor cost, Tensor ext_cost, Tensor X, Tensor count, Tensor seg_offs, Tensor pts, Tensor boxes, Tensor cam_offs, Tensor proj, SymInt scene_base, Tensor(a11!) dense_offs, Tensor(a12!) scene_out, Tensor(a13!) views_out, Tensor(a14!) n_views_out, Tensor(a15!) cost_out, Tensor(a16!) ext_cost_out, Tensor(a17!) X_out, Tensor(a18!) boxes_out, Tensor(a19!) cent_out, Tensor(a20!) reproj_out) -> ()",
    "rig_matrices_out": "mvmatch::rig_matrices_out(Tensor K, Tensor RT, SymInt[] pair_a, SymInt[] pair_b, Tensor(a4!) F, Tensor(a5!) proj, Tensor(a6!) status) -> ()",
    "extend_costs_out": "mvmatch::extend_costs_out(Tensor pts, Tensor cam_offs, Tensor F_ext, Tensor match, Tensor match_offs, Tensor count, Tensor ext_offs, SymInt n_cams, SymInt max_rows, Tensor(a9!) E) -> ()",
    "extend_select_triangulate_out": "mvmatch::extend_select_triangulate_out(Tensor E, Tensor ext_offs, Tensor lsap_offs, Tensor row_ind, Tensor col_ind, Tensor match, Tensor match_offs, Tensor count, Tensor pts, Tensor cam_offs, Tensor proj, float threshold, Tensor(a12!) views, Tensor(a13!) ext_cost, Tensor(a14!) X) -> ()",
}


def test_public_names_frozen():
    assert ops.__all__ == ALL
    for name in ALL:
        assert hasattr(ops, name), name


def test_every_op_is_listed():
    registered = {n for n in dir(torch.ops.mvmatch) if n.endswith("_out")}
    assert registered == set(SCHEMAS)


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_op_schema_frozen(name):
    assert str(getattr(torch.ops.mvmatch, name).default._schema) == SCHEMAS[name]


def _fake_argument(arg):
    kind = str(arg.type)
    if kind.startswith("Optional["):
        return None
    if kind.startswith("List["):
        return []
    return {"Tensor": torch.empty(0), "int": 0, "SymInt": 0, "float": 0.0}[kind]


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_op_fake_returns_none(name):
    """No launch, no validation: what tracing under FakeTensorMode needs of
    an op that only writes its arguments."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = getattr(torch.ops.mvmatch, name)
    with FakeTensorMode():
        assert op(*[_fake_argument(a) for a in op.default._schema.arguments]) is None


@pytest.mark.parametrize("mode", [ops.EXACT, ops.AT_LEAST, ops.ANY])
def test_check_args_modes(mode):
    cpu = torch.device("cpu")
    row = lambda numel: [(torch.zeros(4), "ahead", torch.float32, 4, ops.EXACT),
                         (torch.zeros(numel), "buf", torch.float32, 8, mode)]
    ops._check_args(cpu, row(8))                        # the boundary size
    fewer_ok, more_ok = mode == ops.ANY, mode != ops.EXACT
    for numel, ok, word in ((7, fewer_ok, "expected" if mode == ops.EXACT else "needs"),
                            (9, more_ok, "expected")):
        if ok:
            ops._check_args(cpu, row(numel))
            continue
        with pytest.raises(ValueError, match=rf"^buf holds {numel} elements, {word} 8$"):
            ops._check_args(cpu, row(numel))


def test_check_args_requires_dtype_device_layout():
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="^buf: expected torch.int32"):
        ops._check_args(cpu, [(torch.zeros(2), "buf", torch.int32, None, ops.ANY)])
    with pytest.raises(ValueError, match="^buf: expected device meta"):
        ops._check_args(torch.device("meta"), [(torch.zeros(2), "buf", torch.float32, None, ops.ANY)])
    with pytest.raises(ValueError, match="^buf: must be contiguous"):
        ops._check_args(cpu, [(torch.zeros(2, 2).t(), "buf", torch.float32, None, ops.ANY)])
    with pytest.raises(ValueError, match="^buf: unknown mode"):
        ops._check_args(cpu, [(torch.zeros(2), "buf", torch.float32, 2, "exactly")])


def test_device_refusals_name_the_gpu():
    z = torch.zeros(0)
    with pytest.raises(ValueError, match="K must be a GPU tensor"):
        torch.ops.mvmatch.rig_matrices_out(z, z, [], [], z, z, z)
    with pytest.raises(ValueError, match="cost must be a float32 GPU tensor"):
        torch.ops.mvmatch.lsap_solve_bmin8_out(z, z, z, z, z, z, z, z, z, z, z, z, 0, 0, 0)


# ---- the candidate-list class (loads the library, like tests/test_capi.py) ------
def test_cube_free_refuses_wide_views_of_empty_scenes():
    assert ops.cube_free_scenes(np.array([[0, 300, 50], [0, 200, 50]])).tolist() == [False, True]
    assert ops.cube_free_scenes(np.array([[300, 0, 50], [50, 300, 0], [256, 0, 256]])).tolist() == [
        False, False, True]


@pytest.mark.parametrize("min_cols", [None, 2048, 512])
def test_sparse_class_equals_the_inline_predicates(min_cols):
    """The three expressions sparse_class replaced, as they stood."""
    lo, hi, sh = ops.sparse_class_bounds()
    lo = lo if min_cols is None else int(min_cols)
    c = np.random.default_rng(5).integers(0, 301, (1000, 3)).astype(np.int64)
    extra = c[:40].copy()                      # and 40 more around the short side's bound
    extra[:, 2] = np.random.default_rng(6).integers(sh - 50, sh + 50, 40)
    c = np.concatenate([c, extra])
    nm, p = c[:, 0] * c[:, 1], c[:, 2]
    lng, sht = np.maximum(nm, p), np.minimum(nm, p)
    # cube_free_scenes: ok = ...
    ok = (c.max(axis=1) <= 256) & (lng >= lo) & (lng > 1024) & (lng <= hi) & (sht <= sh)
    assert np.array_equal((c.max(axis=1) <= 256) & ops.sparse_class(lng, sht, min_cols), ok)
    assert ok.any() and not ok.all()
    # what cube_free_scenes now returns differs from the old ``empty | ok``
    # only where an empty scene has a view above 256
    empty = (nm == 0) | (p == 0)
    now = ops.cube_free_scenes(c, min_cols)
    assert np.array_equal(now, (empty | ok) & ~(empty & (c.max(axis=1) > 256)))
    # lsap_sparse_stats: cls = ...   (rows, cols of the plan: any orientation)
    rows, cols = (nm, p) if min_cols is None else (p, nm)
    lng, sht = np.maximum(rows, cols), np.minimum(rows, cols)
    cls = (lng >= lo) & (lng > 1024) & (lng <= hi) & (sht >= 1) & (sht <= sh)
    assert np.array_equal(ops.sparse_class(lng, sht, min_cols) & (sht >= 1), cls)
    # _device_chain, default bounds only: the scenes whose cube kernel also writes the 8-row minima
    if min_cols is None:
        c3 = c
        chain = (nm >= lo) & (nm > 1024) & (nm <= hi) & (c3[:, 2] <= sh) & (nm > c3[:, 2])
        assert np.array_equal(ops.sparse_class(nm, c3[:, 2]) & (nm > c3[:, 2]), chain)
        assert chain.any()
