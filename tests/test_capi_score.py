"""mvm_score_poses and mvm_match_scores (additions to ABI 8, MVM_HAS_SCORES):
the host-side validation of the entry points -- no GPU, nothing is launched
(the kernels' parity is tests/test_score_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

# the pointer arguments in signature order
POINTERS = ["pose_dev", "scene_dev", "gt_pose_dev", "gt_offs_dev", "verts_dev", "syms_dev", "err_dev", "sym_dev",
            "t_err_dev", "rot_cos_dev"]
OPTIONAL = ["t_err_dev", "rot_cos_dev"]
REQUIRED = [p for p in POINTERS if p not in OPTIONAL]
DEFAULTS = dict(scene_base=0, n_scenes=2, g_max=3, n_verts=8, n_syms=2, row0=0, n_rows=3)

MATCH_POINTERS = ["err_dev", "row_offs_dev", "gt_offs_dev", "thresholds_host", "gt_index_dev", "tp_dev"]
MATCH_DEFAULTS = dict(g_max=3, n_scenes=2, n_thresholds=2, n_rows_total=5)


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _score(lib, null=(), every=FAKE, **kw):
    a = dict(DEFAULTS, **kw)
    null = (null,) if isinstance(null, str) else null
    p = {name: (None if name in null else every) for name in POINTERS}
    return lib.mvm_score_poses(p["pose_dev"], p["scene_dev"], a["scene_base"], p["gt_pose_dev"], p["gt_offs_dev"],
                               a["n_scenes"], a["g_max"], p["verts_dev"], a["n_verts"], p["syms_dev"], a["n_syms"],
                               a["row0"], a["n_rows"], p["err_dev"], p["sym_dev"], p["t_err_dev"], p["rot_cos_dev"],
                               None)


def _match(lib, null=(), every=FAKE, **kw):
    a = dict(MATCH_DEFAULTS, **kw)
    null = (null,) if isinstance(null, str) else null
    p = {name: (None if name in null else every) for name in MATCH_POINTERS}
    if p["thresholds_host"] is not None:
        p["thresholds_host"] = (ctypes.c_double * 16)(*([1.0] * 16))
    return lib.mvm_match_scores(p["err_dev"], a["g_max"], p["row_offs_dev"], p["gt_offs_dev"], a["n_scenes"],
                                p["thresholds_host"], a["n_thresholds"], p["gt_index_dev"], p["tp_dev"],
                                a["n_rows_total"], None)


def _score_reaches_the_pointer_check(lib, **kw):
    """Valid arguments get as far as the pointers: the null one is named."""
    assert _score(lib, null="sym_dev", **kw) == 1
    return lib.mvm_last_error_string().endswith(b" sym_dev")


def _match_reaches_the_pointer_check(lib, **kw):
    assert _match(lib, null="thresholds_host", **kw) == 1
    return lib.mvm_last_error_string().endswith(b" thresholds_host")


def test_signatures_declared(lib):
    for name, n_args in (("mvm_score_poses", 18), ("mvm_match_scores", 11)):
        assert name in _native.header_symbols()
        assert hasattr(lib, name)
        assert len(_native.SIGNATURES[name][1]) == n_args
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_ABI_VERSION 8" in text
    assert "#define MVM_HAS_SCORES 1" in text
    # the order of the header is the order of the binding, right behind the poses
    syms = [s for s in _native.header_symbols() if s in _native.SIGNATURES]
    names = list(_native.SIGNATURES)
    assert syms.index("mvm_score_poses") == names.index("mvm_score_poses") == names.index("mvm_fuse_rotations") + 1
    assert syms.index("mvm_match_scores") == names.index("mvm_match_scores") == names.index("mvm_score_poses") + 1


@pytest.mark.parametrize("name", REQUIRED)
def test_score_null_pointer_names_the_argument(lib, name):
    assert _score(lib, null=name) == 1                    # MVM_ERR_INVALID_ARGUMENT
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


def test_t_err_and_rot_cos_are_optional(lib):
    # with both NULL the call still gets as far as naming another null pointer
    assert _score(lib, null=OPTIONAL + ["sym_dev"]) == 1
    assert lib.mvm_last_error_string().endswith(b" sym_dev")


@pytest.mark.parametrize("key, bad, good", [
    ("n_syms", 0, 1), ("n_syms", 65, 64), ("n_verts", 0, 1), ("g_max", 0, 1),
    ("row0", -1, 0), ("n_rows", -1, 1), ("n_scenes", -1, 0),
])
def test_score_each_range_end(lib, key, bad, good):
    assert _score(lib, **{key: bad}) == 1
    msg = lib.mvm_last_error_string()
    assert key.encode() in msg and str(bad).encode() in msg
    assert _score_reaches_the_pointer_check(lib, **{key: good})


def test_score_more_pairs_than_a_grid_holds(lib):
    per_grid = 0xFFFFFFFF // 256 * 256
    assert _score(lib, n_rows=per_grid // 3 + 1, g_max=3) == 2            # MVM_ERR_UNSUPPORTED
    msg = lib.mvm_last_error_string()
    assert b"n_rows" in msg and b"g_max" in msg and b"split" in msg
    assert _score(lib, n_rows=2 ** 62, g_max=2 ** 31 - 1) == 2            # the product is never formed
    assert _score_reaches_the_pointer_check(lib, n_rows=per_grid // 3, g_max=3)


def test_score_no_rows_launches_nothing(lib):
    # ok whatever the other arguments are, and no error is left behind
    assert _score(lib, n_rows=0, every=None) == 0
    assert _score(lib, n_rows=0) == 0
    assert _score(lib, n_rows=0, n_syms=99, n_verts=-4, g_max=0, n_scenes=-1, row0=-7) == 0
    assert lib.mvm_last_error_string() == b""


@pytest.mark.parametrize("name", MATCH_POINTERS)
def test_match_null_pointer_names_the_argument(lib, name):
    assert _match(lib, null=name) == 1
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


def test_match_pointers_nothing_reads_may_be_null(lib):
    # no rows: err and gt_index are not touched; no captures: the offsets and tp are not
    assert _match(lib, null=["err_dev", "gt_index_dev", "tp_dev"], n_rows_total=0) == 1
    assert lib.mvm_last_error_string().endswith(b" tp_dev")
    assert _match(lib, null=["row_offs_dev", "gt_offs_dev", "tp_dev", "gt_index_dev"], n_scenes=0) == 1
    assert lib.mvm_last_error_string().endswith(b" gt_index_dev")


@pytest.mark.parametrize("key, bad, good, status", [
    ("g_max", 0, 1, 2), ("g_max", 1025, 1024, 2),                         # MVM_ERR_UNSUPPORTED
    ("n_thresholds", 0, 1, 1), ("n_thresholds", 17, 16, 1),
    ("n_scenes", -1, 0, 1), ("n_rows_total", -1, 0, 1),
])
def test_match_each_range_end(lib, key, bad, good, status):
    assert _match(lib, **{key: bad}) == status
    msg = lib.mvm_last_error_string()
    assert key.encode() in msg and str(bad).encode() in msg
    assert _match_reaches_the_pointer_check(lib, **{key: good})


def test_match_nothing_to_write_launches_nothing(lib):
    assert _match(lib, n_scenes=0, n_rows_total=0, every=None) == 0
    assert _match(lib, n_scenes=0, n_rows_total=0, g_max=5000, n_thresholds=99) == 0
    assert lib.mvm_last_error_string() == b""
