"""mvm_fuse_rotations_sym (an addition to ABI 8, MVM_HAS_SYM_FUSE): the
host-side validation of the entry point -- no GPU, nothing is launched (the
kernel's parity is tests/test_pose_sym_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

# the pointer arguments in signature order
POINTERS = ["raw_dev", "scene_dev", "views_dev", "X_dev", "RTs_dev", "cams_host", "syms_dev", "rot_views_dev",
            "R_dev", "pose_dev", "spread_dev", "slot_status_dev", "row_status_dev", "sym_index_dev",
            "sym_margin_dev", "n_changed_dev"]
OPTIONAL = ["rot_views_dev", "spread_dev", "sym_margin_dev", "n_changed_dev"]
REQUIRED = [p for p in POINTERS if p not in OPTIONAL]
DEFAULTS = dict(D=4, scene_base=0, n_scenes=2, n_cams=4, row0=0, n_rows=3, mode=1, n_syms=4, rounds=2)


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _call(lib, null=(), every=FAKE, cams=(0, 2), **kw):
    a = dict(DEFAULTS, **kw)
    null = (null,) if isinstance(null, str) else null
    p = {name: (None if name in null else every) for name in POINTERS}
    if p["cams_host"] is not None:
        p["cams_host"] = (ctypes.c_int32 * max(len(cams), 1))(*cams)
    return lib.mvm_fuse_rotations_sym(p["raw_dev"], a["D"], p["scene_dev"], a["scene_base"], p["views_dev"],
                                      p["X_dev"], p["RTs_dev"], a["n_scenes"], a["n_cams"], a["row0"], a["n_rows"],
                                      p["cams_host"], a.get("n_sel", len(cams)), a["mode"], p["syms_dev"],
                                      a["n_syms"], a["rounds"], p["rot_views_dev"], p["R_dev"], p["pose_dev"],
                                      p["spread_dev"], p["slot_status_dev"], p["row_status_dev"],
                                      p["sym_index_dev"], p["sym_margin_dev"], p["n_changed_dev"], None)


def _reaches_the_pointer_check(lib, **kw):
    """Valid arguments get as far as the pointers: the null one is named."""
    assert _call(lib, null="pose_dev", **kw) == 1
    return lib.mvm_last_error_string().endswith(b" pose_dev")


def test_signature_declared(lib):
    assert "mvm_fuse_rotations_sym" in _native.header_symbols()
    assert hasattr(lib, "mvm_fuse_rotations_sym")
    assert len(_native.SIGNATURES["mvm_fuse_rotations_sym"][1]) == 27
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_ABI_VERSION 8" in text
    assert "#define MVM_HAS_SYM_FUSE 1" in text
    # the order of the header is the order of the binding, right behind the scorer
    syms = [s for s in _native.header_symbols() if s in _native.SIGNATURES]
    names = list(_native.SIGNATURES)
    assert syms.index("mvm_fuse_rotations_sym") == names.index("mvm_fuse_rotations_sym") \
        == names.index("mvm_match_scores") + 1


@pytest.mark.parametrize("name", REQUIRED)
def test_null_pointer_names_the_argument(lib, name):
    assert _call(lib, null=name) == 1                     # MVM_ERR_INVALID_ARGUMENT
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


def test_four_outputs_are_optional(lib):
    # with all four NULL the call still gets as far as naming another null pointer
    assert _call(lib, null=OPTIONAL + ["sym_index_dev"]) == 1
    assert lib.mvm_last_error_string().endswith(b" sym_index_dev")


@pytest.mark.parametrize("key, bad, good", [
    ("n_syms", 0, 1), ("n_syms", -3, 1024), ("rounds", 0, 1), ("rounds", 5, 4),
    ("n_cams", 2, 3), ("n_cams", 9, 8), ("mode", -1, 0), ("mode", 3, 2),
    ("row0", -1, 0), ("n_rows", -1, 1), ("n_scenes", -1, 0),
])
def test_each_range_end(lib, key, bad, good):
    width = {0: 3, 1: 4, 2: 6}
    fix = lambda v: dict(D=width.get(v, 4)) if key == "mode" else {}
    assert _call(lib, **{key: bad}, **fix(bad)) != 0
    msg = lib.mvm_last_error_string()
    assert key.encode() in msg and str(bad).encode() in msg
    assert _reaches_the_pointer_check(lib, **{key: good}, **fix(good))


def test_a_long_list_of_symmetries(lib):
    assert _reaches_the_pointer_check(lib, n_syms=1024)
    assert _reaches_the_pointer_check(lib, n_syms=2 ** 31 - 1)


@pytest.mark.parametrize("mode, D", ((0, 3), (1, 4), (2, 6)))
def test_the_width_goes_with_the_mode(lib, mode, D):
    assert _reaches_the_pointer_check(lib, mode=mode, D=D)
    for wrong in (D - 1, D + 1, 0, 9):
        assert _call(lib, mode=mode, D=wrong) == 1
        assert b"D=" + str(wrong).encode() in lib.mvm_last_error_string()


def test_the_selected_cameras(lib):
    assert _call(lib, cams=(), n_sel=0) == 1
    assert b"n_sel" in lib.mvm_last_error_string()
    assert _call(lib, cams=(0, 1, 2, 3, 0), n_cams=4) == 1            # more than n_cams
    assert b"n_sel" in lib.mvm_last_error_string()
    assert _reaches_the_pointer_check(lib, cams=(3, 1, 0, 2), n_cams=4)
    assert _reaches_the_pointer_check(lib, cams=tuple(range(8)), n_cams=8)
    for cams, n_cams in (((0, 4), 4), ((3,), 3), ((-1,), 4), ((0, 8), 8)):
        assert _call(lib, cams=cams, n_cams=n_cams) == 1
        msg = lib.mvm_last_error_string()
        assert b"cams_host" in msg and str(cams[-1]).encode() in msg


def test_more_rows_than_a_launch_holds(lib):
    assert _call(lib, n_rows=2 ** 40) == 2                            # MVM_ERR_UNSUPPORTED
    assert b"split" in lib.mvm_last_error_string()


def test_no_rows_launches_nothing(lib):
    # ok whatever the other arguments are, and no error is left behind
    assert _call(lib, n_rows=0, every=None) == 0
    assert _call(lib, n_rows=0) == 0
    assert _call(lib, n_rows=0, n_cams=9, mode=7, n_syms=0, rounds=9, D=0, cams=(11,)) == 0
    assert lib.mvm_last_error_string() == b""
