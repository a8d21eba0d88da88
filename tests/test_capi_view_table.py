"""mvm_compact_matches_views (an addition to ABI 8, MVM_HAS_VIEW_TABLE): the
host-side validation of the C-camera match-table entry point -- no GPU,
nothing is launched (the kernel's parity is tests/test_view_table_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

# the pointer arguments in signature order (n_scenes, n_cams and scene_base sit after proj_dev)
INPUTS = ["views_dev", "cost_dev", "ext_cost_dev", "X_dev", "count_dev", "seg_offs_dev", "pts_dev",
          "boxes_dev", "cam_offs_dev", "proj_dev"]
OUTPUTS = ["dense_offs_dev", "scene_out_dev", "views_out_dev", "n_views_out_dev", "cost_out_dev",
           "ext_cost_out_dev", "X_out_dev", "boxes_out_dev", "cent_out_dev", "reproj_out_dev"]
POINTERS = INPUTS + OUTPUTS
OPTIONAL_AT_3 = ("ext_cost_dev", "ext_cost_out_dev")     # arrays of no element when C == 3


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _call(lib, n_scenes, n_cams=4, null=None, every=FAKE):
    p = [None if name == null else every for name in POINTERS]
    return lib.mvm_compact_matches_views(*p[:len(INPUTS)], n_scenes, n_cams, 0, *p[len(INPUTS):], None)


def test_signature_declared(lib):
    assert "mvm_compact_matches_views" in _native.header_symbols()
    assert len(_native.SIGNATURES["mvm_compact_matches_views"][1]) == len(POINTERS) + 4
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_ABI_VERSION 8" in text
    assert "#define MVM_HAS_VIEW_TABLE 1" in text
    # the order of the header is the order of the binding
    syms = [s for s in _native.header_symbols() if s in _native.SIGNATURES]
    assert syms.index("mvm_compact_matches_views") == list(_native.SIGNATURES).index(
        "mvm_compact_matches_views")


@pytest.mark.parametrize("n_cams", [4, 8])
@pytest.mark.parametrize("name", POINTERS)
def test_null_pointer_names_the_argument(lib, name, n_cams):
    assert _call(lib, 3, n_cams, null=name) == 1          # MVM_ERR_INVALID_ARGUMENT
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


@pytest.mark.parametrize("name", [n for n in POINTERS if n not in OPTIONAL_AT_3])
def test_null_pointer_with_three_cameras(lib, name):
    assert _call(lib, 3, 3, null=name) == 1
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


@pytest.mark.parametrize("n_cams", [2, 9, 0, -1])
def test_n_cams_outside_the_range_is_refused(lib, n_cams):
    assert _call(lib, 3, n_cams) != 0
    msg = lib.mvm_last_error_string()
    assert b"n_cams" in msg and str(n_cams).encode() in msg


def test_empty_batch_launches_nothing(lib):
    # no scenes: ok whatever the pointers and n_cams are, and no error is left behind
    assert _call(lib, 0, every=None) == 0
    assert _call(lib, 0) == 0
    assert _call(lib, 0, n_cams=9) == 0
    assert lib.mvm_last_error_string() == b""
    assert _call(lib, -1) == 1
    assert b"n_scenes" in lib.mvm_last_error_string()
