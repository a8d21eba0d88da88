"""mvm_extend_costs / mvm_extend_select_triangulate: host-side validation of
the C entries (no kernel is launched here)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

COST_PTRS = ("pts_dev", "cam_offs_dev", "F_ext_dev", "match_dev", "match_offs_dev", "count_dev",
             "ext_offs_dev", "E_dev")
# (name, position) of the pointers mvm_extend_select_triangulate requires
SEL_PTRS = (("ext_offs_dev", 1), ("lsap_out_offs_dev", 2), ("match_dev", 5), ("match_offs_dev", 6),
            ("count_dev", 7), ("cam_offs_dev", 9), ("proj_dev", 10), ("views_dev", 14),
            ("ext_cost_dev", 15), ("X_dev", 16))


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _cost_args(null=None, n_scenes=2, n_cams=4, max_rows=5):
    p = [None if n == null else FAKE for n in COST_PTRS]
    return p[:7] + [n_scenes, n_cams, max_rows, p[7], None]


def _sel_args(null=None, n_scenes=2, n_cams=4):
    a = [FAKE] * 11 + [n_scenes, n_cams, ctypes.c_double(30.0), FAKE, FAKE, FAKE, None]
    for name, pos in SEL_PTRS:
        if name == null:
            a[pos] = None
    return a


def test_header_announces_the_extension():
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_HAS_EXTEND 1" in text
    assert "#define MVM_ABI_VERSION 8" in text
    assert {"mvm_extend_costs", "mvm_extend_select_triangulate"} <= set(_native.header_symbols())


@pytest.mark.parametrize("name", COST_PTRS)
def test_extend_costs_refuses_null_by_name(lib, name):
    assert lib.mvm_extend_costs(*_cost_args(null=name)) == 1
    assert f"null pointer: {name}".encode() in lib.mvm_last_error_string()


@pytest.mark.parametrize("name", [n for n, _ in SEL_PTRS])
def test_extend_select_refuses_null_by_name(lib, name):
    assert lib.mvm_extend_select_triangulate(*_sel_args(null=name)) == 1
    assert f"null pointer: {name}".encode() in lib.mvm_last_error_string()


def test_empty_batches_launch_nothing(lib):
    none8 = [None] * 7
    # no capture, no extra camera, no match: MVM_OK whatever the pointers
    assert lib.mvm_extend_costs(*none8, 0, 4, 5, None, None) == 0
    assert lib.mvm_extend_costs(*none8, 3, 3, 5, None, None) == 0
    assert lib.mvm_extend_costs(*none8, 3, 5, 0, None, None) == 0
    none11 = [None] * 11
    assert lib.mvm_extend_select_triangulate(*none11, 0, 4, ctypes.c_double(30.0), None, None, None,
                                             None) == 0
    assert lib.mvm_extend_select_triangulate(*none11, 2, 3, ctypes.c_double(30.0), None, None, None,
                                             None) == 0


def test_camera_count_and_sizes(lib):
    assert lib.mvm_extend_costs(*_cost_args(n_cams=9)) == 2
    assert b"n_cams" in lib.mvm_last_error_string()
    assert lib.mvm_extend_costs(*_cost_args(n_cams=2)) == 2
    assert lib.mvm_extend_costs(*_cost_args(n_scenes=-1)) == 1
    assert lib.mvm_extend_costs(*_cost_args(max_rows=-1)) == 1
    assert lib.mvm_extend_select_triangulate(*_sel_args(n_cams=9)) == 2
    assert lib.mvm_extend_select_triangulate(*_sel_args(n_cams=2)) == 2
    assert lib.mvm_extend_select_triangulate(*_sel_args(n_scenes=-1)) == 1
