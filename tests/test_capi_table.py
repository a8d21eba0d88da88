"""mvm_compact_matches (ABI 8): the host-side validation of the match-table
entry point -- no GPU, nothing is launched (the kernel's parity is
tests/test_match_table_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

# the pointer arguments in signature order (n_scenes and scene_base sit after cam_offs_dev)
POINTERS = ["match_dev", "cost_dev", "X_dev", "count_dev", "seg_offs_dev", "pts_dev", "boxes_dev",
            "cam_offs_dev", "dense_offs_dev", "scene_out_dev", "match_out_dev", "cost_out_dev",
            "X_out_dev", "boxes_out_dev", "cent_out_dev"]


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _call(lib, n_scenes, null=None, every=FAKE):
    p = [None if name == null else every for name in POINTERS]
    return lib.mvm_compact_matches(*p[:8], n_scenes, 0, *p[8:], None)


def test_signature_declared(lib):
    assert "mvm_compact_matches" in _native.header_symbols()
    assert len(_native.SIGNATURES["mvm_compact_matches"][1]) == len(POINTERS) + 3
    with open(_native.HEADER_PATH) as fh:
        assert "#define MVM_ABI_VERSION 8" in fh.read()


@pytest.mark.parametrize("name", POINTERS)
def test_null_pointer_names_the_argument(lib, name):
    assert _call(lib, 3, null=name) == 1          # MVM_ERR_INVALID_ARGUMENT
    assert name.encode() in lib.mvm_last_error_string()


def test_empty_batch_launches_nothing(lib):
    # no scenes: ok whatever the pointers are, and no error is left behind
    assert _call(lib, 0, every=None) == 0
    assert _call(lib, 0) == 0
    assert lib.mvm_last_error_string() == b""
    assert _call(lib, -1) == 1
    assert b"n_scenes" in lib.mvm_last_error_string()
