"""mvm_rig_matrices (an addition to ABI 8): the host-side validation of the
device F / P entry point -- no GPU, nothing is launched (the kernel's parity is
tests/test_rig_matrices_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

# the pointer arguments in signature order (the three sizes sit after pair_b)
POINTERS = ["K_dev", "RT_dev", "pair_a", "pair_b", "F_dev", "proj_dev", "status_dev"]


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _pairs(pairs):
    a = (ctypes.c_int32 * len(pairs))(*[p[0] for p in pairs])
    b = (ctypes.c_int32 * len(pairs))(*[p[1] for p in pairs])
    return a, b


def _call(lib, n_scenes, n_cams=3, pairs=((0, 1), (0, 2), (1, 2)), null=None, n_pairs=None):
    pa, pb = _pairs(pairs)
    p = {name: FAKE for name in POINTERS}
    p["pair_a"], p["pair_b"] = pa, pb
    if null is not None:
        p[null] = None
    return lib.mvm_rig_matrices(p["K_dev"], p["RT_dev"], p["pair_a"], p["pair_b"], n_scenes, n_cams,
                                len(pairs) if n_pairs is None else n_pairs, p["F_dev"], p["proj_dev"],
                                p["status_dev"], None)


def test_signature_declared(lib):
    assert "mvm_rig_matrices" in _native.header_symbols()
    assert len(_native.SIGNATURES["mvm_rig_matrices"][1]) == len(POINTERS) + 4
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_HAS_RIG_MATRICES 1" in text
    assert "#define MVM_ABI_VERSION 8" in text      # additive: the ABI number stays


@pytest.mark.parametrize("name", [n for n in POINTERS if n != "proj_dev"])
def test_null_pointer_names_the_argument(lib, name):
    assert _call(lib, 3, null=name) == 1          # MVM_ERR_INVALID_ARGUMENT
    assert name.encode() in lib.mvm_last_error_string()


@pytest.mark.parametrize("n_cams", [0, 1, 9])
def test_camera_count_out_of_range(lib, n_cams):
    assert _call(lib, 3, n_cams=n_cams, pairs=((0, 1),)) != 0
    assert b"n_cams" in lib.mvm_last_error_string()


def test_too_many_pairs(lib):
    pairs = [(a, b) for a in range(8) for b in range(a + 1, 8)] + [(1, 0)]
    assert len(pairs) == 29
    assert _call(lib, 3, n_cams=8, pairs=pairs) != 0
    assert b"n_pairs" in lib.mvm_last_error_string()
    assert _call(lib, 3, n_pairs=0) != 0


@pytest.mark.parametrize("pair", [(1, 1), (0, 3), (-1, 2), (3, 0)])
def test_bad_pair(lib, pair):
    assert _call(lib, 3, pairs=((0, 1), pair)) == 1
    assert b"pair 1" in lib.mvm_last_error_string()


def test_empty_batch_launches_nothing(lib):
    # no captures: ok whatever the other arguments are, and no error is left behind
    assert lib.mvm_rig_matrices(None, None, None, None, 0, 0, 0, None, None, None, None) == 0
    assert _call(lib, 0) == 0
    assert lib.mvm_last_error_string() == b""
    assert _call(lib, -1) == 1
    assert b"n_scenes" in lib.mvm_last_error_string()
