"""mvm_refine_points (an addition to ABI 8, MVM_HAS_REFINE): the host-side
validation of the point-refinement entry point -- no GPU, nothing is launched
(the kernel's parity is tests/test_refine_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

# the pointer arguments in signature order (n_scenes, n_cams sit after count_dev, max_evals after X_dev)
HEAD = ["match_offs_dev", "count_dev"]
MID = ["pts_dev", "cam_offs_dev", "proj_dev", "views_dev", "X_dev"]
TAIL = ["X_out_dev", "rms_dev", "info_dev", "cov_dev"]
POINTERS = HEAD + MID + TAIL
REQUIRED = [p for p in POINTERS if p != "cov_dev"]


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _call(lib, n_scenes, n_cams=4, max_evals=10, null=None, every=FAKE):
    p = {name: (None if name == null else every) for name in POINTERS}
    return lib.mvm_refine_points(*[p[k] for k in HEAD], n_scenes, n_cams, *[p[k] for k in MID], max_evals,
                                 *[p[k] for k in TAIL], None)


def test_signature_declared(lib):
    assert "mvm_refine_points" in _native.header_symbols()
    assert hasattr(lib, "mvm_refine_points")
    assert len(_native.SIGNATURES["mvm_refine_points"][1]) == len(POINTERS) + 4
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_ABI_VERSION 8" in text
    assert "#define MVM_HAS_REFINE 1" in text
    # the order of the header is the order of the binding
    syms = [s for s in _native.header_symbols() if s in _native.SIGNATURES]
    assert syms.index("mvm_refine_points") == list(_native.SIGNATURES).index("mvm_refine_points")


@pytest.mark.parametrize("n_cams", [3, 8])
@pytest.mark.parametrize("name", REQUIRED)
def test_null_pointer_names_the_argument(lib, name, n_cams):
    assert _call(lib, 3, n_cams, null=name) == 1          # MVM_ERR_INVALID_ARGUMENT
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


@pytest.mark.parametrize("n_cams", [2, 9, 0, -1])
def test_n_cams_outside_the_range_is_refused(lib, n_cams):
    assert _call(lib, 3, n_cams) != 0
    msg = lib.mvm_last_error_string()
    assert b"n_cams" in msg and str(n_cams).encode() in msg


@pytest.mark.parametrize("max_evals", [0, 65, -1])
def test_max_evals_outside_the_range_is_refused(lib, max_evals):
    assert _call(lib, 3, max_evals=max_evals) == 1
    msg = lib.mvm_last_error_string()
    assert b"max_evals" in msg and str(max_evals).encode() in msg


def test_the_ends_of_the_ranges_pass_validation(lib):
    # 1 and 64 evaluations, 3 and 8 cameras: the call gets as far as the pointer check
    for n_cams, max_evals in ((3, 1), (8, 64)):
        assert _call(lib, 3, n_cams, max_evals, null="info_dev") == 1
        assert lib.mvm_last_error_string().endswith(b" info_dev")


def test_empty_batch_launches_nothing(lib):
    # no captures: ok whatever the pointers, n_cams and max_evals are, and no error is left behind
    assert _call(lib, 0, every=None) == 0
    assert _call(lib, 0) == 0
    assert _call(lib, 0, n_cams=9, max_evals=0) == 0
    assert lib.mvm_last_error_string() == b""
    assert _call(lib, -1) == 1
    assert b"n_scenes" in lib.mvm_last_error_string()
