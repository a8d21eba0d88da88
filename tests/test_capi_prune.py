"""mvm_prune_views_triangulate (an addition to ABI 8, MVM_HAS_VIEW_PRUNE): the
host-side validation of the view-pruning entry point -- no GPU, nothing is
launched (the kernel's parity is tests/test_view_prune_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

# the pointer arguments in signature order (n_scenes, n_cams sit after count_dev, gate after proj_dev)
HEAD = ["match_offs_dev", "count_dev"]
MID = ["pts_dev", "cam_offs_dev", "proj_dev"]
TAIL = ["views_dev", "ext_cost_dev", "X_dev", "pruned_dev"]
POINTERS = HEAD + MID + TAIL


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _call(lib, n_scenes, n_cams=4, gate=3.0, null=None, every=FAKE):
    p = {name: (None if name == null else every) for name in POINTERS}
    return lib.mvm_prune_views_triangulate(*[p[k] for k in HEAD], n_scenes, n_cams, *[p[k] for k in MID],
                                           gate, *[p[k] for k in TAIL], None)


def test_signature_declared(lib):
    assert "mvm_prune_views_triangulate" in _native.header_symbols()
    assert hasattr(lib, "mvm_prune_views_triangulate")
    assert len(_native.SIGNATURES["mvm_prune_views_triangulate"][1]) == len(POINTERS) + 4
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_ABI_VERSION 8" in text
    assert "#define MVM_HAS_VIEW_PRUNE 1" in text
    # the order of the header is the order of the binding
    syms = [s for s in _native.header_symbols() if s in _native.SIGNATURES]
    assert syms.index("mvm_prune_views_triangulate") == list(_native.SIGNATURES).index(
        "mvm_prune_views_triangulate")


@pytest.mark.parametrize("n_cams", [4, 8])
@pytest.mark.parametrize("name", POINTERS)
def test_null_pointer_names_the_argument(lib, name, n_cams):
    assert _call(lib, 3, n_cams, null=name) == 1          # MVM_ERR_INVALID_ARGUMENT
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


@pytest.mark.parametrize("n_cams", [3, 9, 0, -1])
def test_n_cams_outside_the_range_is_refused(lib, n_cams):
    assert _call(lib, 3, n_cams) != 0
    msg = lib.mvm_last_error_string()
    assert b"n_cams" in msg and str(n_cams).encode() in msg


@pytest.mark.parametrize("gate", [float("nan"), -1.0, -1e-300, float("-inf")])
def test_gate_that_is_no_distance_is_refused(lib, gate):
    assert _call(lib, 3, gate=gate) == 1
    assert b"gate" in lib.mvm_last_error_string()


def test_gates_at_the_ends_of_the_range_pass_validation(lib):
    # 0 and +inf are gates: the call gets as far as the pointer check
    for gate in (0.0, float("inf")):
        assert _call(lib, 3, gate=gate, null="pruned_dev") == 1
        assert lib.mvm_last_error_string().endswith(b" pruned_dev")


def test_empty_batch_launches_nothing(lib):
    # no captures: ok whatever the pointers, n_cams and gate are, and no error is left behind
    assert _call(lib, 0, every=None) == 0
    assert _call(lib, 0) == 0
    assert _call(lib, 0, n_cams=9, gate=-1.0) == 0
    assert lib.mvm_last_error_string() == b""
    assert _call(lib, -1) == 1
    assert b"n_scenes" in lib.mvm_last_error_string()
