"""mvm_mark_used, mvm_leftover_counts, mvm_leftover_gather (additions to ABI 8,
MVM_HAS_LEFTOVERS): the host-side validation of the leftover entry points --
no GPU, nothing is launched (the kernels' parity is tests/test_leftovers_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first
NAMES = ("mvm_mark_used", "mvm_leftover_counts", "mvm_leftover_gather")

# the pointer arguments of each entry point, in signature order
POINTERS = {
    "mvm_mark_used": ["views_dev", "match_offs_dev", "count_dev", "cam_offs_dev", "used_dev"],
    "mvm_leftover_counts": ["used_dev", "cam_offs_dev", "counts_dev"],
    "mvm_leftover_gather": ["used_dev", "pts_dev", "boxes_dev", "cam_offs_dev", "sub_cam_offs_dev",
                            "pts_out_dev", "boxes_out_dev", "orig_out_dev"],
}


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _call(lib, name, n_scenes=3, n_cams=5, seed=(2, 3, 4), null=None, every=FAKE, sub=None, orig=None):
    p = {k: (None if k == null else every) for k in POINTERS[name]}
    if name == "mvm_mark_used":
        return lib.mvm_mark_used(p["views_dev"], p["match_offs_dev"], p["count_dev"], 10, n_scenes, n_cams,
                                 *seed, sub, orig, p["cam_offs_dev"], 40, p["used_dev"], None)
    if name == "mvm_leftover_counts":
        return lib.mvm_leftover_counts(p["used_dev"], p["cam_offs_dev"], n_scenes, n_cams, *seed,
                                       p["counts_dev"], None)
    return lib.mvm_leftover_gather(p["used_dev"], p["pts_dev"], p["boxes_dev"], p["cam_offs_dev"],
                                   p["sub_cam_offs_dev"], n_scenes, n_cams, *seed, p["pts_out_dev"],
                                   p["boxes_out_dev"], p["orig_out_dev"], None)


def test_signatures_declared(lib):
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_ABI_VERSION 8" in text
    assert "#define MVM_HAS_LEFTOVERS 1" in text
    syms = [s for s in _native.header_symbols() if s in _native.SIGNATURES]
    for name in NAMES:
        assert name in _native.header_symbols() and hasattr(lib, name)
        # the order of the header is the order of the binding
        assert syms.index(name) == list(_native.SIGNATURES).index(name)
    assert [len(_native.SIGNATURES[n][1]) for n in NAMES] == [15, 9, 14]


@pytest.mark.parametrize("name,ptr", [(n, p) for n in NAMES for p in POINTERS[n]])
def test_null_pointer_names_the_argument(lib, name, ptr):
    assert _call(lib, name, null=ptr) == 1                # MVM_ERR_INVALID_ARGUMENT
    assert lib.mvm_last_error_string().endswith(b" " + ptr.encode())


def test_mark_used_takes_sub_offsets_and_orig_together(lib):
    assert _call(lib, "mvm_mark_used", sub=FAKE) == 1
    assert b"go together" in lib.mvm_last_error_string()
    assert _call(lib, "mvm_mark_used", orig=FAKE) == 1
    # both, or neither: the call gets as far as the pointer check
    for both in (FAKE, None):
        assert _call(lib, "mvm_mark_used", sub=both, orig=both, null="used_dev") == 1
        assert lib.mvm_last_error_string().endswith(b" used_dev")


@pytest.mark.parametrize("n_cams", [3, 9])
@pytest.mark.parametrize("name", NAMES)
def test_n_cams_outside_the_range_is_refused(lib, name, n_cams):
    assert _call(lib, name, n_cams=n_cams, seed=(0, 1, 2)) != 0
    msg = lib.mvm_last_error_string()
    assert b"n_cams" in msg and str(n_cams).encode() in msg


@pytest.mark.parametrize("seed", [(2, 2, 4), (2, 3, 2), (4, 3, 3), (2, 3, 5), (-1, 3, 4), (2, 8, 4)])
@pytest.mark.parametrize("name", NAMES)
def test_triple_with_a_repeated_or_out_of_range_camera_is_refused(lib, name, seed):
    assert _call(lib, name, seed=seed) == 1
    assert b"seed" in lib.mvm_last_error_string()


@pytest.mark.parametrize("name", NAMES)
def test_no_captures_is_ok(lib, name):
    # nothing to launch whatever the pointers, n_cams and the triple are, and no error is left behind
    assert _call(lib, name, n_scenes=0, every=None) == 0
    assert _call(lib, name, n_scenes=0, n_cams=9, seed=(1, 1, 1)) == 0
    assert lib.mvm_last_error_string() == b""
    assert _call(lib, name, n_scenes=-1) == 1
    assert b"n_scenes" in lib.mvm_last_error_string()
