"""mvm_fit_boxes (an addition to ABI 8, MVM_HAS_BOX_FIT): the host-side
validation of the entry point -- no GPU, nothing is launched (the kernel's
parity is tests/test_box_fit_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = 0x10000                   # never dereferenced: validation fails first

# the pointer arguments in signature order
POINTERS = ["pose_dev", "scene_dev", "views_dev", "boxes_dev", "proj_dev", "verts_dev", "pose_out_dev", "rms_dev",
            "info_dev", "cov_dev", "resid_dev"]
OPTIONAL = ["cov_dev", "resid_dev"]
REQUIRED = [p for p in POINTERS if p not in OPTIONAL]
DEFAULTS = dict(scene_base=0, n_rows=5, n_cams=4, n_scenes=2, n_verts=8, max_evals=10)


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _fit(lib, null=(), every=True, ptrs=None, **kw):
    a = dict(DEFAULTS, **kw)
    null = (null,) if isinstance(null, str) else null
    # distinct addresses 1 MiB apart: nothing overlaps unless a test says so
    p = {name: (None if name in null or not every else ctypes.c_void_p(FAKE + (i << 20)))
         for i, name in enumerate(POINTERS)}
    p.update(ptrs or {})
    return lib.mvm_fit_boxes(p["pose_dev"], p["scene_dev"], a["scene_base"], p["views_dev"], p["boxes_dev"],
                             a["n_rows"], a["n_cams"], p["proj_dev"], a["n_scenes"], p["verts_dev"], a["n_verts"],
                             a["max_evals"], p["pose_out_dev"], p["rms_dev"], p["info_dev"], p["cov_dev"],
                             p["resid_dev"], None)


def _reaches_the_pointer_check(lib, **kw):
    """Valid arguments get as far as the pointers: the null one is named."""
    assert _fit(lib, null="info_dev", **kw) == 1
    return lib.mvm_last_error_string().endswith(b" info_dev")


def test_signature_declared(lib):
    assert "mvm_fit_boxes" in _native.header_symbols()
    assert hasattr(lib, "mvm_fit_boxes")
    assert len(_native.SIGNATURES["mvm_fit_boxes"][1]) == 18
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_ABI_VERSION 8" in text
    assert "#define MVM_HAS_BOX_FIT 1" in text
    # the order of the header is the order of the binding, right behind the symmetric mean
    syms = [s for s in _native.header_symbols() if s in _native.SIGNATURES]
    names = list(_native.SIGNATURES)
    assert syms.index("mvm_fit_boxes") == names.index("mvm_fit_boxes") == names.index("mvm_fuse_rotations_sym") + 1


@pytest.mark.parametrize("name", REQUIRED)
def test_null_pointer_names_the_argument(lib, name):
    assert _fit(lib, null=name) == 1                      # MVM_ERR_INVALID_ARGUMENT
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


def test_cov_and_resid_are_optional(lib):
    # with both NULL the call still gets as far as naming another null pointer
    assert _fit(lib, null=OPTIONAL + ["info_dev"]) == 1
    assert lib.mvm_last_error_string().endswith(b" info_dev")


@pytest.mark.parametrize("key, bad, good, status", [
    ("n_cams", 2, 3, 2), ("n_cams", 9, 8, 2),                             # MVM_ERR_UNSUPPORTED
    ("n_verts", 0, 1, 1), ("max_evals", 0, 1, 1), ("max_evals", 65, 64, 1),
    ("n_rows", -1, 1, 1), ("n_scenes", -1, 0, 1),
])
def test_each_range_end(lib, key, bad, good, status):
    assert _fit(lib, **{key: bad}) == status
    msg = lib.mvm_last_error_string()
    assert key.encode() in msg and str(bad).encode() in msg
    assert _reaches_the_pointer_check(lib, **{key: good})


def test_more_rows_than_a_grid_holds(lib):
    per_grid = 0xFFFFFFFF // 256 * 4
    assert _fit(lib, n_rows=per_grid + 1) == 2
    assert b"n_rows" in lib.mvm_last_error_string() and b"split" in lib.mvm_last_error_string()
    assert _fit(lib, n_rows=2 ** 62) == 2
    assert _reaches_the_pointer_check(lib, n_rows=per_grid)


def test_pose_out_must_not_overlap_pose(lib):
    rows, size = 5, 5 * 16 * 8
    base = FAKE + (40 << 20)
    for off in (0, 8, size - 8, -(size - 8)):
        ptrs = dict(pose_dev=ctypes.c_void_p(base), pose_out_dev=ctypes.c_void_p(base + off))
        assert _fit(lib, n_rows=rows, ptrs=ptrs) == 1
        assert b"pose_out_dev overlaps pose_dev" in lib.mvm_last_error_string()
    # back to back is no overlap: tests/test_box_fit_gpu.py runs it


def test_no_rows_launches_nothing(lib):
    # ok whatever the other arguments are, and no error is left behind
    assert _fit(lib, n_rows=0, every=False) == 0
    assert _fit(lib, n_rows=0) == 0
    assert _fit(lib, n_rows=0, n_cams=99, n_verts=-4, max_evals=0, n_scenes=-1) == 0
    assert lib.mvm_last_error_string() == b""
