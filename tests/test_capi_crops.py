"""mvm_crop_views (an addition to ABI 8, MVM_HAS_CROPS): the host-side
validation of the crop entry point -- no GPU, nothing is launched (the
kernel's parity is tests/test_crop_gpu.py)."""
import ctypes

import pytest

from bpc_baseline_amd import _native

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first

# the pointer arguments in signature order
POINTERS = ["images_dev", "scene_dev", "views_dev", "boxes_dev", "cams_host", "lut_dev", "out_dev", "geom_dev"]
REQUIRED = [p for p in POINTERS if p != "geom_dev"]
DEFAULTS = dict(n_scenes=2, n_cams=4, img_h=48, img_w=64, scene_base=0, row0=0, n_rows=3, size=16, fill=255,
                out_kind=0)


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _call(lib, null=None, every=FAKE, cams=(0, 1), out=None, **kw):
    a = dict(DEFAULTS, **kw)
    p = {name: (None if name == null else every) for name in POINTERS}
    if out is not None:
        p["out_dev"] = out
    if p["cams_host"] is not None:
        p["cams_host"] = (ctypes.c_int32 * max(len(cams), 1))(*cams)
    return lib.mvm_crop_views(p["images_dev"], a["n_scenes"], a["n_cams"], a["img_h"], a["img_w"],
                              p["scene_dev"], a["scene_base"], p["views_dev"], p["boxes_dev"], a["row0"],
                              a["n_rows"], p["cams_host"], a.get("n_sel", len(cams)), a["size"], a["fill"],
                              p["lut_dev"], a["out_kind"], p["out_dev"], p["geom_dev"], None)


def _reaches_the_pointer_check(lib, **kw):
    """Valid arguments get as far as the pointers: the null one is named."""
    assert _call(lib, null="out_dev", **kw) == 1
    return lib.mvm_last_error_string().endswith(b" out_dev")


def test_signature_declared(lib):
    assert "mvm_crop_views" in _native.header_symbols()
    assert hasattr(lib, "mvm_crop_views")
    assert len(_native.SIGNATURES["mvm_crop_views"][1]) == 20
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define MVM_ABI_VERSION 8" in text
    assert "#define MVM_HAS_CROPS 1" in text
    # the order of the header is the order of the binding
    syms = [s for s in _native.header_symbols() if s in _native.SIGNATURES]
    assert syms.index("mvm_crop_views") == list(_native.SIGNATURES).index("mvm_crop_views")


@pytest.mark.parametrize("name", REQUIRED)
def test_null_pointer_names_the_argument(lib, name):
    assert _call(lib, null=name) == 1                     # MVM_ERR_INVALID_ARGUMENT
    assert lib.mvm_last_error_string().endswith(b" " + name.encode())


def test_geom_is_optional(lib):
    # with geom_dev NULL the call still gets as far as naming another null pointer
    p = {name: FAKE for name in POINTERS}
    cams = (ctypes.c_int32 * 2)(0, 1)
    a = DEFAULTS
    assert lib.mvm_crop_views(p["images_dev"], a["n_scenes"], a["n_cams"], a["img_h"], a["img_w"], FAKE, 0, FAKE,
                              FAKE, 0, 3, cams, 2, 16, 255, FAKE, 0, None, None, None) == 1
    assert lib.mvm_last_error_string().endswith(b" out_dev")


@pytest.mark.parametrize("key, bad, good", [
    ("n_cams", 2, 3), ("n_cams", 9, 8),
    ("size", 0, 1), ("size", 1025, 1024),
    ("img_h", 0, 1), ("img_h", 16385, 16384),
    ("img_w", 0, 1), ("img_w", 16385, 16384),
    ("fill", -1, 0), ("fill", 256, 255),
    ("out_kind", -1, 0), ("out_kind", 2, 1),
    ("row0", -1, 0), ("n_rows", -1, 1),
])
def test_each_range_end(lib, key, bad, good):
    assert _call(lib, **{key: bad}) != 0
    msg = lib.mvm_last_error_string()
    assert key.encode() in msg and str(bad).encode() in msg
    assert _reaches_the_pointer_check(lib, **{key: good})


def test_the_selected_cameras(lib):
    assert _call(lib, cams=(), n_sel=0) == 1
    assert b"n_sel" in lib.mvm_last_error_string()
    assert _call(lib, cams=(0, 1, 2, 3, 0), n_cams=4) == 1            # more than n_cams
    assert b"n_sel" in lib.mvm_last_error_string()
    assert _reaches_the_pointer_check(lib, cams=(2,))
    assert _reaches_the_pointer_check(lib, cams=(3, 1, 0, 2), n_cams=4)
    assert _reaches_the_pointer_check(lib, cams=tuple(range(8)), n_cams=8)
    for cams, n_cams in (((0, 4), 4), ((3,), 3), ((-1,), 4), ((0, 8), 8)):
        assert _call(lib, cams=cams, n_cams=n_cams) == 1
        msg = lib.mvm_last_error_string()
        assert b"cams_host" in msg and str(cams[-1]).encode() in msg
    assert _reaches_the_pointer_check(lib, cams=(0, 3), n_cams=4)


def test_no_rows_launches_nothing(lib):
    # ok whatever the other arguments are, and no error is left behind
    assert _call(lib, n_rows=0, every=None) == 0
    assert _call(lib, n_rows=0) == 0
    assert _call(lib, n_rows=0, n_cams=9, size=0, fill=700, img_h=-3, out_kind=5, cams=(11,)) == 0
    assert lib.mvm_last_error_string() == b""


KMAX_GRID_BLOCKS = 16777215          # kMaxGridBlocks: what one launch holds


@pytest.mark.parametrize("size, out, n_rows, blocks", [
    (1024, 0x1000, 8192, 256),       # aligned: 4096 pixels a workgroup
    (1024, 0x1004, 2048, 1024),      # unaligned: 1024 pixels a workgroup
    (1023, 0x1000, 2051, 1023),      # an odd side writes elements wherever it starts
])
def test_more_crops_than_one_launch_holds(lib, size, out, n_rows, blocks):
    """Each is the first row count refused: nothing is launched, so the fake
    pointers are never read.  (The accepted side would launch: not called.)"""
    assert blocks == -(-size * size // (4096 if size % 2 == 0 and out % 16 == 0 else 1024))
    assert n_rows * 8 * blocks > KMAX_GRID_BLOCKS >= (n_rows - 1) * 8 * blocks
    assert _call(lib, cams=tuple(range(8)), n_cams=8, size=size, n_rows=n_rows, out=ctypes.c_void_p(out)) == 2
    msg = lib.mvm_last_error_string()                     # MVM_ERR_UNSUPPORTED
    assert b"n_rows=%d" % n_rows in msg and b"split the rows" in msg
