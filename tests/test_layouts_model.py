"""tests/layouts.py on the CPU: every family's regions are disjoint and inside
the buffer, have the residues the family claims, ``reversed`` really runs
downwards, and scatter (``image``) followed by ``gather`` round-trips."""
import numpy as np
import pytest

import layouts as L

SIZES = [
    [16 * 16 * 16, 5 * 3 * 7, 8 * 12 * 4, 0, 1, 12 * 16 * 8],
    [1],
    [0, 0, 3],
    [64, 33, 1000, 7, 260 * 4],
    [],
]


def _units(family):
    if family in L.PHASES:
        return [1]
    return [1, 4] if family == "off_line" else [1, 4, 16, 32]


def _cases():
    for family in L.FAMILIES:
        for unit in _units(family):
            for k, sizes in enumerate(SIZES):
                yield family, unit, k


@pytest.mark.parametrize("family,unit,k", list(_cases()))
def test_regions_disjoint_inside_and_residues(family, unit, k):
    sizes = SIZES[k]
    for seed in range(3):
        lay = L.layout(sizes, family, unit, seed)
        assert lay.offs.dtype == np.int64 and lay.offs.size == len(sizes)
        assert np.array_equal(lay.sizes, np.asarray(sizes, np.int64))
        assert (lay.offs >= 0).all() and (lay.offs + lay.sizes <= lay.total).all()
        assert (lay.offs % unit == 0).all()
        order = lay.order()
        o, n = lay.offs[order], lay.sizes[order]
        assert (o[1:] >= o[:-1] + n[:-1]).all(), "regions overlap"
        if family == "tight":
            # the plan's layout: back to back, each offset rounded up to the unit
            end = 0
            for s, size in enumerate(sizes):
                assert lay.offs[s] == (end + unit - 1) // unit * unit
                end = lay.offs[s] + size
            continue
        # gapped: 1-37 units in front of every region and behind the last
        lo = 0
        for a, b in zip(o, n):
            assert unit <= a - lo, "no gap in front of a region"
            lo = a + b
        assert lay.total - lo >= unit, "no gap behind the last region"
        if family in L.PHASES:
            assert (lay.offs % 4 == L.PHASES[family]).all()
        if family == "off_line":
            assert (lay.offs % 32 == 4).all()
        if family == "reversed" and len(sizes) > 1:
            assert (np.diff(lay.offs) < 0).all(), "region s+1 must lie below region s"
        if family == "gaps" and len(sizes) > 1:
            assert (np.diff(lay.offs) > 0).all()


def test_gaps_stay_within_37_units():
    for family in ("gaps", "reversed"):
        for unit in (1, 16):
            lay = L.layout([5, 0, 40, 7], family, unit, seed=4)
            order = lay.order()
            lo = 0
            for s in order:
                gap = lay.offs[s] - lo
                assert unit <= gap <= L.MAX_GAP * unit + unit - 1
                lo = lay.offs[s] + lay.sizes[s]


def test_seed_changes_the_gaps_and_is_reproducible():
    a = L.layout([10, 20, 30], "gaps", 1, seed=1)
    b = L.layout([10, 20, 30], "gaps", 1, seed=1)
    c = L.layout([10, 20, 30], "gaps", 1, seed=2)
    assert np.array_equal(a.offs, b.offs) and a.total == b.total
    assert not np.array_equal(a.offs, c.offs)


def test_bad_arguments():
    with pytest.raises(ValueError):
        L.layout([1], "phase1", unit=4)
    with pytest.raises(ValueError):
        L.layout([1], "off_line", unit=16)
    with pytest.raises(ValueError):
        L.layout([1], "zigzag")
    with pytest.raises(ValueError):
        L.layout([-1], "gaps")


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64, np.uint16, np.int16,
                                   np.uint8])
@pytest.mark.parametrize("family", L.FAMILIES)
def test_scatter_gather_round_trip(family, dtype):
    rng = np.random.default_rng(3)
    sizes = [7, 0, 130, 1, 64]
    lay = L.layout(sizes, family, 1, seed=5)
    regions = [rng.integers(0, 100, size=n).astype(dtype) for n in sizes]
    regions[3] = None                                   # left as sentinel
    img = L.image(lay, dtype, regions, tail=9)
    assert img.size == lay.total + 9 and img.dtype == np.dtype(dtype)
    back = L.gather(img, lay)
    sent = L.blank(1, dtype)
    covered = np.zeros(img.size, bool)
    for s, (r, g) in enumerate(zip(regions, back)):
        covered[lay.offs[s]:lay.offs[s] + sizes[s]] = True
        want = r if r is not None else np.full(sizes[s], sent[0], dtype)
        assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), s
    # everything outside the regions is the sentinel, bit for bit
    rest = img[~covered]
    assert np.array_equal(rest.view(np.uint8), np.full(rest.size, sent[0], dtype).view(np.uint8))


def test_sentinels_are_what_no_kernel_writes():
    f32 = L.blank(1, np.float32)
    f64 = L.blank(1, np.float64)
    assert np.isfinite(f32[0]) and int(f32.view(np.uint32)[0]) & 1
    assert np.isfinite(f64[0]) and int(f64.view(np.uint64)[0]) & 1
    assert int(L.blank(1, np.int32)[0]) == -2 ** 31 + 7
    assert int(L.blank(1, np.uint16)[0]) == 0x5A5A
    assert int(L.blank(1, np.int16).view(np.uint16)[0]) == 0x5A5A


def test_first_diff_names_index_and_place():
    lay = L.layout([10, 6], "gaps", 1, seed=0)
    want = L.image(lay, np.float32, [np.arange(10, dtype=np.float32), np.zeros(6, np.float32)])
    assert L.first_diff(want.copy(), want, lay) is None
    got = want.copy()
    got[lay.offs[1] + 2] = 5.0
    msg = L.first_diff(got, want, lay, "cube")
    assert f"first at {lay.offs[1] + 2}" in msg and "region 1 (+2 of 6" in msg and "cube [gaps]" in msg
    got = want.copy()
    got[lay.offs[0] + 10] = 1.0                          # one past region 0: the gap below region 1
    assert "below region 1" in L.first_diff(got, want, lay)
    got = want.copy()
    got[-1] = 1.0
    assert "tail" in L.first_diff(got, want, lay)
    # bit patterns: NaN equals NaN, -0 differs from +0
    a = np.array([np.nan, 0.0], np.float32)
    lay2 = L.layout([2], "tight")
    assert L.first_diff(a.copy(), a, lay2) is None
    assert L.first_diff(np.array([np.nan, -0.0], np.float32), a, lay2) is not None
    with pytest.raises(AssertionError, match="region 1"):
        bad = want.copy()
        bad[lay.offs[1]] = 9.0
        L.assert_image(bad, want, lay)
