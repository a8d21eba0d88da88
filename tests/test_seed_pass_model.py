"""The numpy restatement of the extra seed passes (tests/seed_pass_model.py,
DESIGN §3.16) on hand-built captures with known identity, under the CPU chain
the extension's tests use: the seed-missed objects are found by the extra pass
and by no other, with the right detections -- no GPU."""
import numpy as np
import pytest

import seed_pass_model as M


def _rows_of(p, s):
    return p["orig_views"][int(p["offs"][s]):int(p["offs"][s + 1])]


def _want_row(f, s, obj):
    """The detection of object ``obj`` in every view of capture s (-1: not seen)."""
    row = np.full(f.C, -1, np.int64)
    for c in range(f.C):
        hit = np.nonzero(f.ident[s][c] == obj)[0]
        if hit.size:
            row[c] = hit[0]
    return row


@pytest.fixture(scope="module", params=(5, 6))
def run(request):
    f = M.captures(request.param)
    return f, M.cpu_passes(f, [M.SEED])


def test_the_inputs_hold_what_the_passes_are_about(run):
    f, _ = run
    assert f.S == 8 and sum(len(m) for m in f.missed) >= 6 and sum(len(u) for u in f.under) >= 2
    for s in range(f.S):
        for o in f.missed[s]:
            seen = [c for c in range(f.C) if o in f.ident[s][c]]
            assert sorted(set(range(f.C)) - set(seen)) == [f.miss_cam[s]] and f.miss_cam[s] < 3
            assert all(c in seen for c in M.SEED)
        for o in f.under[s]:
            assert sum(o in f.ident[s][c] for c in range(f.C)) < 3
        assert all((np.bincount(f.ident[s][c], minlength=7)[:M.N_ALL] == 1).all() for c in range(f.C))


def test_pass_0_finds_no_seed_missed_object_and_pass_1_every_one(run):
    f, (p0, p1) = run
    found = 0
    for s in range(f.S):
        rows0, rows1 = _rows_of(p0, s), _rows_of(p1, s)
        # pass 0: the objects every camera sees, each with its own detections in every view
        want0 = sorted(tuple(_want_row(f, s, o)) for o in range(M.N_ALL))
        assert sorted(tuple(r) for r in rows0) == want0, s
        for o in f.missed[s]:
            want = _want_row(f, s, o)
            assert (want >= 0).sum() == f.C - 1
            for c in np.nonzero(want >= 0)[0]:          # none of its detections is in a pass-0 match
                assert want[c] not in rows0[:, c]
            hits = [r for r in rows1 if np.array_equal(r, want)]
            assert len(hits) == 1, (s, o, rows1, want)
            found += 1
    assert found >= 6


def test_no_detection_is_used_twice_and_the_under_seen_stay_unmatched(run):
    f, passes = run
    for s in range(f.S):
        for c in range(f.C):
            held = np.concatenate([_rows_of(p, s)[:, c] for p in passes])
            held = held[held >= 0]
            assert len(np.unique(held)) == len(held), (s, c)
            assert ((0 <= held) & (held < f.counts[s, c])).all()
            for o in f.under[s]:
                for l in np.nonzero(f.ident[s][c] == o)[0]:
                    assert l not in held, (s, c, o)


def test_second_seed_sees_the_first_ones_matches_as_used():
    f = M.captures(5)
    p0, p1, p2 = M.cpu_passes(f, [M.SEED, (1, 3, 4)])
    assert p1["count"].sum() >= 6
    # what pass 1 matched is gone from pass 2's sub-batch: its leftover counts
    # are pass 1's minus the detections pass 1's matches hold
    held1 = (p1["views"] >= 0).sum()
    assert np.diff(p2["sub_offs"]).sum() == np.diff(p1["sub_offs"]).sum() - held1
    for s in range(f.S):
        for c in range(f.C):
            a, b = _rows_of(p1, s)[:, c], _rows_of(p2, s)[:, c]
            assert not set(a[a >= 0]) & set(b[b >= 0])


def test_mark_ignores_what_is_no_index_and_rows_beyond_count():
    cam_offs = np.array([0, 3, 5, 9, 9], np.int64)       # one capture, views of 3, 2, 4, 0
    views = np.array([[0, 1, 3, 0], [2, 2, -1, -1], [M.I32_MIN, 0, 4, 0], [1, 1, 1, 1]], np.int32)
    used = M.mark_used(np.zeros(9, np.int32), views, np.array([0, 4]), np.array([3], np.int32), cam_offs, 4)
    # row 3 is beyond count; 2 of view 1, 4 of view 2 and anything of the empty view are no indices
    assert used.tolist() == [1, 0, 1, 1, 1, 0, 0, 0, 1]
    order = M.seed_order((3, 1, 0), 4)
    assert order == (3, 1, 0, 2)
    assert M.leftover_counts(used, cam_offs, 4, order).tolist() == [0, 0, 1, 3]
    pts = np.arange(18, dtype=np.float64).reshape(9, 2)
    boxes = np.arange(36, dtype=np.int32).reshape(9, 4)
    p, b, orig, so = M.leftover_gather(used, pts, boxes, cam_offs, 4, order)
    assert so.tolist() == [0, 0, 0, 1, 4] and orig.tolist() == [1, 0, 1, 2]
    assert np.array_equal(p, pts[[1, 5, 6, 7]]) and np.array_equal(b, boxes[[1, 5, 6, 7]])
