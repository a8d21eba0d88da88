"""Extra seed passes (match_captures(extra_seeds=[...])) restated
in numpy -- the normative statement of what mvm_mark_used, mvm_leftover_counts,
mvm_leftover_gather and MatchBatch.table_all compute -- and the hand-built
captures the CPU and GPU tests share.

Pass 0 is the call without the keyword.  Pass p >= 1 with triple (a, b, c):

  1. detection l of camera c of capture s is USED if it occurs as views[w][c]
     of a match row w < count[s] of an earlier pass (after that pass's gate);
     an entry that is negative or no index of its view marks nothing.  The
     LEFTOVERS of a view are its unused detections, ascending.
  2. pi = (a, b, c, then the other cameras ascending); the sub-batch holds for
     capture s and slot q the leftovers of camera pi[q]: pts, boxes, cam_offs
     over the leftover counts, orig = each one's index in its original view.
  3. Ks / RTs permuted by pi; F and P of extension_pairs(C) of that rig.
  4. the C-camera path, unchanged, on the sub-batch.
"""
import functools

import numpy as np

from bpc_baseline_amd.synth import make_rig

I32_MIN = -2 ** 31


def seed_order(seed, C):
    seed = tuple(int(c) for c in seed)
    assert len(set(seed)) == 3 and all(0 <= c < C for c in seed)
    return seed + tuple(c for c in range(C) if c not in seed)


def mark_used(used, views, match_offs, count, cam_offs, C, order=None, sub_offs=None, orig=None):
    """``used`` (int32, one per detection of the C-camera CSR ``cam_offs``)
    with 1 written for every detection a match row names; in place.  ``views``
    [cap, C] in slot order of ``order`` (default: the identity); with
    ``sub_offs`` / ``orig`` its entries index the pass's own views."""
    order = tuple(range(C)) if order is None else order
    for s in range(len(count)):
        n = min(int(count[s]), int(match_offs[s + 1] - match_offs[s]))
        for w in range(max(n, 0)):
            for q in range(C):
                v = int(views[match_offs[s] + w, q])
                if sub_offs is not None:
                    so = int(sub_offs[s * C + q])
                    if not 0 <= v < int(sub_offs[s * C + q + 1]) - so:
                        continue
                    v = int(orig[so + v])
                o = int(cam_offs[s * C + order[q]])
                if 0 <= v < int(cam_offs[s * C + order[q] + 1]) - o:
                    used[o + v] = 1
    return used


def leftover_counts(used, cam_offs, C, order):
    """int32 [C S], slot order."""
    S = (len(cam_offs) - 1) // C
    out = np.zeros(S * C, np.int32)
    for s in range(S):
        for q in range(C):
            o, e = cam_offs[s * C + order[q]], cam_offs[s * C + order[q] + 1]
            out[s * C + q] = int((used[o:e] == 0).sum())
    return out


def leftover_gather(used, pts, boxes, cam_offs, C, order):
    """-> (pts f64 [m, 2], boxes int32 [m, 4], orig int32 [m], sub_offs int64 [C S + 1])."""
    S = (len(cam_offs) - 1) // C
    sub_offs = np.zeros(S * C + 1, np.int64)
    np.cumsum(leftover_counts(used, cam_offs, C, order), out=sub_offs[1:])
    rows, orig = [], []
    for s in range(S):
        for q in range(C):
            o, e = int(cam_offs[s * C + order[q]]), int(cam_offs[s * C + order[q] + 1])
            left = np.nonzero(used[o:e] == 0)[0]
            rows.append(o + left)
            orig.append(left)
    rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    orig = np.concatenate(orig).astype(np.int32) if orig else np.zeros(0, np.int32)
    return pts[rows].reshape(-1, 2), boxes[rows].reshape(-1, 4), orig, sub_offs


def merged_table(tables, orders, origs, sub_offs, C):
    """The merged table of MatchBatch.table_all from the passes' own tables
    (dicts of host arrays with ``offs``, slot order; pass 0 first: its order,
    orig and sub_offs are None).  Per capture pass 0's rows, then pass 1's ...;
    per-camera columns in original camera order, views through orig,
    ext_cost in slot order, match of a later pass = the seed triple's original
    indices, seed_pass = the pass index."""
    S = len(tables[0]["offs"]) - 1
    conv = []
    for p, t in enumerate(tables):
        t = {k: np.array(v) for k, v in t.items()}
        if orders[p] is not None:
            order, views = orders[p], t["views"].copy()
            for r in range(len(views)):
                s = int(t["scene"][r])
                for q in range(C):
                    if views[r, q] >= 0:
                        views[r, q] = origs[p][sub_offs[p][s * C + q] + views[r, q]]
            inv = np.argsort(order)
            for k in ("boxes", "centroids", "reproj"):
                t[k] = t[k][:, inv]
            t["views"] = views[:, inv]
            t["match"] = t["views"][:, list(order[:3])]
        t["seed_pass"] = np.full(len(t["scene"]), p, np.int32)
        conv.append(t)
    keys = [k for k in conv[0] if k != "offs"]
    out = {k: [] for k in keys}
    offs = np.zeros(S + 1, np.int64)
    for s in range(S):
        for t in conv:
            a, b = int(t["offs"][s]), int(t["offs"][s + 1])
            for k in keys:
                out[k].append(t[k][a:b])
            offs[s + 1] += b - a
    np.cumsum(offs, out=offs)
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["offs"] = offs
    return out


# ------------------------------------------------------------- the inputs ----
SEED = (2, 3, 4)
N_CAPTURES = 8
N_ALL, N_UNDER = 5, 1          # objects every camera sees; objects only cameras 0 and 3 see


class Captures:
    pass


def _project(K, RT, X):
    cam = X @ RT[:3, :3].T + RT[:3, 3]
    uv = cam @ K.astype(np.float64).T
    return uv[:, :2] / uv[:, 2:3]


# the generator seeds: the first ones under which the CPU chain alone meets the
# conditions tests/test_seed_pass_model.py states on the inputs (pass 0 matches
# exactly the objects every camera sees, so no seed-missed detection is taken
# by a chance match below the threshold)
RNG_SEEDS = {5: 7127, 6: 7131}


@functools.lru_cache(maxsize=None)
def captures(C, rng_seed=None):
    """8 captures of C cameras with known identity.  Capture s holds N_ALL
    objects every camera sees, one that exactly one of cameras 0 and 1 misses
    (camera s % 2; every other camera, so all of SEED, sees it) and N_UNDER
    that only cameras 0 and 3 see.  Objects are projected exactly, the boxes
    are integers around the projection plus 0.3 px of noise, and every view is
    shuffled.  ``ident[s][c]``: the object of each detection of the view;
    ``missed`` / ``under``: per capture the object ids of the two kinds."""
    rng = np.random.default_rng(RNG_SEEDS[C] if rng_seed is None else rng_seed)
    S = N_CAPTURES
    f = Captures()
    f.S, f.C = S, C
    f.Ks, f.RTs = np.zeros((S, C, 3, 3), np.float32), np.zeros((S, C, 4, 4))
    f.ident, f.missed, f.under, f.miss_cam = [], [], [], []
    boxes, counts = [], []
    for s in range(S):
        Ks, RTs = make_rig(rng, C)
        f.Ks[s], f.RTs[s] = np.stack(Ks), np.stack(RTs)
        n_obj = N_ALL + 1 + N_UNDER
        X = np.stack([rng.uniform(-250, 250, n_obj), rng.uniform(-250, 250, n_obj),
                      rng.uniform(-80, 80, n_obj)], axis=1)
        missed, under = N_ALL, list(range(N_ALL + 1, n_obj))
        f.missed.append([missed])
        f.under.append(under)
        f.miss_cam.append(s % 2)
        ident = []
        for c in range(C):
            seen = [o for o in range(n_obj)
                    if not (o == missed and c == s % 2) and not (o in under and c not in (0, 3))]
            seen = np.asarray(seen, np.int64)[rng.permutation(len(seen))]
            uv = _project(f.Ks[s, c], f.RTs[s, c], X[seen]) + rng.normal(0.0, 0.3, (len(seen), 2))
            half = rng.integers(20, 50, (len(seen), 2)).astype(np.float64)
            boxes.append(np.trunc(np.concatenate([uv - half, uv + half], axis=1)))
            counts.append(len(seen))
            ident.append(seen)
        f.ident.append(ident)
    f.boxes = np.concatenate(boxes).astype(np.float32)
    f.conf = np.full(len(f.boxes), 0.9, np.float32)
    f.cls = np.zeros(len(f.boxes), np.float32)
    f.img_offs = np.zeros(S * C + 1, np.int64)
    np.cumsum(counts, out=f.img_offs[1:])
    f.counts = np.asarray(counts).reshape(S, C)
    f.boxes_int = f.boxes.astype(np.int32)
    f.cent = 0.5 * (f.boxes[:, :2].astype(np.float64) + f.boxes[:, 2:].astype(np.float64))
    return f


def sub_captures(f, used, seed):
    """The sub-batch of a pass as captures of their own, built on the host:
    the leftovers of ``f`` under ``used`` in the camera order of ``seed``, as
    detector boxes (the integers as float32: the packing gives them back
    exactly) with the permuted Ks / RTs.  -> (captures, orig, sub_offs)."""
    order = seed_order(seed, f.C)
    cent, boxes_int, orig, sub_offs = leftover_gather(used, f.cent, f.boxes_int, f.img_offs, f.C, order)
    g = Captures()
    g.S, g.C = f.S, f.C
    g.Ks = np.ascontiguousarray(f.Ks[:, list(order)])
    g.RTs = np.ascontiguousarray(f.RTs[:, list(order)])
    g.boxes_int, g.cent = boxes_int, cent
    g.boxes = boxes_int.astype(np.float32)
    g.conf = np.full(len(g.boxes), 0.9, np.float32)
    g.cls = np.zeros(len(g.boxes), np.float32)
    g.img_offs = sub_offs
    g.counts = np.diff(sub_offs).reshape(f.S, f.C)
    return g, orig, sub_offs


def flat_views(comp, C):
    """compose()'s per-capture results as one views array with offs / count."""
    count = np.array([len(c[0]) for c in comp], np.int32)
    offs = np.zeros(len(comp) + 1, np.int64)
    np.cumsum(count, out=offs[1:])
    views = np.concatenate([c[1] for c in comp]).reshape(-1, C).astype(np.int32)
    return views, offs, count


def cpu_passes(f, seeds, thr=30.0):
    """Pass 0 and one pass per triple by the CPU chain the extension's tests
    use (tests/test_extend_gpu.py's ``compose``: the oracle's cube, scipy's
    assignment, the threshold, the extension) -> list of dicts per pass:
    views [n, C] in the pass's slot order, offs, count, order, orig, sub_offs,
    and ``orig_views`` [n, C]: the views in original camera order and
    original detection indices."""
    from bpc_baseline_amd.inference.batch_match import extension_pairs
    from bpc_baseline_amd.inference.utils.camera_utils import fundamental_matrices_batched
    from test_extend_gpu import compose
    C = f.C
    pairs = extension_pairs(C)
    used = np.zeros(len(f.cent), np.int32)
    out = []
    g, order, orig, sub_offs = f, None, None, None
    for p in range(len(seeds) + 1):
        if p:
            order = seed_order(seeds[p - 1], C)
            g, orig, sub_offs = sub_captures(f, used, seeds[p - 1])
        F = fundamental_matrices_batched(g.Ks, g.RTs, pairs).reshape(f.S, len(pairs), 9)
        views, offs, count = flat_views(compose(g, F, thr), C)
        mark_used(used, views, offs, count, f.img_offs, C, order, sub_offs, orig)
        ov = views.copy()
        if p:
            for s in range(f.S):
                for r in range(int(offs[s]), int(offs[s + 1])):
                    for q in range(C):
                        if views[r, q] >= 0:
                            ov[r, q] = orig[sub_offs[s * C + q] + views[r, q]]
            ov = ov[:, np.argsort(order)]
        out.append(dict(views=views, offs=offs, count=count, order=order, orig=orig, sub_offs=sub_offs,
                        orig_views=ov))
    return out
