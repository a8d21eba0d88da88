"""The chordal mean of a row's views under the object's symmetries (DESIGN
§3.21, mvm_fuse_rotations_sym): the normative statement.  A helper, not a test.

``fuse_rotations_sym`` is the definition, in numpy float64 over all slots at
once; every product, sum and comparison below is one rounded operation in the
order it stands, so the kernel, which is built with contraction off, must
return its bits (NaN equal to NaN, ``pose_model.same``).

Slots, decoding, the world product ``W = RTs[s, c, :3, :3]^T M`` and the slot
statuses NO_CAPTURE / NO_VIEW / DEGENERATE are ``pose_model.fuse_rotations``'s,
which is called for them.  A head that sees a symmetric part may answer, per
view, any of the rotations ``R S_k`` that look alike from there; so each usable
slot is first multiplied by the symmetry that takes it nearest a reference
rotation, and the mean is taken of the aligned views:

1. the reference ``R_ref`` of round 1 is the W of the row's first usable slot
   in the order of ``cams``;
2. per usable slot ``B = R_ref^T W`` (``to_world``'s operation order) and, for
   k ascending, ``s_k = sum_ij B_ij S_k,ji`` summed over (i, j) row-major, left
   to right: the trace of ``B S_k = R_ref^T W S_k``, whose largest value is
   the smallest Frobenius distance of ``W S_k`` to ``R_ref`` (note the
   transposed index of S: ``sum_ij B_ij S_k,ij`` would be the trace with
   ``S_k^T`` and pick the inverse element).  ``best`` and ``second`` start at -inf;
   ``s_k > best`` moves best to second and takes k, else ``s_k > second``
   replaces second: the lowest index wins a tie, a NaN is never taken, and
   ``sym_margin = best - second`` is +inf where only one score was taken (and
   +inf or NaN where scores of absurd symmetries overflow).  ``W' = W
   S_k`` is ``(W_i0 S_0j + W_i1 S_1j) + W_i2 S_2j``.  A slot where no k was
   taken, or whose W' has an entry that is not below 2^500 in magnitude, gets
   NO_SYM and is not used again in this round or a later one;
3. ``R_r = pose_model.mean_rotation`` of the W' of the slots still usable, in
   slot order; a row without one has NO_ROTATION and is done;
4. steps 2 and 3 are repeated with ``R_ref = R_(r-1)``, ``rounds`` in all.

Only the top-left 3 x 3 block of a symmetry is read.  With ``syms = [I]`` every
s_0 is finite, k = 0 is taken and ``W' = W`` as numbers (a -0 in W comes back
+0: ``(-0 * 1 + w * 0) + w * 0`` is +0), so R, pose, spread and the statuses
are ``fuse="mean"``'s.
"""
import numpy as np

import pose_model as P
from pose_model import (AMBIGUOUS, DEGENERATE, NO_CAPTURE, NO_ROTATION, NO_VIEW, WORLD_MAX,  # noqa: F401
                        decode, euler_filter, mean_rotation, quat_matrix, same, to_world)

NO_SYM = 8                                                    # slot status: no symmetry left the slot usable
MAX_ROUNDS = 4


def align_scores(R_ref, W, S):
    """R_ref f64 [n, 3, 3], W f64 [n, 3, 3], S f64 [K, 3, 3] -> (index int32
    [n] or -1, best f64 [n], second f64 [n]): step 2's scan."""
    n = len(W)
    with np.errstate(all="ignore"):
        B = [[(R_ref[:, 0, i] * W[:, 0, j] + R_ref[:, 1, i] * W[:, 1, j]) + R_ref[:, 2, i] * W[:, 2, j]
              for j in range(3)] for i in range(3)]
        best, second = np.full(n, -np.inf), np.full(n, -np.inf)
        index = np.full(n, -1, np.int32)
        for k in range(len(S)):
            s = B[0][0] * S[k, 0, 0]                          # B_ij S_ji: the trace of B S
            for i, j in [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]:
                s = s + B[i][j] * S[k, j, i]
            up = s > best
            second = np.where(up, best, np.where(s > second, s, second))
            best = np.where(up, s, best)
            index = np.where(up, np.int32(k), index)
    return index, best, second


def apply_symmetry(W, S, index):
    """W' = W S_index, f64 [n, 3, 3] (the rows with index -1 take S_0: their
    caller drops them)."""
    Sk = S[np.maximum(index, 0)]
    out = np.empty(W.shape)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                out[:, i, j] = (W[:, i, 0] * Sk[:, 0, j] + W[:, i, 1] * Sk[:, 1, j]) + W[:, i, 2] * Sk[:, 2, j]
    return out


def fuse_rotations_sym(raw, scene, views, X, RTs, mode, syms, rows=None, cams=None, rounds=2, scene_base=0):
    """The definition.  The arguments of ``pose_model.fuse_rotations`` and
    ``syms`` f64 [K, 4, 4], ``rounds`` 1..4.
    -> dict of ``pose_model.fuse_rotations``'s outputs (rot_views holds the
    aligned W' of the last round, spread their squared distance to R,
    slot_status may hold NO_SYM) and sym_index int32 [rows, cams] (the k of
    the last round, -1 where the slot is not usable), sym_margin f64
    [rows, cams] (best - second of the last round, NaN where the slot is not
    usable), n_changed int32 [rows] (the slots usable in the end whose k of the
    last round is not the one of the round before; 0 for rounds = 1)."""
    syms = np.asarray(syms, np.float64)
    if syms.ndim != 3 or syms.shape[1:] != (4, 4) or len(syms) < 1:
        raise ValueError(f"syms must be [K, 4, 4] with K >= 1, got {syms.shape}")
    if not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError(f"rounds: expected 1..{MAX_ROUNDS}, got {rounds}")
    S = np.ascontiguousarray(syms[:, :3, :3])
    base = P.fuse_rotations(raw, scene, views, X, RTs, mode, rows=rows, cams=cams, fuse="mean",
                            scene_base=scene_base)
    W, status = base["rot_views"], base["slot_status"].copy()
    m, K = status.shape
    first = np.argmax(status == 0, axis=1)                    # the first usable slot (0 where there is none)
    R_ref = np.where(np.isnan(W[np.arange(m), first]), 0.0, W[np.arange(m), first])
    index = np.full((m, K), -1, np.int32)
    margin = np.full((m, K), np.nan)
    Wp = np.full((m, K, 3, 3), np.nan)
    n_changed = np.zeros(m, np.int32)
    lam = np.full((m, 2), np.nan)
    for rnd in range(rounds):
        before = index.copy()
        for k in range(K):
            used = status[:, k] == 0
            Wk = np.where(used[:, None, None], W[:, k], 0.0)
            idx, best, second = align_scores(R_ref, Wk, S)
            Wa = apply_symmetry(Wk, S, idx)
            with np.errstate(invalid="ignore"):
                sane = (idx >= 0) & (np.abs(Wa) < WORLD_MAX).all(axis=(1, 2))
                diff = best - second
            status[:, k] = np.where(used & ~sane, NO_SYM, status[:, k])
            used = used & sane
            index[:, k] = np.where(used, idx, -1)
            margin[:, k] = np.where(used, diff, np.nan)
            Wp[:, k] = np.where(used[:, None, None], Wa, np.nan)
        used = status == 0
        R, lam_r = mean_rotation(np.where(used[:, :, None, None], Wp, 0.0), used)
        ok = used.any(axis=1)
        R_ref = np.where(ok[:, None, None], R, R_ref)
        lam = np.where(ok[:, None], lam_r, np.nan)
        n_changed = (used & (index != before)).sum(axis=1).astype(np.int32) if rnd else n_changed
    used = status == 0
    n_used = used.sum(axis=1)
    ok = n_used > 0
    row_status = np.where(ok, np.where(lam[:, 0] - lam[:, 1] <= P.AMBIGUOUS_GAP * n_used, AMBIGUOUS, 0),
                          NO_ROTATION).astype(np.int32)
    R = np.where(ok[:, None, None], R_ref, np.nan)
    spread = np.zeros((m, K))
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                dlt = Wp[:, :, i, j] - R[:, None, i, j]
                spread = spread + dlt * dlt
    spread = np.where(used & ok[:, None], spread, np.nan)
    pose = base["pose"].copy()
    pose[:, :3, :3] = R
    return dict(rot_views=Wp, R=R, pose=pose, spread=spread, slot_status=status, row_status=row_status, lam=lam,
                sym_index=index, sym_margin=margin, n_changed=n_changed)


def invariants(out):
    """``pose_model.invariants`` with NO_SYM among the slot statuses, and what
    the new outputs promise: sym_index >= 0 exactly on the usable slots,
    sym_margin NaN off them and never below 0; n_changed within the usable
    slots."""
    masked = dict(out)
    masked["slot_status"] = np.where(np.asarray(out["slot_status"]) == NO_SYM, DEGENERATE, out["slot_status"])
    assert np.isin(out["slot_status"], (0, NO_VIEW, NO_CAPTURE, DEGENERATE, NO_SYM)).all()
    P.invariants(masked)
    usable = np.asarray(out["slot_status"]) == 0
    assert ((np.asarray(out["sym_index"]) >= 0) == usable).all() and (out["sym_index"][~usable] == -1).all()
    if "sym_margin" in out:
        assert np.isnan(out["sym_margin"][~usable]).all() and not (out["sym_margin"][usable] < 0).any()
    if "n_changed" in out:
        assert ((0 <= out["n_changed"]) & (out["n_changed"] <= usable.sum(axis=1))).all()


def rot_z(angle):
    return P.axis_angle((0, 0, 1), angle)


def z_fold(n):
    """The n-fold symmetry about z as f64 [n, 4, 4], exact for n = 1, 2, 4."""
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        out[k, :3, :3] = np.round(rot_z(2 * np.pi * k / n)) if n in (1, 2, 4) else rot_z(2 * np.pi * k / n)
    return out


def with_blocks(G):
    """Rotations f64 [K, 3, 3] -> symmetry transforms f64 [K, 4, 4]."""
    out = np.tile(np.eye(4), (len(G), 1, 1))
    out[:, :3, :3] = G
    return out
