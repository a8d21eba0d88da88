// mvm_poses.hip — from the rotation head's raw outputs to a pose per match
// (DESIGN §3.19): per (table row, selected camera) slot the raw vector is
// decoded in float32 by the reference's rule (Euler, quaternion or 6-D), taken
// to the world by the camera's extrinsic rotation in float64, and the usable
// slots of a row are fused: one camera's rotation, or the chordal mean (the
// largest eigenvector of Horn's 4 x 4 matrix by cyclic Jacobi rotations).
// Every step and its order are stated by tests/pose_model.py, whose bits the
// kernel returns.
// fuse_rotations_sym_kernel takes the same mean under the object's symmetries
// (tests/pose_sym_model.py).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "mvmatch.h"
#include "mvm_device.h"
#include "mvm_internal.h"

#pragma clang fp contract(off)

namespace {

enum : int { kModeEuler = 0, kModeQuat = 1, kMode6d = 2 };
enum : int { kFuseCam = 0, kFuseMean = 1 };
enum : int32_t { kSlotNoView = 1, kSlotNoCapture = 2, kSlotDegenerate = 4, kSlotNoSym = 8 };
constexpr int kMaxRounds = 4;
enum : int32_t { kRowNoRotation = 1, kRowAmbiguous = 2 };

constexpr int kJacobiSweeps = 8;
constexpr double kAmbiguousGap = 1e-9;
// a world rotation with an entry of 2^500 or more in magnitude is degenerate:
// below it the sum of eight, Horn's combinations, the power step's squares and
// the spread's nine stay finite
constexpr int kWorldMaxExp = 500;
constexpr float kEps32 = 1e-8f;
constexpr float kPi32 = (float)3.14159265358979323846;
constexpr float kTwoPi32 = (float)6.28318530717958647692;

constexpr int mode_width(int mode) { return mode == kModeEuler ? 3 : mode == kModeQuat ? 4 : 6; }

// the nine entries of quat_to_rotmat, left to right, in T
template <typename T>
__device__ __forceinline__ void quat_matrix(T x, T y, T z, T w, T m[9]) {
    const T one = 1, two = 2;
    m[0] = one - two * y * y - two * z * z;
    m[1] = two * x * y - two * z * w;
    m[2] = two * x * z + two * y * w;
    m[3] = two * x * y + two * z * w;
    m[4] = one - two * x * x - two * z * z;
    m[5] = two * y * z - two * x * w;
    m[6] = two * x * z - two * y * w;
    m[7] = two * y * z + two * x * w;
    m[8] = one - two * x * x - two * y * y;
}

__device__ __forceinline__ float norm3(float a, float b, float c) { return sqrtf((a * a + b * b) + c * c); }
// max(n, 1e-8) that lets a NaN through
__device__ __forceinline__ float clamp_eps(float n) { return n < kEps32 ? kEps32 : n; }

// ((a + pi) mod 2 pi) - pi, the modulo floored: fmodf, plus the divisor where
// the remainder is non-zero and negative; a zero remainder is +0
__device__ __forceinline__ float wrap_angle(float a) {
    float m = fmodf(a + kPi32, kTwoPi32);
    if (m != 0.0f) {
        if (m < 0.0f) m += kTwoPi32;
    } else {
        m = 0.0f;
    }
    return m - kPi32;
}

template <int MODE>
__device__ __forceinline__ void decode(const float *__restrict__ raw, float m[9]) {
    if constexpr (MODE == kModeQuat) {
        float x = raw[0], y = raw[1], z = raw[2], w = raw[3];
        float n = sqrtf(((x * x + y * y) + z * z) + w * w) + kEps32;
        x = x / n, y = y / n, z = z / n, w = w / n;
        n = sqrtf(((x * x + y * y) + z * z) + w * w);
        x = x / n, y = y / n, z = z / n, w = w / n;
        quat_matrix<float>(x, y, z, w, m);
    } else if constexpr (MODE == kMode6d) {
        const float a10 = raw[0], a11 = raw[1], a12 = raw[2], a20 = raw[3], a21 = raw[4], a22 = raw[5];
        float n = clamp_eps(norm3(a10, a11, a12));
        const float b10 = a10 / n, b11 = a11 / n, b12 = a12 / n;
        const float d = (b10 * a20 + b11 * a21) + b12 * a22;
        const float t0 = a20 - d * b10, t1 = a21 - d * b11, t2 = a22 - d * b12;
        n = clamp_eps(norm3(t0, t1, t2));
        const float b20 = t0 / n, b21 = t1 / n, b22 = t2 / n;
        m[0] = b10, m[3] = b11, m[6] = b12;
        m[1] = b20, m[4] = b21, m[7] = b22;
        m[2] = b11 * b22 - b12 * b21;
        m[5] = b12 * b20 - b10 * b22;
        m[8] = b10 * b21 - b11 * b20;
    } else {
        const double ax = (double)wrap_angle(raw[0]), ay = (double)wrap_angle(raw[1]),
                     az = (double)wrap_angle(raw[2]);
        const float sx = (float)sin(ax), sy = (float)sin(ay), sz = (float)sin(az);
        const float cx = (float)cos(ax), cy = (float)cos(ay), cz = (float)cos(az);
        m[0] = cy * cz;
        m[1] = -cy * sz;
        m[2] = sy;
        m[3] = sx * sy * cz + cx * sz;
        m[4] = -sx * sy * sz + cx * cz;
        m[5] = -sx * cy;
        m[6] = -cx * sy * cz + sx * sz;
        m[7] = cx * sy * sz + sx * cz;
        m[8] = cx * cy;
    }
}

// |x| < 2^kWorldMaxExp, false for a NaN: the biased exponent alone decides
__device__ __forceinline__ bool below_world_max(double x) {
    return (uint32_t)(__double2hiint(x) & 0x7fffffff) < ((uint32_t)(1023 + kWorldMaxExp) << 20);
}

// What one thread knows of its row
struct PoseRow {
    const float *raw;        // the row's first raw vector
    const int32_t *views;    // the row's views
    const double *rts;       // the capture's first extrinsic matrix, or nullptr: no such capture
    uint32_t cams_packed;
};

// Slot k of the row -> its status and, where that is 0, W = R_c^T M in float64;
// degenerate where M has a non-finite entry or W one that is not below_world_max
template <int MODE>
__device__ __forceinline__ int32_t slot_world(const PoseRow &row, int k, double W[9]) {
    if (!row.rts) return kSlotNoCapture;
    const int cam = (int)((row.cams_packed >> (4 * k)) & 15u);
    if (row.views[cam] < 0) return kSlotNoView;
    float m[9];
    decode<MODE>(row.raw + k * mode_width(MODE), m);
    bool finite = true;
#pragma unroll
    for (int e = 0; e < 9; ++e) finite = finite && __builtin_isfinite(m[e]);
    if (!finite) return kSlotDegenerate;
    const double *R = row.rts + cam * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            W[3 * i + j] = (R[i] * (double)m[j] + R[4 + i] * (double)m[3 + j]) + R[8 + i] * (double)m[6 + j];
    // a NaN, an infinity or an absurd magnitude from the extrinsic rotation: no
    // rotation either
    bool sane = true;
#pragma unroll
    for (int e = 0; e < 9; ++e) sane = sane && below_world_max(W[e]);
    if (!sane) return kSlotDegenerate;
    return 0;
}

// One Jacobi rotation of the pair (P, Q) on the upper triangle of a, gathered
// into v; skipped where the off-diagonal entry is exactly 0.  Every index is a
// compile-time constant once the k loops are unrolled: a and v stay in registers.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = theta < 0.0 ? -t : t;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    a[P][P] = a[P][P] - h;
    a[Q][Q] = a[Q][Q] + h;
    a[P][Q] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == P || k == Q) continue;
        double &kp = k < P ? a[k][P] : a[P][k];
        double &kq = k < Q ? a[k][Q] : a[Q][k];
        const double akp = kp, akq = kq;
        kp = c * akp - s * akq;
        kq = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
}

// The rotation nearest the sum A of rotations -> Rm, and the two largest
// eigenvalues of Horn's matrix
__device__ __forceinline__ void mean_rotation(const double A[9], double Rm[9], double &lam1, double &lam2) {
    double N[4][4] = {};
    N[0][0] = (A[0] - A[4]) - A[8];
    N[1][1] = (A[4] - A[0]) - A[8];
    N[2][2] = (A[8] - A[0]) - A[4];
    N[3][3] = (A[0] + A[4]) + A[8];
    N[0][1] = A[1] + A[3];
    N[0][2] = A[2] + A[6];
    N[0][3] = A[7] - A[5];
    N[1][2] = A[5] + A[7];
    N[1][3] = A[2] - A[6];
    N[2][3] = A[3] - A[1];
    double a[4][4], v[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[p][q] = N[p][q];
            v[p][q] = p == q ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<0, 3>(a, v);
        jacobi_rotate<1, 2>(a, v);
        jacobi_rotate<1, 3>(a, v);
        jacobi_rotate<2, 3>(a, v);
    }
    int best = 0;
    lam1 = a[0][0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (a[j][j] > lam1) best = j, lam1 = a[j][j];          // the lowest index wins a tie
    lam2 = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (best != j && a[j][j] > lam2) lam2 = a[j][j];
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = best == 0 ? v[k][0] : best == 1 ? v[k][1] : best == 2 ? v[k][2] : v[k][3];
    // one shifted power step polishes the vector (tr N = 0: -lam1 / 3 is the
    // mean of the other eigenvalues); kept only where it has a length
    const double third = lam1 / 3.0;
    double p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double ni0 = i <= 0 ? N[i][0] : N[0][i], ni1 = i <= 1 ? N[i][1] : N[1][i];
        const double ni2 = i <= 2 ? N[i][2] : N[2][i], ni3 = N[i][3];
        p[i] = (((ni0 * q[0] + ni1 * q[1]) + ni2 * q[2]) + ni3 * q[3]) + third * q[i];
    }
    const double np = sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3]);
    if (np > 0.0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = p[i];
    }
    const double nq = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = q[i] / nq;
    double big = fabs(q[0]);
    bool neg = q[0] < 0.0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (fabs(q[k]) > big) big = fabs(q[k]), neg = q[k] < 0.0;
    if (neg) {
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = -q[i];
    }
    quat_matrix<double>(q[0], q[1], q[2], q[3], Rm);
}

// One thread per row of the range.  A slot's world rotation is computed where
// it is needed and never kept: once for the sum (mean) or the chosen camera,
// once more for its own outputs, so no per-slot array exists to be indexed.
template <int MODE, int FUSE>
__global__ __launch_bounds__(kThreads) void fuse_rotations_kernel(
    const float *__restrict__ raw, const int32_t *__restrict__ scene, int32_t scene_base,
    const int32_t *__restrict__ views, const double *__restrict__ X, const double *__restrict__ RTs,
    int32_t n_scenes, int32_t n_cams, int64_t row0, int64_t n_rows, uint32_t cams_packed, int32_t n_sel,
    int32_t fuse_k, double *__restrict__ rot_views, double *__restrict__ R_out, double *__restrict__ pose,
    double *__restrict__ spread, int32_t *__restrict__ slot_status, int32_t *__restrict__ row_status) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t t = row0 + r;
    const int64_t sc = (int64_t)scene[t] - scene_base;
    PoseRow row;
    row.raw = raw + r * n_sel * mode_width(MODE);
    row.views = views + t * n_cams;
    row.rts = (sc >= 0 && sc < n_scenes) ? RTs + sc * n_cams * 16 : nullptr;
    row.cams_packed = cams_packed;

    const double nan = __builtin_nan("");
    double Rr[9] = {}, W[9] = {};
    bool ok;
    int32_t rstat = 0;
    if constexpr (FUSE == kFuseCam) {
        ok = slot_world<MODE>(row, fuse_k, Rr) == 0;
    } else {
        double A[9] = {};
        int n_used = 0;
#pragma unroll 1
        for (int k = 0; k < n_sel; ++k) {
            if (slot_world<MODE>(row, k, W) != 0) continue;
            ++n_used;
#pragma unroll
            for (int e = 0; e < 9; ++e) A[e] = A[e] + W[e];
        }
        ok = n_used > 0;
        if (ok) {
            double lam1, lam2;
            mean_rotation(A, Rr, lam1, lam2);
            if (lam1 - lam2 <= kAmbiguousGap * (double)n_used) rstat = kRowAmbiguous;
        }
    }
    if (!ok) {
        rstat = kRowNoRotation;
#pragma unroll
        for (int e = 0; e < 9; ++e) Rr[e] = nan;
    }

#pragma unroll 1
    for (int k = 0; k < n_sel; ++k) {
        const int32_t st = slot_world<MODE>(row, k, W);
        const int64_t slot = r * n_sel + k;
        slot_status[slot] = st;
        if (rot_views) {
#pragma unroll
            for (int e = 0; e < 9; ++e) rot_views[slot * 9 + e] = st == 0 ? W[e] : nan;
        }
        if (spread) {
            double s = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                const double d = W[e] - Rr[e];
                s = s + d * d;
            }
            spread[slot] = (st == 0 && ok) ? s : nan;
        }
    }

    row_status[r] = rstat;
    double *Ro = R_out + r * 9, *P = pose + r * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Ro[3 * i + j] = Rr[3 * i + j];
            P[4 * i + j] = Rr[3 * i + j];
        }
        P[4 * i + 3] = X[t * 3 + i];
    }
    P[12] = 0.0, P[13] = 0.0, P[14] = 0.0, P[15] = 1.0;
}

// ---- the mean under the object's symmetries (tests/pose_sym_model.py) ----

// W S for the top-left 3 x 3 block of the row-major 4 x 4 symmetry S
__device__ __forceinline__ void apply_symmetry(const double W[9], const double *__restrict__ S, double Wp[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Wp[3 * i + j] = (W[3 * i] * S[j] + W[3 * i + 1] * S[4 + j]) + W[3 * i + 2] * S[8 + j];
}

// The symmetry that takes W nearest Rref: B = Rref^T W, s_k = sum_ij B_ij S_k,ji
// (the trace of B S_k) over ascending k; strict '>' from -inf keeps the lowest index of a tie and
// never takes a NaN.  Every lane walks the same k, so a symmetry is read at a
// wave-uniform address (scalar loads).  -> the index or -1, and best - second.
__device__ __forceinline__ int32_t nearest_symmetry(const double Rref[9], const double W[9],
                                                    const double *__restrict__ syms, int32_t n_syms,
                                                    double &margin) {
    double B[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            B[3 * i + j] = (Rref[i] * W[j] + Rref[3 + i] * W[3 + j]) + Rref[6 + i] * W[6 + j];
    double best = -INFINITY, second = -INFINITY;
    int32_t kb = -1;
#pragma unroll 1
    for (int32_t k = 0; k < n_syms; ++k) {
        const double *__restrict__ S = syms + (int64_t)k * 16;
        double s = B[0] * S[0];
        s = s + B[1] * S[4];
        s = s + B[2] * S[8];
#pragma unroll
        for (int i = 1; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) s = s + B[3 * i + j] * S[4 * j + i];
        if (s > best) {
            second = best, best = s, kb = k;
        } else if (s > second) {
            second = s;
        }
    }
    margin = best - second;
    return kb;
}

// The row's fused rotation, into R_out and the pose's block, and its two
// counts; n_changed first: where it is not wanted it lies on row_status
__device__ __forceinline__ void store_row(const double Rr[9], int32_t rstat, int32_t changed, double *Ro,
                                          double *P, int32_t *row_status, int32_t *n_changed) {
    *n_changed = changed;
    *row_status = rstat;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Ro[3 * i + j] = Rr[3 * i + j];
            P[4 * i + j] = Rr[3 * i + j];
        }
}

// One thread per row of the range.  Each round walks the row's slots: a usable
// slot's world rotation is computed anew, aligned to the reference by its
// nearest symmetry and added to the sum; the mean of the round is the next
// round's reference.  What a slot took and whether it is still usable live in
// the thread's own sym_index / slot_status outputs between the rounds, so no
// per-slot array exists to be indexed.
template <int MODE>
__global__ __launch_bounds__(kThreads) void fuse_rotations_sym_kernel(
    const float *__restrict__ raw, const int32_t *__restrict__ scene, int32_t scene_base,
    const int32_t *__restrict__ views, const double *__restrict__ X, const double *__restrict__ RTs,
    int32_t n_scenes, int32_t n_cams, int64_t row0, int64_t n_rows, uint32_t cams_packed, int32_t n_sel,
    const double *__restrict__ syms, int32_t n_syms, int32_t rounds, double *__restrict__ rot_views,
    double *__restrict__ R_out, double *__restrict__ pose, double *__restrict__ spread,
    int32_t *slot_status, int32_t *__restrict__ row_status, int32_t *sym_index,
    double *__restrict__ sym_margin, int32_t *__restrict__ n_changed) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t t = row0 + r;
    const int64_t sc = (int64_t)scene[t] - scene_base;
    PoseRow row;
    row.raw = raw + r * n_sel * mode_width(MODE);
    row.views = views + t * n_cams;
    row.rts = (sc >= 0 && sc < n_scenes) ? RTs + sc * n_cams * 16 : nullptr;
    row.cams_packed = cams_packed;

    // The row's own places in the outputs, taken once.  An optional output that
    // is not wanted is written all the same, into the row's own R_out (whose
    // nine entries hold a value per slot; the views go there with a slot stride
    // of 0) or row_status, which the end of every walk writes after it:
    // so the walks hold no test for the four, whose lane masks would otherwise
    // stay in scalar registers that the Euler decoder needs for itself.
    int32_t *const my_status = slot_status + r * n_sel, *const my_index = sym_index + r * n_sel;
    int32_t *const my_row_status = row_status + r, *const my_changed = n_changed ? n_changed + r : my_row_status;
    double *const Ro = R_out + r * 9, *const P = pose + r * 16;
    double *const my_margin = sym_margin ? sym_margin + r * n_sel : Ro;
    double *const my_views = rot_views ? rot_views + r * n_sel * 9 : Ro;
    double *const my_spread = spread ? spread + r * n_sel : Ro;
    const int views_step = rot_views ? 9 : 0;
    // the pose's translation and last row wait for no rotation
#pragma unroll
    for (int i = 0; i < 3; ++i) P[4 * i + 3] = X[t * 3 + i];
    P[12] = 0.0, P[13] = 0.0, P[14] = 0.0, P[15] = 1.0;

    // the entry point has checked these: no loop below needs a guard for zero trips
    __builtin_assume(n_sel >= 1 && n_sel <= MVM_MAX_CAMS);
    __builtin_assume(n_syms >= 1);
    __builtin_assume(rounds >= 1 && rounds <= kMaxRounds);
    // what round 1 reads back as every later round does: every slot still in,
    // no symmetry taken; and what a slot that ends unusable keeps: NaN
    const double nan = __builtin_nan("");
#pragma unroll 1
    for (int k = 0; k < n_sel; ++k) {
        my_status[k] = 0, my_index[k] = -1;
        my_spread[k] = nan;
#pragma unroll
        for (int e = 0; e < 9; ++e) my_views[k * views_step + e] = nan;
    }

    double Rr[9] = {}, W[9] = {}, Wp[9] = {};
    bool have_ref = false;
    int32_t rstat = 0, changed = 0;
    // the rounds: align every usable slot to the reference, average, and leave
    // the row as the round has it; the last round's is what stays
#pragma unroll 1
    for (int round = 0; round < rounds; ++round) {
        double A[9] = {};
        int n_here = 0;
        int32_t changed_here = 0;
#pragma unroll 1
        for (int k = 0; k < n_sel; ++k) {
            int32_t st = slot_world<MODE>(row, k, W);
            if (st == 0) st = my_status[k];                            // lost to an earlier round
            int32_t kb = -1;
            double margin = nan;
            if (st == 0) {
                if (!have_ref) {                                       // round 1's reference: the first usable slot
                    have_ref = true;
#pragma unroll
                    for (int e = 0; e < 9; ++e) Rr[e] = W[e];
                }
                kb = nearest_symmetry(Rr, W, syms, n_syms, margin);
                bool sane = kb >= 0;
                if (sane) {
                    apply_symmetry(W, syms + (int64_t)kb * 16, Wp);
#pragma unroll
                    for (int e = 0; e < 9; ++e) sane = sane && below_world_max(Wp[e]);
                }
                if (sane) {
                    ++n_here;
#pragma unroll
                    for (int e = 0; e < 9; ++e) A[e] = A[e] + Wp[e];
                    if (my_index[k] != kb) ++changed_here;
                } else {
                    st = kSlotNoSym, kb = -1, margin = nan;
                }
            }
            my_status[k] = st;
            my_index[k] = kb;
            my_margin[k] = margin;
        }
        rstat = 0, changed = round > 0 ? changed_here : 0;
        if (n_here == 0) {
            rstat = kRowNoRotation;
            round = rounds;                                            // every slot is lost: nothing left to align
#pragma unroll
            for (int e = 0; e < 9; ++e) Rr[e] = nan;
        } else {
            double lam1, lam2;
            mean_rotation(A, Rr, lam1, lam2);
            if (lam1 - lam2 <= kAmbiguousGap * (double)n_here) rstat = kRowAmbiguous;
        }
        store_row(Rr, rstat, changed, Ro, P, my_row_status, my_changed);
    }
    // what needs the last mean: the aligned views and their distance to it
#pragma unroll 1
    for (int k = 0; k < n_sel; ++k) {
        if (my_status[k] != 0) continue;
        slot_world<MODE>(row, k, W);
        apply_symmetry(W, syms + (int64_t)my_index[k] * 16, Wp);
#pragma unroll
        for (int e = 0; e < 9; ++e) my_views[k * views_step + e] = Wp[e];
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const double d = Wp[e] - Rr[e];
            s = s + d * d;
        }
        my_spread[k] = s;
    }
    // once more, behind whatever that walk wrote in the row's place
    store_row(Rr, rstat, changed, Ro, P, my_row_status, my_changed);
}

// What both entry points refuse before their pointers
int check_rotation_sizes(int32_t D, int32_t n_scenes, int32_t n_cams, int64_t row0, int64_t n_rows,
                         int32_t n_sel, int32_t mode) {
    if (n_rows < 0 || row0 < 0)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative row0=%lld or n_rows=%lld", (long long)row0,
                        (long long)n_rows);
    if (n_scenes < 0 || n_scenes > 0x7FFFFFFF / MVM_MAX_CAMS)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_scenes=%d outside [0, %d]", n_scenes,
                        0x7FFFFFFF / MVM_MAX_CAMS);
    if (n_cams < 3 || n_cams > MVM_MAX_CAMS)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_cams=%d outside [3, %d]", n_cams, MVM_MAX_CAMS);
    if (n_sel < 1 || n_sel > n_cams)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_sel=%d outside [1, %d]", n_sel, n_cams);
    if (mode < kModeEuler || mode > kMode6d)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "mode=%d: 0 (euler), 1 (quat) or 2 (6d)", mode);
    if (D != mode_width(mode))
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "D=%d: mode=%d takes %d values per slot", D, mode,
                        mode_width(mode));
    return MVM_OK;
}

// The selected cameras, four bits each
int pack_cams(const int32_t *cams_host, int32_t n_sel, int32_t n_cams, uint32_t &cams_packed) {
    cams_packed = 0;
    for (int k = 0; k < n_sel; ++k) {
        if (cams_host[k] < 0 || cams_host[k] >= n_cams)
            return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "cams_host[%d]=%d is no camera < %d", k, cams_host[k],
                            n_cams);
        cams_packed |= (uint32_t)cams_host[k] << (4 * k);
    }
    return MVM_OK;
}

int row_grid(int64_t n_rows, int64_t &grid) {
    grid = (n_rows + kThreads - 1) / kThreads;
    if (grid > kMaxGridBlocks)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_rows=%lld: more rows than one launch holds; split the rows",
                        (long long)n_rows);
    return MVM_OK;
}

}  // namespace

extern "C" {

int mvm_fuse_rotations(const float *raw_dev, int32_t D, const int32_t *scene_dev, int32_t scene_base,
                       const int32_t *views_dev, const double *X_dev, const double *RTs_dev, int32_t n_scenes,
                       int32_t n_cams, int64_t row0, int64_t n_rows, const int32_t *cams_host, int32_t n_sel,
                       int32_t mode, int32_t fuse, int32_t fuse_cam, double *rot_views_dev, double *R_dev,
                       double *pose_dev, double *spread_dev, int32_t *slot_status_dev, int32_t *row_status_dev,
                       mvm_stream_t stream) {
    mvm_clear_error();
    if (n_rows == 0) return MVM_OK;
    if (const int st = check_rotation_sizes(D, n_scenes, n_cams, row0, n_rows, n_sel, mode)) return st;
    if (fuse != kFuseCam && fuse != kFuseMean)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "fuse=%d: 0 (cam) or 1 (mean)", fuse);
    if (const int st = mvm_require_ptrs({{raw_dev, "raw_dev"},
                                         {scene_dev, "scene_dev"},
                                         {views_dev, "views_dev"},
                                         {X_dev, "X_dev"},
                                         {RTs_dev, "RTs_dev"},
                                         {cams_host, "cams_host"},
                                         {R_dev, "R_dev"},
                                         {pose_dev, "pose_dev"},
                                         {slot_status_dev, "slot_status_dev"},
                                         {row_status_dev, "row_status_dev"}}))
        return st;                       // rot_views_dev and spread_dev may be NULL: not written
    uint32_t cams_packed;
    if (const int st = pack_cams(cams_host, n_sel, n_cams, cams_packed)) return st;
    int fuse_k = -1;
    for (int k = n_sel - 1; k >= 0; --k)
        if (cams_host[k] == fuse_cam) fuse_k = k;                 // the first of equal ones
    if (fuse == kFuseCam && fuse_k < 0)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "fuse_cam=%d is not among the selected cameras", fuse_cam);
    int64_t grid;
    if (const int st = row_grid(n_rows, grid)) return st;
    dispatch_int<kModeEuler, kModeQuat, kMode6d>(mode, [&](auto m) {
        dispatch_bool(fuse == kFuseMean, [&](auto mean) {
            fuse_rotations_kernel<decltype(m)::value, decltype(mean)::value ? kFuseMean : kFuseCam>
                <<<(unsigned)grid, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
                    raw_dev, scene_dev, scene_base, views_dev, X_dev, RTs_dev, n_scenes, n_cams, row0, n_rows,
                    cams_packed, n_sel, fuse_k < 0 ? 0 : fuse_k, rot_views_dev, R_dev, pose_dev, spread_dev,
                    slot_status_dev, row_status_dev);
        });
    });
    return mvm_check_launch("fuse_rotations_kernel");
}

int mvm_fuse_rotations_sym(const float *raw_dev, int32_t D, const int32_t *scene_dev, int32_t scene_base,
                           const int32_t *views_dev, const double *X_dev, const double *RTs_dev,
                           int32_t n_scenes, int32_t n_cams, int64_t row0, int64_t n_rows,
                           const int32_t *cams_host, int32_t n_sel, int32_t mode, const double *syms_dev,
                           int32_t n_syms, int32_t rounds, double *rot_views_dev, double *R_dev,
                           double *pose_dev, double *spread_dev, int32_t *slot_status_dev,
                           int32_t *row_status_dev, int32_t *sym_index_dev, double *sym_margin_dev,
                           int32_t *n_changed_dev, mvm_stream_t stream) {
    mvm_clear_error();
    if (n_rows == 0) return MVM_OK;
    if (const int st = check_rotation_sizes(D, n_scenes, n_cams, row0, n_rows, n_sel, mode)) return st;
    if (n_syms < 1) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_syms=%d: at least 1", n_syms);
    if (rounds < 1 || rounds > kMaxRounds)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "rounds=%d outside [1, %d]", rounds, kMaxRounds);
    if (const int st = mvm_require_ptrs({{raw_dev, "raw_dev"},
                                         {scene_dev, "scene_dev"},
                                         {views_dev, "views_dev"},
                                         {X_dev, "X_dev"},
                                         {RTs_dev, "RTs_dev"},
                                         {cams_host, "cams_host"},
                                         {syms_dev, "syms_dev"},
                                         {R_dev, "R_dev"},
                                         {pose_dev, "pose_dev"},
                                         {slot_status_dev, "slot_status_dev"},
                                         {row_status_dev, "row_status_dev"},
                                         {sym_index_dev, "sym_index_dev"}}))
        return st;       // rot_views_dev, spread_dev, sym_margin_dev and n_changed_dev may be NULL: not written
    uint32_t cams_packed;
    if (const int st = pack_cams(cams_host, n_sel, n_cams, cams_packed)) return st;
    int64_t grid;
    if (const int st = row_grid(n_rows, grid)) return st;
    dispatch_int<kModeEuler, kModeQuat, kMode6d>(mode, [&](auto m) {
        fuse_rotations_sym_kernel<decltype(m)::value>
            <<<(unsigned)grid, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
                raw_dev, scene_dev, scene_base, views_dev, X_dev, RTs_dev, n_scenes, n_cams, row0, n_rows,
                cams_packed, n_sel, syms_dev, n_syms, rounds, rot_views_dev, R_dev, pose_dev, spread_dev,
                slot_status_dev, row_status_dev, sym_index_dev, sym_margin_dev, n_changed_dev);
    });
    return mvm_check_launch("fuse_rotations_sym_kernel");
}

}  // extern "C"
