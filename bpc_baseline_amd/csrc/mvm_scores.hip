// mvm_scores.hip — poses against ground truth: the BOP pose
// error MSSD (maximum symmetry-aware surface distance) of every (estimate,
// ground-truth object) pair of a capture, and the greedy matching of a
// capture's rows to its ground truth under a list of thresholds.  Every step
// and its order are stated by tests/score_model.py, whose bits the kernels
// return.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "mvmatch.h"
#include "mvm_device.h"
#include "mvm_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxSyms = 64;
constexpr int kMaxThresholds = 16;
constexpr int kMaxMatchGt = 1024;        // one taken bit per lane and 64-column chunk: 16 chunks
// a pose with a read entry of 2^200 or more in magnitude is not scored: below
// it, with vertices and symmetries below it too, no term of the error is a NaN
constexpr int kPoseMaxExp = 200;
enum : int32_t { kSymPadding = -1, kSymNoCapture = -2, kSymNotFinite = -3 };
constexpr int32_t kNoColumn = 0x7FFFFFFF;

// |x| < 2^kPoseMaxExp, false for a NaN: the biased exponent alone decides
__device__ __forceinline__ bool below_pose_max(double x) {
    return (uint32_t)(__double2hiint(x) & 0x7fffffff) < ((uint32_t)(1023 + kPoseMaxExp) << 20);
}

// the top three rows of a row-major 4 x 4 -> R (row-major 3 x 3), t; false
// where one of the twelve is not below_pose_max
__device__ __forceinline__ bool load_pose(const double *__restrict__ p, double R[9], double t[3]) {
    bool sane = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R[3 * i + j] = p[4 * i + j];
            sane = sane && below_pose_max(R[3 * i + j]);
        }
        t[i] = p[4 * i + 3];
        sane = sane && below_pose_max(t[i]);
    }
    return sane;
}

// One thread per (row of the range, ground-truth column).  The symmetries and
// the vertices are walked by loops every lane runs alike, so what they index
// is read at wave-uniform addresses (scalar loads: no LDS, no vector register);
// a thread holds the two poses, and per symmetry the affine map (A, b) of
// estimate minus ground truth.  The minimum over the symmetries is the
// thread's own running one: strict '<' keeps the lowest index.
__global__ __launch_bounds__(kThreads) void score_poses_kernel(
    const double *__restrict__ pose, const int32_t *__restrict__ scene, int32_t scene_base,
    const double *__restrict__ gt_pose, const int64_t *__restrict__ gt_offs, int32_t n_scenes, int32_t g_max,
    const double *__restrict__ verts, int32_t n_verts, const double *__restrict__ syms, int32_t n_syms,
    int64_t row0, int64_t n_pairs, double *__restrict__ err, int32_t *__restrict__ sym,
    double *__restrict__ t_err, double *__restrict__ rot_cos) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_pairs) return;
    const int64_t r = idx / g_max;
    const int64_t g = idx - r * g_max;
    const int64_t t = row0 + r;
    const int64_t sc = (int64_t)scene[t] - scene_base;

    double Rp[9] = {}, tp[3] = {}, Rg[9] = {}, tg[3] = {};
    int32_t code = 0;
    if (sc < 0 || sc >= n_scenes) {
        code = kSymNoCapture;
    } else {
        const int64_t g0 = gt_offs[sc];
        if (g >= gt_offs[sc + 1] - g0) {
            code = kSymPadding;
        } else {
            const bool sane_p = load_pose(pose + t * 16, Rp, tp);
            const bool sane_g = load_pose(gt_pose + (g0 + g) * 16, Rg, tg);
            if (!(sane_p && sane_g)) code = kSymNotFinite;
        }
    }

    double o_err = INFINITY, o_terr = INFINITY, o_cos = __builtin_nan("");
    int32_t o_sym = code;
    if (code == 0) {
        double best = 0.0, best_dot = 0.0;
#pragma unroll 1
        for (int k = 0; k < n_syms; ++k) {
            const double *__restrict__ S = syms + (int64_t)k * 16;
            double A[9], b[3], dot = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double m = (Rg[3 * i] * S[j] + Rg[3 * i + 1] * S[4 + j]) + Rg[3 * i + 2] * S[8 + j];
                    A[3 * i + j] = Rp[3 * i + j] - m;
                    const double pm = Rp[3 * i + j] * m;
                    dot = (i == 0 && j == 0) ? pm : dot + pm;
                }
                const double u = ((Rg[3 * i] * S[3] + Rg[3 * i + 1] * S[7]) + Rg[3 * i + 2] * S[11]) + tg[i];
                b[i] = tp[i] - u;
            }
            double mk = 0.0;               // every q is >= +0
#pragma unroll 4
            for (int v = 0; v < n_verts; ++v) {
                const double x = verts[3 * (int64_t)v], y = verts[3 * (int64_t)v + 1], z = verts[3 * (int64_t)v + 2];
                const double d0 = ((A[0] * x + A[1] * y) + A[2] * z) + b[0];
                const double d1 = ((A[3] * x + A[4] * y) + A[5] * z) + b[1];
                const double d2 = ((A[6] * x + A[7] * y) + A[8] * z) + b[2];
                const double q = (d0 * d0 + d1 * d1) + d2 * d2;
                mk = q > mk ? q : mk;
            }
            if (k == 0 || mk < best) best = mk, best_dot = dot, o_sym = k;
        }
        o_err = sqrt(best);
        const double e0 = tp[0] - tg[0], e1 = tp[1] - tg[1], e2 = tp[2] - tg[2];
        o_terr = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        o_cos = (best_dot - 1.0) * 0.5;
    }
    err[idx] = o_err;
    sym[idx] = o_sym;
    if (t_err) t_err[idx] = o_terr;
    if (rot_cos) rot_cos[idx] = o_cos;
}

struct Thresholds {
    double v[kMaxThresholds];
};

__device__ __forceinline__ int64_t clamp_i64(int64_t x, int64_t lo, int64_t hi) {
    return x < lo ? lo : x > hi ? hi : x;
}

// One wave per (capture, threshold).  The capture's rows are walked in table
// order; per row the lanes run over the ground-truth columns in chunks of 64,
// each keeping its own best free column below the threshold (strict '<' over
// ascending chunks: its lowest), then the wave takes the smallest error and,
// among the lanes holding it, the lowest column.  Bit c of a lane's `taken`
// says that column 64 c + lane is taken.  The row range is clamped into
// 0 .. n_rows before any row is touched; the waves of the first and the last
// capture write -1 to the rows before and behind every capture's.
__global__ __launch_bounds__(kThreads) void match_scores_kernel(
    const double *__restrict__ err, int32_t g_max, const int64_t *__restrict__ row_offs,
    const int64_t *__restrict__ gt_offs, int32_t n_scenes, Thresholds th, int32_t n_thresholds,
    int32_t *__restrict__ gt_index, int32_t *__restrict__ tp, int64_t n_rows) {
    const int lane = threadIdx.x % kWave;
    const int64_t n_items = (int64_t)(n_scenes > 0 ? n_scenes : 1) * n_thresholds;
    const int64_t item = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (item >= n_items) return;
    const int64_t s = item / n_thresholds;
    const int t = (int)(item - s * n_thresholds);
    double tau = th.v[0];
#pragma unroll
    for (int i = 1; i < kMaxThresholds; ++i) tau = t == i ? th.v[i] : tau;   // no indexed read of the arguments

    int64_t b = 0, e = 0;
    int32_t gs = 0;
    if (n_scenes > 0) {
        b = clamp_i64(row_offs[s], 0, n_rows);
        e = clamp_i64(row_offs[s + 1], b, n_rows);
        gs = (int32_t)clamp_i64(gt_offs[s + 1] - gt_offs[s], 0, g_max);
    }
    int32_t *__restrict__ out = gt_index + (int64_t)t * n_rows;
    if (s == 0)
        for (int64_t r = lane; r < b; r += kWave) out[r] = -1;
    if (s + 1 >= n_scenes)
        for (int64_t r = e + lane; r < n_rows; r += kWave) out[r] = -1;

    uint32_t taken = 0;
    int32_t count = 0;
    for (int64_t r = b; r < e; ++r) {
        const double *__restrict__ row = err + r * g_max;
        double bv = INFINITY;
        int32_t bg = kNoColumn;
        for (int c = 0; c * kWave < gs; ++c) {
            const int32_t g = c * kWave + lane;
            if (g < gs && !((taken >> c) & 1u)) {
                const double v = row[g];
                if (v < tau && v < bv) bv = v, bg = g;
            }
        }
        // a lane without a candidate holds (+inf, no column); a candidate is
        // below tau, so never a NaN and never +inf
        const double vmin = wave_min_f64(bv);
        const int32_t gmin = wave_min_i32(bv == vmin ? bg : kNoColumn);
        const bool hit = gmin != kNoColumn;
        if (hit && lane == (gmin & (kWave - 1))) taken |= 1u << (gmin / kWave);
        if (lane == 0) out[r] = hit ? gmin : -1;
        count += hit ? 1 : 0;
    }
    if (lane == 0 && n_scenes > 0) tp[(int64_t)t * n_scenes + s] = count;
}

}  // namespace

extern "C" {

int mvm_score_poses(const double *pose_dev, const int32_t *scene_dev, int32_t scene_base,
                    const double *gt_pose_dev, const int64_t *gt_offs_dev, int32_t n_scenes, int32_t g_max,
                    const double *verts_dev, int32_t n_verts, const double *syms_dev, int32_t n_syms,
                    int64_t row0, int64_t n_rows, double *err_dev, int32_t *sym_dev, double *t_err_dev,
                    double *rot_cos_dev, mvm_stream_t stream) {
    mvm_clear_error();
    if (n_rows == 0) return MVM_OK;
    if (n_rows < 0 || row0 < 0)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative row0=%lld or n_rows=%lld", (long long)row0,
                        (long long)n_rows);
    if (n_scenes < 0) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_scenes=%d is negative", n_scenes);
    if (g_max < 1) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "g_max=%d: at least 1", g_max);
    if (n_verts < 1) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_verts=%d: at least 1", n_verts);
    if (n_syms < 1 || n_syms > kMaxSyms)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_syms=%d outside [1, %d]", n_syms, kMaxSyms);
    if (const int st = mvm_require_ptrs({{pose_dev, "pose_dev"},
                                         {scene_dev, "scene_dev"},
                                         {gt_pose_dev, "gt_pose_dev"},
                                         {gt_offs_dev, "gt_offs_dev"},
                                         {verts_dev, "verts_dev"},
                                         {syms_dev, "syms_dev"},
                                         {err_dev, "err_dev"},
                                         {sym_dev, "sym_dev"}}))
        return st;                       // t_err_dev and rot_cos_dev may be NULL: not written
    if (n_rows > kMaxGridBlocks * kThreads / g_max)
        return mvm_fail(MVM_ERR_UNSUPPORTED,
                        "n_rows=%lld x g_max=%d: more pairs than one launch holds; split the rows",
                        (long long)n_rows, g_max);
    const int64_t n_pairs = n_rows * g_max;
    const int64_t grid = (n_pairs + kThreads - 1) / kThreads;
    score_poses_kernel<<<(unsigned)grid, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        pose_dev, scene_dev, scene_base, gt_pose_dev, gt_offs_dev, n_scenes, g_max, verts_dev, n_verts, syms_dev,
        n_syms, row0, n_pairs, err_dev, sym_dev, t_err_dev, rot_cos_dev);
    return mvm_check_launch("score_poses_kernel");
}

int mvm_match_scores(const double *err_dev, int32_t g_max, const int64_t *row_offs_dev,
                     const int64_t *gt_offs_dev, int32_t n_scenes, const double *thresholds_host,
                     int32_t n_thresholds, int32_t *gt_index_dev, int32_t *tp_dev, int64_t n_rows_total,
                     mvm_stream_t stream) {
    mvm_clear_error();
    if (n_scenes < 0 || n_rows_total < 0)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative n_scenes=%d or n_rows_total=%lld", n_scenes,
                        (long long)n_rows_total);
    if (n_scenes == 0 && n_rows_total == 0) return MVM_OK;      // nothing to write
    if (n_thresholds < 1 || n_thresholds > kMaxThresholds)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_thresholds=%d outside [1, %d]", n_thresholds,
                        kMaxThresholds);
    if (g_max < 1 || g_max > kMaxMatchGt)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "g_max=%d outside [1, %d]", g_max, kMaxMatchGt);
    if (const int st = mvm_require_ptrs({{thresholds_host, "thresholds_host"}})) return st;
    if (n_scenes > 0)
        if (const int st = mvm_require_ptrs(
                {{row_offs_dev, "row_offs_dev"}, {gt_offs_dev, "gt_offs_dev"}, {tp_dev, "tp_dev"}}))
            return st;
    if (n_rows_total > 0)
        if (const int st = mvm_require_ptrs({{err_dev, "err_dev"}, {gt_index_dev, "gt_index_dev"}})) return st;
    Thresholds th = {};
    for (int i = 0; i < n_thresholds; ++i) th.v[i] = thresholds_host[i];
    const int64_t n_items = (int64_t)(n_scenes > 0 ? n_scenes : 1) * n_thresholds;
    const int64_t grid = (n_items + kWaves - 1) / kWaves;
    if (grid > kMaxGridBlocks)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_scenes=%d: more captures than one launch holds", n_scenes);
    match_scores_kernel<<<(unsigned)grid, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        err_dev, g_max, row_offs_dev, gt_offs_dev, n_scenes, th, n_thresholds, gt_index_dev, tp_dev,
        n_rows_total);
    return mvm_check_launch("match_scores_kernel");
}

}  // extern "C"
