// mvm_boxfit.hip — the translation of a pose fitted to the detected boxes,
// given the model: per table row, the t for which the bounding
// box of the model's projected vertices under (R, t) best matches the detected
// box in every kept view, by the damped Gauss-Newton descent of §3.17 from the
// table's X.  Every step and its order are stated by tests/box_fit_model.py,
// whose bits the kernel returns.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "mvmatch.h"
#include "mvm_device.h"
#include "mvm_internal.h"
#include "mvm_refine.h"

#pragma clang fp contract(off)

namespace {

constexpr int32_t kNoVertex = 0x7FFFFFFF;

struct BoxSums {
    double cost, A[6], g[3];     // A: A00 A01 A02 A11 A12 A22
};

// A lane's strict-first extreme: its value, its vertex (kNoVertex: none yet)
// and that vertex's depth.
struct Extreme {
    double p, h2;
    int32_t i;
};

// The lane that holds the wave's extreme: `key` is the lane's value (a
// maximum: its negation; +inf where it has none), `idx` its vertex.  The wave
// takes the smallest key and, among the lanes holding it, the lowest vertex:
// no order of evaluation changes a minimum, so this is the model's strict
// ascending scan.  -0 == +0 here as there, and the value is read from the
// winning lane, not from the reduction.  No lane has a vertex: lane 0, whose
// extreme is (+-inf, NaN) like every other's.
__device__ __forceinline__ int extreme_lane(double key, int32_t idx) {
    const double m = wave_min_f64(key);
    const uint64_t hit = __ballot(key == m);
    if (__builtin_popcountll(hit) == 1) return (int)__builtin_ctzll(hit);
    const int32_t w = wave_min_i32(key == m ? idx : kNoVertex);
    return (int)__builtin_ctzll(__ballot(key == m && idx == w));
}

// cost, A and g at t over the views of `mask`, ascending.  The view loop is a
// run-time loop over the camera slots: P and the box of a view are read where
// they are used (uniform addresses), so no register array is indexed by c.
// `resid_row` (may be NULL): lane 0 writes the four residuals of every kept
// view and NaN for the others.
__device__ __forceinline__ void box_sums(const double *__restrict__ proj_s, const int32_t *__restrict__ box_row,
                                         uint32_t mask, int n_cams, const double (&R)[9],
                                         const double *__restrict__ verts, int n_verts, int lane, double t0,
                                         double t1, double t2, BoxSums &e, double *__restrict__ resid_row) {
    e.cost = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) e.A[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) e.g[q] = 0.0;
    const double qnan = __builtin_nan("");
    bool invalid = false;
#pragma unroll 1
    for (int c = 0; c < n_cams; ++c) {
        if (!((mask >> c) & 1u)) {
            if (resid_row != nullptr && lane == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) resid_row[4 * c + k] = qnan;
            }
            continue;
        }
        const double *__restrict__ p = proj_s + 12 * c;
        double M[9], cc[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                M[3 * q + j] = (p[4 * q] * R[j] + p[4 * q + 1] * R[3 + j]) + p[4 * q + 2] * R[6 + j];
            cc[q] = ((p[4 * q] * t0 + p[4 * q + 1] * t1) + p[4 * q + 2] * t2) + p[4 * q + 3];
        }
        Extreme x[4] = {{INFINITY, qnan, kNoVertex},
                        {INFINITY, qnan, kNoVertex},
                        {-INFINITY, qnan, kNoVertex},
                        {-INFINITY, qnan, kNoVertex}};           // umin, vmin, umax, vmax
        bool bad = false;
        for (int i = lane; i < n_verts; i += kWave) {
            const double vx = verts[3 * (int64_t)i], vy = verts[3 * (int64_t)i + 1], vz = verts[3 * (int64_t)i + 2];
            const double h0 = ((M[0] * vx + M[1] * vy) + M[2] * vz) + cc[0];
            const double h1 = ((M[3] * vx + M[4] * vy) + M[5] * vz) + cc[1];
            const double h2 = ((M[6] * vx + M[7] * vy) + M[8] * vz) + cc[2];
            bad = bad || !(h2 > 0.0);
            const double u = h0 / h2, v = h1 / h2;
            if (u < x[0].p) x[0] = {u, h2, i};
            if (v < x[1].p) x[1] = {v, h2, i};
            if (u > x[2].p) x[2] = {u, h2, i};
            if (v > x[3].p) x[3] = {v, h2, i};
        }
        invalid = invalid || __ballot(bad) != 0;
        double r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int l = extreme_lane(k < 2 ? x[k].p : -x[k].p, x[k].i);
            const double pe = read_lane(x[k].p, l), h2 = read_lane(x[k].h2, l);
            r[k] = pe - (double)box_row[4 * c + k];
            e.cost = e.cost + r[k] * r[k];
            const int q = 4 * (k & 1);       // a u edge reads P's row 0, a v edge row 1
            const double a0 = (p[q] - pe * p[8]) / h2, a1 = (p[q + 1] - pe * p[9]) / h2,
                         a2 = (p[q + 2] - pe * p[10]) / h2;
            e.A[0] = e.A[0] + a0 * a0;
            e.A[1] = e.A[1] + a0 * a1;
            e.A[2] = e.A[2] + a0 * a2;
            e.A[3] = e.A[3] + a1 * a1;
            e.A[4] = e.A[4] + a1 * a2;
            e.A[5] = e.A[5] + a2 * a2;
            e.g[0] = e.g[0] + a0 * r[k];
            e.g[1] = e.g[1] + a1 * r[k];
            e.g[2] = e.g[2] + a2 * r[k];
        }
        if (resid_row != nullptr && lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) resid_row[4 * c + k] = r[k];
        }
    }
    if (invalid) e.cost = INFINITY;
}

__device__ __forceinline__ bool sums_finite(const BoxSums &e) {
    bool finite = true;
#pragma unroll
    for (int q = 0; q < 6; ++q) finite &= refine_finite(e.A[q]);
#pragma unroll
    for (int q = 0; q < 3; ++q) finite &= refine_finite(e.g[q]);
    return finite;
}

// One wave per row of the range, four rows per workgroup.  The row is
// wave-uniform, so P, M, c, the box and the whole 3 x 3 solve are the same in
// every lane; the lanes stride over the vertices.  The step and the loop are
// refine_points_kernel's (mvm_pipeline.hip), with t for X.
__global__ __launch_bounds__(kThreads) void fit_boxes_kernel(
    const double *__restrict__ pose, const int32_t *__restrict__ scene, int32_t scene_base,
    const int32_t *__restrict__ views, const int32_t *__restrict__ boxes, int64_t n_rows, int32_t n_cams,
    const double *__restrict__ proj, int32_t n_scenes, const double *__restrict__ verts, int32_t n_verts,
    int32_t max_evals, double *__restrict__ pose_out, double *__restrict__ rms, int32_t *__restrict__ info,
    double *__restrict__ cov, double *__restrict__ resid) {
    const int lane = threadIdx.x % kWave;
    const int64_t row = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (row >= n_rows) return;
    const double *__restrict__ pr = pose + 16 * row;
    const int64_t s = (int64_t)scene[row] - scene_base;
    uint32_t mask = 0;
#pragma unroll 1
    for (int c = 0; c < n_cams; ++c) mask |= views[row * n_cams + c] >= 0 ? 1u << c : 0u;
    const bool fit = s >= 0 && s < n_scenes && mask != 0;
    const double qnan = __builtin_nan("");
    const double Ti0 = pr[3], Ti1 = pr[7], Ti2 = pr[11];
    double T0 = Ti0, T1 = Ti1, T2 = Ti2, rms0 = qnan, rms1 = qnan;
    int32_t status = 3, evals = 0;
    BoxSums cur;
#pragma unroll
    for (int q = 0; q < 6; ++q) cur.A[q] = qnan;
    double *resid_row = resid != nullptr ? resid + row * n_cams * 4 : nullptr;
    if (fit) {
        double R[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) R[3 * i + j] = pr[4 * i + j];
        }
        const double *__restrict__ proj_s = proj + s * n_cams * 12;
        const int32_t *__restrict__ box_row = boxes + row * n_cams * 4;
        box_sums(proj_s, box_row, mask, n_cams, R, verts, n_verts, lane, T0, T1, T2, cur, nullptr);
        const double cost0 = cur.cost;
        double cost = cost0, lam = 1e-3;
        status = refine_finite(cost) ? -1 : 2;
        if (status < 0 && !sums_finite(cur)) status = 2;
        while (status < 0) {
            RefineLdlt f;
            const bool pivots = refine_ldlt(cur.A[0] + lam * cur.A[0], cur.A[1], cur.A[2],
                                            cur.A[3] + lam * cur.A[3], cur.A[4], cur.A[5] + lam * cur.A[5], f);
            const double y0 = -cur.g[0];
            const double y1 = -cur.g[1] - f.l10 * y0;
            const double y2 = (-cur.g[2] - f.l20 * y0) - f.l21 * y1;
            const double z0 = y0 / f.d0, z1 = y1 / f.d1, z2 = y2 / f.d2;
            const double e2 = z2;
            const double e1 = z1 - f.l21 * e2;
            const double e0 = (z0 - f.l10 * e1) - f.l20 * e2;
            if (!pivots || !(refine_finite(e0) && refine_finite(e1) && refine_finite(e2))) {
                status = 2;
                break;
            }
            if ((e0 * e0 + e1 * e1) + e2 * e2 <= 1e-20 * ((T0 * T0 + T1 * T1) + T2 * T2)) {
                status = 0;
                break;
            }
            if (evals == max_evals) {
                status = 1;
                break;
            }
            ++evals;
            const double Y0 = T0 + e0, Y1 = T1 + e1, Y2 = T2 + e2;
            BoxSums tr;
            box_sums(proj_s, box_row, mask, n_cams, R, verts, n_verts, lane, Y0, Y1, Y2, tr, nullptr);
            if (tr.cost < cost) {                    // a NaN fails this
                T0 = Y0, T1 = Y1, T2 = Y2;
                cost = tr.cost;
                cur = tr;
                lam = fmax(lam / 10.0, 1e-15);
                if (!sums_finite(cur)) status = 2;
            } else {
                lam = lam * 10.0;
            }
        }
        if (status == 2) {                           // the input stands
            T0 = Ti0, T1 = Ti1, T2 = Ti2;
            cost = cost0;
        }
        // the same operations at the same point give the same bits: A of a
        // rolled-back row and the residuals come from one more evaluation
        if (resid_row != nullptr || (cov != nullptr && status == 2))
            box_sums(proj_s, box_row, mask, n_cams, R, verts, n_verts, lane, T0, T1, T2, cur, resid_row);
        const double k4 = 4.0 * (double)__builtin_popcount(mask);
        rms0 = sqrt(cost0 / k4);
        rms1 = sqrt(cost / k4);
    } else if (resid_row != nullptr && lane < 4 * n_cams) {
        resid_row[lane] = qnan;
    }
    if (lane < 16) {                                 // R and the bottom row bit for bit
        double v = pr[lane];
        v = lane == 3 ? T0 : lane == 7 ? T1 : lane == 11 ? T2 : v;
        pose_out[16 * row + lane] = v;
    }
    if (lane == 0) {
        rms[2 * row] = rms0;
        rms[2 * row + 1] = rms1;
        info[2 * row] = status;
        info[2 * row + 1] = evals;
        if (cov != nullptr) {
            double c00 = qnan, c01 = qnan, c02 = qnan, c11 = qnan, c12 = qnan, c22 = qnan;
            RefineLdlt f;
            // A^-1 = L^-T D^-1 L^-1 of the undamped A at t_out (a skipped row's A is NaN)
            if (refine_ldlt(cur.A[0], cur.A[1], cur.A[2], cur.A[3], cur.A[4], cur.A[5], f)) {
                const double i0 = 1.0 / f.d0, i1 = 1.0 / f.d1, i2 = 1.0 / f.d2;
                const double m20 = f.l10 * f.l21 - f.l20;
                const double q2 = f.l21 * i2, p1 = f.l10 * i1, r2 = m20 * i2;
                c00 = (i0 + f.l10 * p1) + m20 * r2;
                c01 = -p1 - m20 * q2;
                c02 = r2;
                c11 = i1 + f.l21 * q2;
                c12 = -q2;
                c22 = i2;
            }
            cov[6 * row] = c00;
            cov[6 * row + 1] = c01;
            cov[6 * row + 2] = c02;
            cov[6 * row + 3] = c11;
            cov[6 * row + 4] = c12;
            cov[6 * row + 5] = c22;
        }
    }
}

}  // namespace

extern "C" {

int mvm_fit_boxes(const double *pose_dev, const int32_t *scene_dev, int32_t scene_base, const int32_t *views_dev,
                  const int32_t *boxes_dev, int64_t n_rows, int32_t n_cams, const double *proj_dev,
                  int32_t n_scenes, const double *verts_dev, int32_t n_verts, int32_t max_evals,
                  double *pose_out_dev, double *rms_dev, int32_t *info_dev, double *cov_dev, double *resid_dev,
                  mvm_stream_t stream) {
    mvm_clear_error();
    if (n_rows == 0) return MVM_OK;
    if (n_rows < 0) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_rows=%lld is negative", (long long)n_rows);
    if (n_scenes < 0) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_scenes=%d is negative", n_scenes);
    if (n_cams < 3 || n_cams > MVM_MAX_CAMS)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_cams=%d outside [3, %d]", n_cams, MVM_MAX_CAMS);
    if (n_verts < 1) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_verts=%d: at least 1", n_verts);
    if (max_evals < 1 || max_evals > 64)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "max_evals=%d outside [1, 64]", max_evals);
    if (const int st = mvm_require_ptrs({{pose_dev, "pose_dev"},
                                         {scene_dev, "scene_dev"},
                                         {views_dev, "views_dev"},
                                         {boxes_dev, "boxes_dev"},
                                         {proj_dev, "proj_dev"},
                                         {verts_dev, "verts_dev"},
                                         {pose_out_dev, "pose_out_dev"},
                                         {rms_dev, "rms_dev"},
                                         {info_dev, "info_dev"}}))
        return st;                       // cov_dev and resid_dev may be NULL: not written
    const int64_t grid = (n_rows + kWaves - 1) / kWaves;
    if (grid > kMaxGridBlocks)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_rows=%lld: more rows than one launch holds; split the rows",
                        (long long)n_rows);
    // 16 n_rows doubles each; n_rows <= 4 kMaxGridBlocks, so no product overflows
    const uintptr_t in = reinterpret_cast<uintptr_t>(pose_dev), out = reinterpret_cast<uintptr_t>(pose_out_dev);
    const uintptr_t bytes = (uintptr_t)n_rows * 16 * sizeof(double);
    if (in < out + bytes && out < in + bytes)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "pose_out_dev overlaps pose_dev: the input is kept");
    fit_boxes_kernel<<<(unsigned)grid, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        pose_dev, scene_dev, scene_base, views_dev, boxes_dev, n_rows, n_cams, proj_dev, n_scenes, verts_dev,
        n_verts, max_evals, pose_out_dev, rms_dev, info_dev, cov_dev, resid_dev);
    return mvm_check_launch("fit_boxes_kernel");
}

}  // extern "C"
