// mvm_pipeline.hip — the device steps on either side of the matcher
// (SURVEY §8f #3 and #4), so a batch can go detector -> matcher -> 3-D
// centres without a host round trip.
//
//  * mvm_pack_detections: the box packing of PoseEstimator._detect
//    (bpc/inference/process_pose.py:122-140): keep boxes whose class equals
//    class_id and whose float32 confidence >= the float32 threshold (:130), in
//    input order; truncate xyxy to int (:134, Python int() of a float32 =
//    truncation toward zero); centre = 0.5 * (x1 + x2) (:135-136) in float64,
//    exact.  Output is the matcher's CSR input (pts f64 [n, 2] + offsets).
//  * mvm_triangulate_dlt: triangulate_multi_view (epipolar_matching.py:118-127)
//    as called by PosePrediction.triangulate (process_pose.py:86-94): A is
//    the 2V x 4 DLT system, X the right singular vector of its smallest
//    singular value, returned as X[:3] / X[3].  One-sided Jacobi SVD in fp64,
//    one thread per point (tolerance parity with LAPACK's gesdd: the vector
//    is unique up to sign, which X[:3]/X[3] cancels).
//  * mvm_rig_matrices: compute_fundamental_matrix (camera_utils.py:23-46) per
//    (capture, pair) and P = K @ RT[:3] (process_pose.py:91) per (capture,
//    camera) for pinhole K, so a batch whose rigs differ needs no host numpy.
//  * mvm_mark_used, mvm_leftover_counts, mvm_leftover_gather: the sub-batch of
//    an extra seed pass over a C-camera batch: the detections no
//    earlier match holds, compacted per view in order, cameras reordered.
//  * mvm_refine_points: the minimiser of the summed squared reprojection
//    error from the DLT point, with its covariance.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "mvmatch.h"
#include "mvm_device.h"
#include "mvm_internal.h"
#include "mvm_refine.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPackThreads = 256;

// ---------------------------------------------------------- packing ----
__device__ __forceinline__ bool keep_box(const float *conf, const float *cls, int64_t k,
                                         float thresh, float class_id) {
    return (cls[k] == class_id) && (conf[k] >= thresh);
}

// per image: number of kept boxes
__global__ __launch_bounds__(kPackThreads) void pack_count_kernel(
    const float *conf, const float *cls, const int64_t *img_offs, float thresh, float class_id,
    int32_t *counts) {
    __shared__ int s_cnt;
    const int img = blockIdx.x;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int64_t b = img_offs[img], e = img_offs[img + 1];
    int c = 0;
    for (int64_t k = b + threadIdx.x; k < e; k += kPackThreads) c += keep_box(conf, cls, k, thresh, class_id);
    atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) counts[img] = s_cnt;
}

// exclusive prefix of the counts -> CSR offsets (one workgroup; chunked scan)
__global__ __launch_bounds__(1024) void pack_scan_kernel(const int32_t *counts, int32_t n,
                                                         int64_t *offs) {
    // each thread sums a contiguous range; the 1024 partial sums are scanned
    // with wave shuffles (64 lanes) and once more over the 16 wave totals
    __shared__ int64_t s_wave[16];
    const int t = threadIdx.x, lane = t % 64, wave = t / 64;
    const int64_t per = (n + 1023) / 1024;
    const int64_t b = (int64_t)t * per, e = min<int64_t>(n, b + per);
    int64_t sum = 0;
    for (int64_t k = b; k < e; ++k) sum += counts[k];
    int64_t x = sum;                                  // inclusive scan in the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    if (wave == 0) {                                  // inclusive scan of the wave totals
        int64_t w = lane < 16 ? s_wave[lane] : 0;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const int64_t y = __shfl_up(w, d, 64);
            if (lane >= d) w += y;
        }
        if (lane < 16) s_wave[lane] = w;
    }
    __syncthreads();
    int64_t run = x - sum + (wave > 0 ? s_wave[wave - 1] : 0);   // exclusive prefix
    if (t == 1023) offs[n] = run + sum;
    for (int64_t k = b; k < e; ++k) {
        offs[k] = run;
        run += counts[k];
    }
}

// per image: order-preserving compaction of the kept boxes
__global__ __launch_bounds__(kPackThreads) void pack_write_kernel(
    const float *boxes, const float *conf, const float *cls, const int64_t *img_offs,
    float thresh, float class_id, const int64_t *out_offs, double *pts, int32_t *boxes_out,
    int32_t *status) {
    __shared__ int s_wave[kPackThreads / 64];
    __shared__ int s_base;
    const int img = blockIdx.x;
    const int t = threadIdx.x, lane = t % 64, wave = t / 64;
    const int64_t b = img_offs[img], e = img_offs[img + 1];
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int64_t k0 = b; k0 < e; k0 += kPackThreads) {
        const int64_t k = k0 + t;
        const bool keep = k < e && keep_box(conf, cls, k, thresh, class_id);
        const uint64_t m = __ballot(keep);
        const int in_wave = __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __builtin_popcountll(m);
        __syncthreads();
        int before = s_base;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (keep) {
            const int64_t o = out_offs[img] + before + in_wave;
            int32_t q[4];
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float f = boxes[4 * k + c];
                ok &= isfinite(f) && fabsf(f) < 1073741824.0f;   // |x| < 2^30
                q[c] = ok ? (int32_t)f : 0;                        // int(): toward zero
            }
            if (!ok) atomicOr(status, 1);
#pragma unroll
            for (int c = 0; c < 4; ++c) boxes_out[4 * o + c] = q[c];
            pts[2 * o] = 0.5 * (double)(q[0] + q[2]);
            pts[2 * o + 1] = 0.5 * (double)(q[1] + q[3]);
        }
        __syncthreads();
        if (t == 0) {
            int tot = 0;
            for (int w = 0; w < kPackThreads / 64; ++w) tot += s_wave[w];
            s_base += tot;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------- DLT ----
constexpr int kMaxViews = MVM_MAX_CAMS;

// One-sided (Hestenes) Jacobi SVD of the 2V x 4 DLT system, fp64, fully
// unrolled for a compile-time V so A and the rotations stay in registers:
// rotate column pairs until every pair is orthogonal to one ulp; V
// accumulates the rotations.  The right singular vector of the smallest
// singular value is the column of V whose rotated A-column has the smallest
// norm.  P: V row-major 3x4 matrices; xy: V points.
template <int NV>
__device__ __forceinline__ void dlt_point(const double *P, const double *xy, double X[3]) {
    constexpr int m = 2 * NV;
    double A[m][4];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const double x = xy[2 * v], y = xy[2 * v + 1];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double p2 = P[12 * v + 8 + c];
            A[2 * v][c] = x * p2 - P[12 * v + c];          // x * P[2] - P[0]   (:122)
            A[2 * v + 1][c] = y * p2 - P[12 * v + 4 + c];  // y * P[2] - P[1]   (:123)
        }
    }
    double W[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = a + 1; b < 4; ++b) {
                double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
                for (int r = 0; r < m; ++r) {
                    alpha += A[r][a] * A[r][a];
                    beta += A[r][b] * A[r][b];
                    gamma += A[r][a] * A[r][b];
                }
                if (fabs(gamma) > 2.220446049250313e-16 * sqrt(alpha * beta)) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int r = 0; r < m; ++r) {
                        const double ra = A[r][a], rb = A[r][b];
                        A[r][a] = c * ra - s * rb;
                        A[r][b] = s * ra + c * rb;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double va = W[r][a], vb = W[r][b];
                        W[r][a] = c * va - s * vb;
                        W[r][b] = s * va + c * vb;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    double n2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        n2[c] = 0;
#pragma unroll
        for (int r = 0; r < m; ++r) n2[c] += A[r][c] * A[r][c];
    }
    double x0 = W[0][0], x1 = W[1][0], x2 = W[2][0], w = W[3][0], bn = n2[0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        if (n2[c] < bn) {
            bn = n2[c];
            x0 = W[0][c], x1 = W[1][c], x2 = W[2][c], w = W[3][c];
        }
    }
    X[0] = x0 / w;
    X[1] = x1 / w;
    X[2] = x2 / w;
}

template <int NV>
__global__ __launch_bounds__(256) void dlt_kernel(const double *proj, const int32_t *set_of_point,
                                                  const double *pts2d, int32_t n_points,
                                                  double *X) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_points) return;
    const int64_t set = set_of_point ? (int64_t)set_of_point[p] : p;
    double xy[2 * NV], out[3];
#pragma unroll
    for (int k = 0; k < 2 * NV; ++k) xy[k] = pts2d[p * 2 * NV + k];
    dlt_point<NV>(proj + set * NV * 12, xy, out);
    X[3 * p + 0] = out[0];
    X[3 * p + 1] = out[1];
    X[3 * p + 2] = out[2];
}

// ------------------------------- shared by the match and view kernels ----
// The pieces the kernels below have in common, each written once.
constexpr int kCompactThreads = 256;
constexpr int kCompactScenes = kCompactThreads / 64;

// One wave per item (a capture, or one view of a capture), four items to a
// workgroup, lanes striding over the item's rows: no LDS, no barrier.  The
// wave's item comes back as a scalar, so what it indexes (offsets, the
// capture's P) is read by scalar loads ahead of the row loop; -1 beyond n_items.
__device__ __forceinline__ int64_t wave_item(int64_t n_items, int &lane) {
    lane = threadIdx.x % 64;
    const int64_t item = (int64_t)blockIdx.x * kCompactScenes +
                         __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    return item < n_items ? item : -1;
}

// capture s's matches: rows mo .. mo + n, never more than match_offs leaves it
struct MatchRange { int64_t mo, n; };
__device__ __forceinline__ MatchRange match_range(const int64_t *match_offs, const int32_t *count,
                                                  int64_t s) {
    const int64_t mo = match_offs[s];
    return {mo, min<int64_t>(count[s], match_offs[s + 1] - mo)};
}

// The view rule.  vw: a row's C view slots, co: its capture's cam_offs (C + 1
// entries are readable: cam_offs holds C S + 1).  A slot c < n_cams with
// v >= 0 is kept (its bit in the mask) if v is a detection of its view,
// v < co[c + 1] - co[c]; if it is not, the row is not `ok` and no index of it
// may be used.  A slot < 0 is no view and says nothing about `ok`.  The slot
// loop is compile-time under `c < n_cams`.
//  * refine_points_kernel asked exactly this of every slot; a seed < 0 is not
//    in the mask, and fewer than two kept views are its status 3, not `!ok`.
//  * prune_views_kernel asked `0 <= v < size` of the seeds and `v < size` of
//    the extras (negative: no view), kept the extras >= 0, and left a row that
//    failed alone: seeded_views, below -- a seed passes the old test exactly
//    when its bit is set, and `ok` covers an extra that is >= 0 and too large.
//  * extend_select_triangulate_kernel asked the same of the seeds and kept the
//    extras by sign alone.  It wrote those slots itself: -1, or an l it had
//    checked against nd = co[3 + e + 1] - co[3 + e], the size the rule reads,
//    so the size test it now makes of them never fails: seeded_views again.
__device__ __forceinline__ uint32_t kept_views(const int32_t *vw, const int64_t *co, int n_cams,
                                               bool &ok) {
    uint32_t mask = 0u;
    ok = true;
#pragma unroll
    for (int c = 0; c < MVM_MAX_CAMS; ++c) {
        if (c < n_cams) {
            const int32_t v = vw[c];
            const bool in_view = v < co[c + 1] - co[c];
            if (v >= 0 && in_view) mask |= 1u << c;
            ok &= v < 0 || in_view;
        }
    }
    return mask;
}

// kept_views of a row that stands on its three seeds: the mask, or 7 (no
// extra view: the row is left as it is) when the row is not ok or a seed is not kept
__device__ __forceinline__ uint32_t seeded_views(const int32_t *vw, const int64_t *co, int n_cams) {
    bool ok;
    const uint32_t mask = kept_views(vw, co, n_cams, ok);
    return ok && (mask & 7u) == 7u ? mask : 7u;
}

// the centroids of the views of `mask` (kept views: every index is checked),
// by compile-time slot: no register array is indexed by a runtime value
__device__ __forceinline__ void gather_centroids(const double *pts, const int64_t *co,
                                                 const int32_t *vw, uint32_t mask,
                                                 double (&cx)[MVM_MAX_CAMS],
                                                 double (&cy)[MVM_MAX_CAMS]) {
#pragma unroll
    for (int c = 0; c < MVM_MAX_CAMS; ++c) {
        if ((mask >> c) & 1u) {
            const int64_t row = co[c] + vw[c];
            cx[c] = pts[2 * row];
            cy[c] = pts[2 * row + 1];
        }
    }
}

// h = P (X, 1) for a row-major 3x4 P: every product and sum rounded on its
// own (this file's fp contract(off)), associated ((p0 X0 + p1 X1) + p2 X2) + p3
struct Homog { double h0, h1, h2; };
__device__ __forceinline__ Homog project(const double *p, double X0, double X1, double X2) {
    return {((p[0] * X0 + p[1] * X1) + p[2] * X2) + p[3], ((p[4] * X0 + p[5] * X1) + p[6] * X2) + p[7],
            ((p[8] * X0 + p[9] * X1) + p[10] * X2) + p[11]};
}

// One detection row -- a 16-byte box and a 16-byte centroid -- read from row
// `row` of the packer's arrays, or written to row o of a table's.  VEC: as
// 16-byte accesses (every base 16-byte aligned), else element by element.
struct Detection { int4 box; double2 cent; };
template <bool VEC>
__device__ __forceinline__ Detection load_detection(const int32_t *boxes, const double *pts, int64_t row) {
    if (VEC)
        return {reinterpret_cast<const int4 *>(boxes)[row], reinterpret_cast<const double2 *>(pts)[row]};
    return {make_int4(boxes[4 * row], boxes[4 * row + 1], boxes[4 * row + 2], boxes[4 * row + 3]),
            make_double2(pts[2 * row], pts[2 * row + 1])};
}
template <bool VEC>
__device__ __forceinline__ void store_detection(int32_t *boxes_out, double *cent_out, int64_t o,
                                                const Detection &d) {
    if (VEC) {
        reinterpret_cast<int4 *>(boxes_out)[o] = d.box;
        reinterpret_cast<double2 *>(cent_out)[o] = d.cent;
    } else {
        boxes_out[4 * o] = d.box.x, boxes_out[4 * o + 1] = d.box.y;
        boxes_out[4 * o + 2] = d.box.z, boxes_out[4 * o + 3] = d.box.w;
        cent_out[2 * o] = d.cent.x, cent_out[2 * o + 1] = d.cent.y;
    }
}

// ------------------------------------------- select + triangulate ----
// The tail of PoseEstimator._match for a batch of 3-camera captures
// (process_pose.py:182-187 with match_objects :100-116): for scene s, the
// assignment (row_ind, col_ind) of its flattened (N*M, P) cube is filtered by
// cost < threshold, decoded i = r / M, j = r % M, k = c, stably sorted by
// cost (Python's sorted on the float32 cube values; ties keep the
// assignment's ascending-row order), and each match's centroids are
// triangulated.  One workgroup per scene; ranks by counting through an LDS
// tile of costs (non-kept entries are +inf and never precede a kept one).
constexpr int kSelThreads = 256;
constexpr int kSelTile = 1024;

// the cube entry (r, k) of scene s: read from the cube, or -- cube-free
// (mvm_select_triangulate_resid) -- recomputed from the scene's fp64 pair
// residuals (mvm_triplet_minima's layout) with the cube's own arithmetic
struct SelSrc {
    const float *cb;
    const double *e12, *e13t, *e23t;   // e12 != nullptr: the residual form
    int64_t M, P;
    int64_t rows;   // N * M
    int ld;
    // the value select compares: the entry's, or +inf (kept under no threshold)
    // for a pair that is not an index of the scene's (N*M, P) problem -- what a
    // problem whose assignment failed leaves in its row_ind / col_ind region
    __device__ __forceinline__ float at_checked(int64_t r, int64_t k) const {
        return (r >= 0 && r < rows && k >= 0 && k < P) ? at(r, k) : INFINITY;
    }
    __device__ __forceinline__ float at(int64_t r, int64_t k) const {
        if (e12) {
            const int64_t i = r / M, j = r - i * M;
            return cube_f32(e12[i * ld + j], e13t[k * ld + i], e23t[k * ld + j]);
        }
        return cb[r * P + k];
    }
};

__global__ __launch_bounds__(kSelThreads) void select_triangulate_kernel(
    const float *cube, const int64_t *cube_offs, const int64_t *cam_offs,
    const int64_t *lsap_offs, const int64_t *row_ind, const int64_t *col_ind, const double *pts,
    const double *proj, double threshold, int32_t *match, float *cost_out, double *X,
    int32_t *count, const double *resid, int64_t rstride, int32_t rld, int32_t rrows) {
    __shared__ float s_cost[kSelTile];
    __shared__ int s_kept;
    const int s = blockIdx.x, t = threadIdx.x;
    const int64_t o = lsap_offs[s], n = lsap_offs[s + 1] - o;
    const int64_t c0 = cam_offs[3 * s], c1 = cam_offs[3 * s + 1], c2 = cam_offs[3 * s + 2];
    const int64_t M = c2 - c1, P = cam_offs[3 * s + 3] - c2;
    SelSrc cb{};
    cb.M = M;
    cb.P = P;
    cb.rows = (c1 - c0) * M;
    if (resid) {
        cb.ld = rld;
        cb.e12 = resid + (int64_t)s * rstride;
        cb.e13t = cb.e12 + (int64_t)rrows * rld;
        cb.e23t = cb.e13t + (int64_t)rrows * rld;
    } else {
        cb.cb = cube + cube_offs[s];
    }
    if (t == 0) s_kept = 0;
    for (int64_t m0 = 0; m0 < n; m0 += kSelThreads) {
        const int64_t m = m0 + t;
        float mine = INFINITY;
        if (m < n) {
            const float v = cb.at_checked(row_ind[o + m], col_ind[o + m]);
            if ((double)v < threshold) mine = v;
        }
        int64_t rank = 0;
        for (int64_t q0 = 0; q0 < n; q0 += kSelTile) {
            __syncthreads();
            for (int q = t; q < kSelTile && q0 + q < n; q += kSelThreads) {
                const float v = cb.at_checked(row_ind[o + q0 + q], col_ind[o + q0 + q]);
                s_cost[q] = (double)v < threshold ? v : INFINITY;
            }
            __syncthreads();
            if (mine < INFINITY) {
                const int lim = (int)min<int64_t>(kSelTile, n - q0);
                for (int q = 0; q < lim; ++q) {
                    const float v = s_cost[q];
                    rank += (v < mine) || (v == mine && q0 + q < m);
                }
            }
        }
        if (mine < INFINITY) {
            atomicAdd(&s_kept, 1);
            const int64_t r = row_ind[o + m], k = col_ind[o + m];
            const int64_t i = r / M, j = r % M, w = o + rank;
            match[3 * w + 0] = (int32_t)i;
            match[3 * w + 1] = (int32_t)j;
            match[3 * w + 2] = (int32_t)k;
            cost_out[w] = mine;
            double xy[6], out[3];
            xy[0] = pts[2 * (c0 + i)], xy[1] = pts[2 * (c0 + i) + 1];
            xy[2] = pts[2 * (c1 + j)], xy[3] = pts[2 * (c1 + j) + 1];
            xy[4] = pts[2 * (c2 + k)], xy[5] = pts[2 * (c2 + k) + 1];
            dlt_point<3>(proj + (int64_t)s * 36, xy, out);
            X[3 * w + 0] = out[0];
            X[3 * w + 1] = out[1];
            X[3 * w + 2] = out[2];
        }
    }
    __syncthreads();
    if (t == 0) count[s] = s_kept;
}

// ------------------------------------------- extension: select + DLT ----
// The tail of the extension into extra cameras, after
// mvm_extend_costs and the assignment of every (n, n_d) matrix: per capture,
// views[w] = (i, j, k, -1, ...) and ext_cost[w] = +inf for its count matches;
// each assigned pair (w, l) of extra camera d with (double)E_d[w][l] <
// threshold (select_triangulate's compare) sets views[w][d] = l and
// ext_cost[w][d - 3]; a match that kept an extra view is triangulated again
// over its V views in ascending camera order, a match that kept none keeps
// the X it came with.  One workgroup per capture; a row is assigned at most
// once per camera, so the scatter has no conflicting writers.

// DLT of one match over the NV cameras whose bits `mask` holds, ascending: the
// P and centroids are gathered by constant slot (the camera of a slot comes
// from the mask, so no register array is indexed dynamically).
template <int NV>
__device__ __forceinline__ void extend_dlt(const double *proj_s, const double *pts,
                                           const int64_t *co, const int32_t *vw, uint32_t mask,
                                           double X[3]) {
    double P[12 * NV], xy[2 * NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int cam = __builtin_ctz(mask);
        mask &= mask - 1u;
        const int64_t row = co[cam] + vw[cam];
        xy[2 * v] = pts[2 * row];
        xy[2 * v + 1] = pts[2 * row + 1];
#pragma unroll
        for (int k = 0; k < 12; ++k) P[12 * v + k] = proj_s[12 * cam + k];
    }
    dlt_point<NV>(P, xy, X);
}

// extend_dlt<V> over the V = popcount(mask) views of the mask, instantiated
// for LO .. HI only (a count above HI takes HI's, as a switch's default would)
template <int LO, int HI>
__device__ __forceinline__ void mask_dlt(const double *proj_s, const double *pts, const int64_t *co,
                                         const int32_t *vw, uint32_t mask, double X[3]) {
    if constexpr (LO < HI) {
        if (__builtin_popcount(mask) == LO) return extend_dlt<LO>(proj_s, pts, co, vw, mask, X);
        return mask_dlt<LO + 1, HI>(proj_s, pts, co, vw, mask, X);
    } else {
        extend_dlt<HI>(proj_s, pts, co, vw, mask, X);
    }
}

__global__ __launch_bounds__(kSelThreads) void extend_select_triangulate_kernel(
    const float *E, const int64_t *ext_offs, const int64_t *lsap_offs, const int64_t *row_ind,
    const int64_t *col_ind, const int32_t *match, const int64_t *match_offs, const int32_t *count,
    const double *pts, const int64_t *cam_offs, const double *proj, double threshold,
    int32_t n_cams, int32_t *views, float *ext_cost, double *X) {
    const int64_t s = blockIdx.x;
    const int t = threadIdx.x;
    const int n_ext = n_cams - 3;
    const auto [mo, n] = match_range(match_offs, count, s);
    const int64_t *co = cam_offs + s * n_cams;
    for (int64_t w = t; w < n; w += kSelThreads) {
        int32_t *vw = views + (mo + w) * n_cams;
#pragma unroll
        for (int c = 0; c < 3; ++c) vw[c] = match[3 * (mo + w) + c];
        for (int c = 3; c < n_cams; ++c) vw[c] = -1;
        for (int e = 0; e < n_ext; ++e) ext_cost[(mo + w) * n_ext + e] = INFINITY;
    }
    __syncthreads();
    for (int e = 0; e < n_ext; ++e) {
        const int64_t sd = s * n_ext + e;
        const int64_t nd = co[3 + e + 1] - co[3 + e];
        if (nd <= 0) continue;
        const int64_t eo = ext_offs[sd], lo = lsap_offs[sd];
        const int64_t rows = min<int64_t>(n, (ext_offs[sd + 1] - eo) / nd);   // E_d's rows
        const int64_t na = min<int64_t>(min<int64_t>(rows, nd), lsap_offs[sd + 1] - lo);
        for (int64_t m = t; m < na; m += kSelThreads) {
            const int64_t r = row_ind[lo + m], l = col_ind[lo + m];
            // a failed assignment leaves its pairs unspecified: never an index
            if (r < 0 || r >= rows || l < 0 || l >= nd) continue;
            const float v = E[eo + r * nd + l];
            if ((double)v < threshold) {
                views[(mo + r) * n_cams + 3 + e] = (int32_t)l;
                ext_cost[(mo + r) * n_ext + e] = v;
            }
        }
    }
    __syncthreads();
    const double *proj_s = proj + s * n_cams * 12;
    for (int64_t w = t; w < n; w += kSelThreads) {
        const int32_t *vw = views + (mo + w) * n_cams;
        const uint32_t mask = seeded_views(vw, co, n_cams);
        if (mask == 7u) continue;             // the three-view X stands
        double out[3];
        mask_dlt<4, 8>(proj_s, pts, co, vw, mask, out);
        X[3 * (mo + w) + 0] = out[0];
        X[3 * (mo + w) + 1] = out[1];
        X[3 * (mo + w) + 2] = out[2];
    }
}

// ------------------------------------------------- match table ----
// The select kernels leave scene s's matches at lsap_offs[s] with slack rows
// behind them, as per-view indices.  This copies them to dense rows
// dense_offs[s] + w and resolves the indices against the packer's rows, so a
// row stands on its own (mvm_compact_matches).  One wave per scene
// (wave_item); VEC: the detection rows move as 16-byte accesses.

// The reprojection residual of X in one view (include/mvmatch.h,
// mvm_compact_matches_views): p the view's row-major 3x4 P, (cx, cy) its
// centroid.  `project`, then IEEE divisions and square root.
__device__ __forceinline__ double reproj_residual(const double *p, double X0, double X1, double X2,
                                                  double cx, double cy) {
    const Homog h = project(p, X0, X1, X2);
    const double du = h.h0 / h.h2 - cx, dv = h.h1 / h.h2 - cy;
    return sqrt(du * du + dv * dv);
}

template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void compact_matches_kernel(
    const int32_t *__restrict__ match, const float *__restrict__ cost, const double *__restrict__ X,
    const int32_t *__restrict__ count, const int64_t *__restrict__ seg_offs,
    const int64_t *__restrict__ dense_offs, const double *__restrict__ pts,
    const int32_t *__restrict__ boxes, const int64_t *__restrict__ cam_offs, int32_t n_scenes,
    int32_t scene_base, int32_t *__restrict__ scene_out, int32_t *__restrict__ match_out,
    float *__restrict__ cost_out, double *__restrict__ X_out, int32_t *__restrict__ boxes_out,
    double *__restrict__ cent_out) {
    int lane;
    const int64_t s = wave_item(n_scenes, lane);
    if (s < 0) return;
    const int64_t src = seg_offs[s], dst = dense_offs[s];
    const int32_t n = count[s];
    const int64_t c[3] = {cam_offs[3 * s], cam_offs[3 * s + 1], cam_offs[3 * s + 2]};
    for (int32_t w = lane; w < n; w += 64) {
        const int64_t a = src + w, r = dst + w;
        int32_t m[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) m[v] = match[3 * a + v];
        scene_out[r] = scene_base + (int32_t)s;
        cost_out[r] = cost[a];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            match_out[3 * r + v] = m[v];
            X_out[3 * r + v] = X[3 * a + v];
        }
#pragma unroll
        for (int v = 0; v < 3; ++v)
            store_detection<VEC>(boxes_out, cent_out, 3 * r + v, load_detection<VEC>(boxes, pts, c[v] + m[v]));
    }
}

// The table of a C-camera batch (mvm_compact_matches_views): the same copy
// over the C view slots of mvm_extend_select_triangulate's rows, -1 slots
// filled with (-1, -1, -1, -1) / NaN, plus the reprojection residual of X in
// every kept view (reproj_residual).  The capture's P (12 C doubles) and
// cam_offs are the same for every lane of the wave (wave_item): loaded once,
// ahead of the match loop and of every store.  The camera slot is a
// compile-time index (MVM_MAX_CAMS slots, `c < n_cams` predicated), so P and
// co stay in registers.
template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void compact_matches_views_kernel(
    const int32_t *__restrict__ views, const float *__restrict__ cost,
    const float *__restrict__ ext_cost, const double *__restrict__ X,
    const int32_t *__restrict__ count, const int64_t *__restrict__ seg_offs,
    const int64_t *__restrict__ dense_offs, const double *__restrict__ pts,
    const int32_t *__restrict__ boxes, const int64_t *__restrict__ cam_offs,
    const double *__restrict__ proj, int32_t n_scenes, int32_t n_cams, int32_t scene_base,
    int32_t *__restrict__ scene_out, int32_t *__restrict__ views_out, int32_t *__restrict__ nviews_out,
    float *__restrict__ cost_out, float *__restrict__ ext_cost_out, double *__restrict__ X_out,
    int32_t *__restrict__ boxes_out, double *__restrict__ cent_out, double *__restrict__ reproj_out) {
    int lane;
    const int64_t s = wave_item(n_scenes, lane);
    if (s < 0) return;
    const int64_t src = seg_offs[s], dst = dense_offs[s];
    const int32_t n = count[s];
    const int n_ext = n_cams - 3;
    int64_t co[MVM_MAX_CAMS];
    double P[12 * MVM_MAX_CAMS];
#pragma unroll
    for (int c = 0; c < MVM_MAX_CAMS; ++c) {
        if (c < n_cams) {
            co[c] = cam_offs[s * n_cams + c];
#pragma unroll
            for (int k = 0; k < 12; ++k) P[12 * c + k] = proj[(s * n_cams + c) * 12 + k];
        }
    }
    const double qnan = __builtin_nan("");
    for (int32_t w = lane; w < n; w += 64) {
        const int64_t a = src + w, r = dst + w;
        const double X0 = X[3 * a], X1 = X[3 * a + 1], X2 = X[3 * a + 2];
        scene_out[r] = scene_base + (int32_t)s;
        cost_out[r] = cost[a];
        X_out[3 * r] = X0;
        X_out[3 * r + 1] = X1;
        X_out[3 * r + 2] = X2;
        for (int e = 0; e < n_ext; ++e) ext_cost_out[r * n_ext + e] = ext_cost[a * n_ext + e];
        int32_t kept = 0;
#pragma unroll
        for (int c = 0; c < MVM_MAX_CAMS; ++c) {
            if (c < n_cams) {
                const int32_t v = views[a * n_cams + c];
                const int64_t o = r * n_cams + c;
                views_out[o] = v;
                if (v >= 0) {
                    ++kept;
                    const Detection d = load_detection<VEC>(boxes, pts, co[c] + v);
                    store_detection<VEC>(boxes_out, cent_out, o, d);
                    reproj_out[o] = reproj_residual(P + 12 * c, X0, X1, X2, d.cent.x, d.cent.y);
                } else {
                    store_detection<VEC>(boxes_out, cent_out, o,
                                         {make_int4(-1, -1, -1, -1), make_double2(qnan, qnan)});
                    reproj_out[o] = qnan;
                }
            }
        }
        nviews_out[r] = kept;
    }
}

// ------------------------------------------------- view pruning ----
// mvm_prune_views_triangulate: per match of a C-camera batch,
// drop the extra views whose reprojection residual exceeds `gate`, the worst
// one at a time, and triangulate again over what is left after every drop.
// One wave per capture (wave_item), so the extra cameras' P and the capture's
// cam_offs are scalar loads ahead of the match loop.  The kept set is the bit
// mask of seeded_views (a row that fails the view rule is left alone); the
// worst view is chosen over compile-time camera slots under the mask's bit,
// and the DLT gathers by constant slot (mask_dlt), so no register array is
// indexed by a runtime value.  A row that drops nothing is not written (its
// `pruned` word is 0).
constexpr int kPruneSlots = MVM_MAX_CAMS - 3;    // the extra cameras 3 .. 7

__global__ __launch_bounds__(kCompactThreads) void prune_views_kernel(
    const int64_t *__restrict__ match_offs, const int32_t *__restrict__ count,
    const double *__restrict__ pts, const int64_t *__restrict__ cam_offs,
    const double *__restrict__ proj, double gate, int32_t n_scenes, int32_t n_cams, int32_t *views,
    float *ext_cost, double *X, int32_t *__restrict__ pruned) {
    int lane;
    const int64_t s = wave_item(n_scenes, lane);
    if (s < 0) return;
    const auto [mo, n] = match_range(match_offs, count, s);
    const int n_ext = n_cams - 3;
    const int64_t *co_s = cam_offs + s * n_cams;
    const double *proj_s = proj + s * n_cams * 12;
    double P[12 * kPruneSlots];
#pragma unroll
    for (int e = 0; e < kPruneSlots; ++e)
        if (e < n_ext)
#pragma unroll
            for (int k = 0; k < 12; ++k) P[12 * e + k] = proj_s[12 * (3 + e) + k];
    for (int64_t w = lane; w < n; w += 64) {
        const int64_t row = mo + w;
        int32_t *vw = views + row * n_cams;
        uint32_t mask = seeded_views(vw, co_s, n_cams), dropped = 0u;
        double cx[MVM_MAX_CAMS], cy[MVM_MAX_CAMS];
        gather_centroids(pts, co_s, vw, mask & ~7u, cx, cy);     // the seeds are never candidates
        if (mask != 7u) {
            double X0 = X[3 * row], X1 = X[3 * row + 1], X2 = X[3 * row + 2];
            for (int pass = 0; pass < n_ext; ++pass) {
                // the worst candidate: NaN above every number, then the largest
                // residual, ties to the lowest camera (ascending slots, strict >)
                int worst = -1;
                double worst_r = 0.0;
                bool worst_nan = false;
#pragma unroll
                for (int e = 0; e < kPruneSlots; ++e) {
                    if ((mask >> (3 + e)) & 1u) {
                        const double r = reproj_residual(P + 12 * e, X0, X1, X2, cx[3 + e], cy[3 + e]);
                        if (!(r <= gate)) {
                            const bool r_nan = r != r;
                            if (worst < 0 || (!worst_nan && (r_nan || r > worst_r))) {
                                worst = 3 + e;
                                worst_r = r;
                                worst_nan = r_nan;
                            }
                        }
                    }
                }
                if (worst < 0) break;
                mask &= ~(1u << worst);
                dropped |= 1u << worst;
                vw[worst] = -1;
                ext_cost[row * n_ext + (worst - 3)] = INFINITY;
                double out[3];
                mask_dlt<3, 7>(proj_s, pts, co_s, vw, mask, out);     // V = 8 cannot follow a drop
                X0 = out[0], X1 = out[1], X2 = out[2];
            }
            if (dropped) {
                X[3 * row] = X0;
                X[3 * row + 1] = X1;
                X[3 * row + 2] = X2;
            }
        }
        pruned[row] = (int32_t)dropped;
    }
}

// --------------------------------------------- point refinement ----
// mvm_refine_points: per match, a damped Gauss-Newton descent
// of the summed squared reprojection error from the DLT point, and the inverse
// of the normal matrix at the result.  One wave per capture (wave_item), so
// the capture's P is read through uniform addresses.  The kept set is the bit
// mask of kept_views and the view loop runs over compile-time camera slots
// under the mask's bit, so no register array is indexed by a runtime value.
// Every product, sum, division and square root is rounded on its own (this
// file's fp contract(off)), in the order of tests/refine_model.py, whose bits
// the kernel returns.  The 3 x 3 factorisation (refine_ldlt, refine_finite) is
// mvm_refine.h's, shared with the box fit (mvm_boxfit.hip).
struct RefineSums {
    double cost, A[6], g[3];     // A: A00 A01 A02 A11 A12 A22
};

// cost, A and g at X over the views of `mask`, ascending
__device__ __forceinline__ void refine_sums(const double *proj_s, uint32_t mask,
                                            const double (&cx)[MVM_MAX_CAMS],
                                            const double (&cy)[MVM_MAX_CAMS], double X0, double X1,
                                            double X2, RefineSums &e) {
    e.cost = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) e.A[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) e.g[q] = 0.0;
#pragma unroll
    for (int c = 0; c < MVM_MAX_CAMS; ++c) {
        if ((mask >> c) & 1u) {
            const double *p = proj_s + 12 * c;
            const Homog h = project(p, X0, X1, X2);
            const double h2 = h.h2, u = h.h0 / h2, v = h.h1 / h2;
            const double ru = u - cx[c], rv = v - cy[c];
            e.cost = e.cost + (ru * ru + rv * rv);
            const double a0 = (p[0] - u * p[8]) / h2, a1 = (p[1] - u * p[9]) / h2,
                         a2 = (p[2] - u * p[10]) / h2;
            const double b0 = (p[4] - v * p[8]) / h2, b1 = (p[5] - v * p[9]) / h2,
                         b2 = (p[6] - v * p[10]) / h2;
            e.A[0] = e.A[0] + (a0 * a0 + b0 * b0);
            e.A[1] = e.A[1] + (a0 * a1 + b0 * b1);
            e.A[2] = e.A[2] + (a0 * a2 + b0 * b2);
            e.A[3] = e.A[3] + (a1 * a1 + b1 * b1);
            e.A[4] = e.A[4] + (a1 * a2 + b1 * b2);
            e.A[5] = e.A[5] + (a2 * a2 + b2 * b2);
            e.g[0] = e.g[0] + (a0 * ru + b0 * rv);
            e.g[1] = e.g[1] + (a1 * ru + b1 * rv);
            e.g[2] = e.g[2] + (a2 * ru + b2 * rv);
        }
    }
}

__global__ __launch_bounds__(kCompactThreads) void refine_points_kernel(
    const int64_t *__restrict__ match_offs, const int32_t *__restrict__ count,
    const double *__restrict__ pts, const int64_t *__restrict__ cam_offs,
    const double *__restrict__ proj, const int32_t *__restrict__ views, const double *__restrict__ X,
    int32_t n_scenes, int32_t n_cams, int32_t max_evals, double *__restrict__ X_out,
    double *__restrict__ rms, int32_t *__restrict__ info, double *__restrict__ cov) {
    int lane;
    const int64_t s = wave_item(n_scenes, lane);
    if (s < 0) return;
    const auto [mo, n] = match_range(match_offs, count, s);
    const int64_t *co_s = cam_offs + s * n_cams;
    const double *proj_s = proj + s * n_cams * 12;
    const double qnan = __builtin_nan("");
    for (int64_t w = lane; w < n; w += 64) {
        const int64_t row = mo + w;
        const double Xi0 = X[3 * row], Xi1 = X[3 * row + 1], Xi2 = X[3 * row + 2];
        // an entry that is no detection of its view skips the row (status 3)
        bool ok;
        const uint32_t mask = kept_views(views + row * n_cams, co_s, n_cams, ok);
        double cx[MVM_MAX_CAMS], cy[MVM_MAX_CAMS];
        gather_centroids(pts, co_s, views + row * n_cams, mask, cx, cy);
        const int kept = __builtin_popcount(mask);
        double X0 = Xi0, X1 = Xi1, X2 = Xi2, rms0 = qnan, rms1 = qnan;
        int32_t status = 3, evals = 0;
        RefineSums cur;
        if (ok && kept >= 2) {
            refine_sums(proj_s, mask, cx, cy, X0, X1, X2, cur);
            const double cost0 = cur.cost;
            double A_in[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) A_in[q] = cur.A[q];
            double cost = cost0, lam = 1e-3;
            bool sums_ok = refine_finite(cost);
#pragma unroll
            for (int q = 0; q < 6; ++q) sums_ok &= refine_finite(cur.A[q]);
#pragma unroll
            for (int q = 0; q < 3; ++q) sums_ok &= refine_finite(cur.g[q]);
            status = sums_ok ? -1 : 2;
            while (status < 0) {
                RefineLdlt f;
                const bool pivots = refine_ldlt(cur.A[0] + lam * cur.A[0], cur.A[1], cur.A[2],
                                                cur.A[3] + lam * cur.A[3], cur.A[4],
                                                cur.A[5] + lam * cur.A[5], f);
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
                if ((e0 * e0 + e1 * e1) + e2 * e2 <= 1e-20 * ((X0 * X0 + X1 * X1) + X2 * X2)) {
                    status = 0;
                    break;
                }
                if (evals == max_evals) {
                    status = 1;
                    break;
                }
                ++evals;
                const double Y0 = X0 + e0, Y1 = X1 + e1, Y2 = X2 + e2;
                RefineSums tr;
                refine_sums(proj_s, mask, cx, cy, Y0, Y1, Y2, tr);
                if (tr.cost < cost) {                // a NaN fails this
                    X0 = Y0, X1 = Y1, X2 = Y2;
                    cost = tr.cost;
                    cur = tr;
                    lam = fmax(lam / 10.0, 1e-15);
                    bool finite = true;
#pragma unroll
                    for (int q = 0; q < 6; ++q) finite &= refine_finite(cur.A[q]);
#pragma unroll
                    for (int q = 0; q < 3; ++q) finite &= refine_finite(cur.g[q]);
                    if (!finite) status = 2;
                } else {
                    lam = lam * 10.0;
                }
            }
            if (status == 2) {                       // the input stands
                X0 = Xi0, X1 = Xi1, X2 = Xi2;
                cost = cost0;
#pragma unroll
                for (int q = 0; q < 6; ++q) cur.A[q] = A_in[q];
            }
            const double k = (double)kept;
            rms0 = sqrt(cost0 / k);
            rms1 = sqrt(cost / k);
        }
        X_out[3 * row] = X0;
        X_out[3 * row + 1] = X1;
        X_out[3 * row + 2] = X2;
        rms[2 * row] = rms0;
        rms[2 * row + 1] = rms1;
        info[2 * row] = status;
        info[2 * row + 1] = evals;
        if (cov != nullptr) {
            double c00 = qnan, c01 = qnan, c02 = qnan, c11 = qnan, c12 = qnan, c22 = qnan;
            if (status != 3) {
                // A^-1 = L^-T D^-1 L^-1 of the undamped A at X_out
                RefineLdlt f;
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

// ------------------------------------------------- rig matrices ----
// compute_fundamental_matrix (camera_utils.py:23-46) for every (capture, pair)
// and P = K @ RT[:3] (process_pose.py:91) for every (capture, camera): one
// work item each over a flat index, no LDS, no barrier.  The arithmetic is the
// host function's, dtype by dtype, every dot product in index order.  As in
// mvm_device.h, FMAs stand exactly where numpy / OpenBLAS placed them in the
// reference run and nowhere else (this file's `#pragma clang fp contract(off)`
// and the build's -ffp-contract=off): the fp64 3x3 products of F go through
// OpenBLAS's FMA kernels, a0 * b0 then one fma per further term (dot3_fma: the
// reference's own F of tests/golden/a6_fundamental.npz bit for bit); the
// float32 inverse and P = K @ RT[:3] (numpy's own loop) are un-fused (dot3).
constexpr int kRigThreads = 256;

struct RigPairs {
    int32_t a[MVM_MAX_PAIRS];
    int32_t b[MVM_MAX_PAIRS];
};

__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2,
                                       double b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

__device__ __forceinline__ double dot3_fma(double a0, double b0, double a1, double b1, double a2,
                                           double b2) {
    return __builtin_fma(a2, b2, __builtin_fma(a1, b1, a0 * b0));
}

// the K the kernel inverts: upper triangular without skew, K[2][2] == 1
__device__ __forceinline__ bool pinhole_k(const float *K) {
    return K[3] == 0.0f && K[6] == 0.0f && K[7] == 0.0f && K[1] == 0.0f && K[8] == 1.0f &&
           K[0] != 0.0f && K[4] != 0.0f;
}

// float32 inverse of a pinhole K, column by column by back substitution,
// x[r] = (b[r] - sum_{q > r} K[r][q] * x[q]) / K[r][r]: the bits of
// np.linalg.inv (:38-39) for such K.  Promoted to fp64 as the product does.
__device__ __forceinline__ void pinhole_inverse(const float *K, double inv[9]) {
    float k[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) k[q] = K[q];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x[3];
#pragma unroll
        for (int r = 2; r >= 0; --r) {
            float acc = (r == c) ? 1.0f : 0.0f;
#pragma unroll
            for (int q = r + 1; q < 3; ++q) acc = acc - k[3 * r + q] * x[q];
            x[r] = acc / k[3 * r + r];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) inv[3 * r + c] = (double)x[r];
    }
}

__device__ __forceinline__ void rig_fundamental(const float *K1, const double *RT1, const float *K2,
                                                const double *RT2, double *F) {
    double R1[9], R2[9], t1[3], t2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R1[3 * i + j] = RT1[4 * i + j];
            R2[3 * i + j] = RT2[4 * i + j];
        }
        t1[i] = RT1[4 * i + 3];
        t2[i] = RT2[4 * i + 3];
    }
    double R[9], t[3];                       // R_rel = R2 R1^T (:27), t_rel = t2 - R_rel t1 (:28)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = dot3_fma(R2[3 * i], R1[3 * j], R2[3 * i + 1], R1[3 * j + 1], R2[3 * i + 2],
                                R1[3 * j + 2]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        t[i] = t2[i] - dot3_fma(R[3 * i], t1[0], R[3 * i + 1], t1[1], R[3 * i + 2], t1[2]);
    // the skew matrix is float32 (:31-35) and promoted by the product (:37)
    const double tx = (double)(float)t[0], ty = (double)(float)t[1], tz = (double)(float)t[2];
    const double sk[9] = {0.0, -tz, ty, tz, 0.0, -tx, -ty, tx, 0.0};
    double E[9], K1i[9], K2i[9], M[9], f[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            E[3 * i + j] = dot3_fma(sk[3 * i], R[j], sk[3 * i + 1], R[3 + j], sk[3 * i + 2], R[6 + j]);
    pinhole_inverse(K1, K1i);
    pinhole_inverse(K2, K2i);
#pragma unroll
    for (int i = 0; i < 3; ++i)              // (K2inv^T E) K1inv, left to right (:40)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            M[3 * i + j] = dot3_fma(K2i[i], E[j], K2i[3 + i], E[3 + j], K2i[6 + i], E[6 + j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            f[3 * i + j] = dot3_fma(M[3 * i], K1i[j], M[3 * i + 1], K1i[3 + j], M[3 * i + 2], K1i[6 + j]);
    const double f22 = f[8];
    const bool norm = fabs(f22) > 1e-8;      // :43-44
#pragma unroll
    for (int q = 0; q < 9; ++q) F[q] = norm ? f[q] / f22 : f[q];
}

__global__ __launch_bounds__(kRigThreads) void rig_matrices_kernel(
    const float *__restrict__ K, const double *__restrict__ RT, RigPairs pairs, int64_t n_items,
    int32_t n_cams, int32_t n_pairs, int32_t per_scene, double *__restrict__ F,
    double *__restrict__ proj, int32_t *__restrict__ status) {
    const int64_t idx = (int64_t)blockIdx.x * kRigThreads + threadIdx.x;
    if (idx >= n_items) return;
    const int64_t s = idx / per_scene;
    const int w = (int)(idx - s * per_scene);
    const float *Ks = K + s * n_cams * 9;
    const double *RTs = RT + s * n_cams * 16;
    // every item of the capture reads all its K's, so they agree on the status
    bool ok = true;
    for (int c = 0; c < n_cams; ++c) ok &= pinhole_k(Ks + 9 * c);
    if (w == 0) status[s] = ok ? 0 : 1;
    if (!ok) return;                         // the caller fills this capture's rows
    if (w < n_pairs) {
        const int a = pairs.a[w], b = pairs.b[w];
        rig_fundamental(Ks + 9 * a, RTs + 16 * a, Ks + 9 * b, RTs + 16 * b,
                        F + (s * n_pairs + w) * 9);
    } else {
        const int c = w - n_pairs;           // P = K @ RT[:3]: float32 K promoted (process_pose.py:91)
        const float *k = Ks + 9 * c;
        const double *rt = RTs + 16 * c;
        double *P = proj + (s * n_cams + c) * 12;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                P[4 * i + j] = dot3((double)k[3 * i], rt[j], (double)k[3 * i + 1], rt[4 + j],
                                    (double)k[3 * i + 2], rt[8 + j]);
    }
}

// ------------------------------------------------- leftovers ----
// The sub-batch of an extra seed pass: the detections no match
// of an earlier pass holds, per view in ascending index order, with the
// cameras reordered so that the pass's seed triple comes first.  `order`
// packs that camera order pi, four bits a slot: slot q reads camera
// (order >> 4 q) & 15.

constexpr int kMarkThreads = 256;

__device__ __forceinline__ int order_cam(uint32_t order, int q) { return (int)(order >> (4 * q) & 15u); }

// One thread per (match row, slot): used[cam_offs[s C + pi[q]] + l] = 1 for the
// row's detection l of slot q.  The row's capture is found by bisection of
// match_offs; rows at and beyond count[s] mark nothing.  With sub_offs / orig
// (a later pass) l indexes the pass's own view and orig maps it to the
// original one.  Every index is range-checked against its view (and the flag
// array) before it is used.  Plain vector stores of the same value: threads
// that meet on a flag write what is already being written.
__global__ __launch_bounds__(kMarkThreads) void mark_used_kernel(
    const int32_t *__restrict__ views, const int64_t *__restrict__ match_offs,
    const int32_t *__restrict__ count, const int64_t *__restrict__ sub_offs,
    const int32_t *__restrict__ orig, const int64_t *__restrict__ cam_offs, int64_t n_rows,
    int32_t n_scenes, int32_t n_cams, uint32_t order, int64_t n_det, int32_t *__restrict__ used) {
    const int64_t t = (int64_t)blockIdx.x * kMarkThreads + threadIdx.x;
    const int64_t row = t / n_cams;
    const int q = (int)(t - row * n_cams);
    if (row >= n_rows || row < match_offs[0]) return;
    int32_t lo = 0, hi = n_scenes;          // match_offs[lo] <= row, the last such capture
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (match_offs[mid] <= row)
            lo = mid;
        else
            hi = mid;
    }
    const int64_t s = lo;
    const int64_t w = row - match_offs[s];
    if (w >= min<int64_t>(count[s], match_offs[s + 1] - match_offs[s])) return;
    int64_t v = views[row * n_cams + q];
    if (sub_offs) {
        const int64_t so = sub_offs[s * n_cams + q];
        if (v < 0 || v >= sub_offs[s * n_cams + q + 1] - so) return;
        v = orig[so + v];
    }
    const int c = order_cam(order, q);
    const int64_t o = cam_offs[s * n_cams + c];
    if (v < 0 || v >= cam_offs[s * n_cams + c + 1] - o) return;
    const int64_t k = o + v;
    if (k < 0 || k >= n_det) return;
    used[k] = 1;
}

// One wave per (capture, slot) (wave_item): the leftovers of camera pi[q],
// counted by ballot + popcount over 64-detection chunks -- the walk of
// leftover_gather_kernel, so the two agree on every view by construction.
__global__ __launch_bounds__(kCompactThreads) void leftover_count_kernel(
    const int32_t *__restrict__ used, const int64_t *__restrict__ cam_offs, int64_t n_views,
    int32_t n_cams, uint32_t order, int32_t *__restrict__ counts) {
    int lane;
    const int64_t sq = wave_item(n_views, lane);
    if (sq < 0) return;
    const int64_t s = sq / n_cams;
    const int c = order_cam(order, (int)(sq - s * n_cams));
    const int64_t b = cam_offs[s * n_cams + c], e = cam_offs[s * n_cams + c + 1];
    int32_t n = 0;
    for (int64_t k0 = b; k0 < e; k0 += 64) {
        const int64_t k = k0 + lane;
        n += __builtin_popcountll(__ballot(k < e && used[k] == 0));
    }
    if (lane == 0) counts[sq] = n;
}

// The same wave per (capture, slot): leftover l of the chunk goes to row
// sub_offs[s C + q] + base + (leftovers of the chunk in lower lanes), `base`
// the scalar count of the chunks before -- input order is kept.  A row is a
// detection (load / store_detection<VEC>) and its index in its original
// view.  Never more rows than sub_offs leaves the view.
template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void leftover_gather_kernel(
    const int32_t *__restrict__ used, const double *__restrict__ pts,
    const int32_t *__restrict__ boxes, const int64_t *__restrict__ cam_offs,
    const int64_t *__restrict__ sub_offs, int64_t n_views, int32_t n_cams, uint32_t order,
    double *__restrict__ pts_out, int32_t *__restrict__ boxes_out, int32_t *__restrict__ orig_out) {
    int lane;
    const int64_t sq = wave_item(n_views, lane);
    if (sq < 0) return;
    const int64_t s = sq / n_cams;
    const int c = order_cam(order, (int)(sq - s * n_cams));
    const int64_t b = cam_offs[s * n_cams + c], e = cam_offs[s * n_cams + c + 1];
    const int64_t dst = sub_offs[sq], room = sub_offs[sq + 1] - dst;
    int64_t base = 0;
    for (int64_t k0 = b; k0 < e; k0 += 64) {
        const int64_t k = k0 + lane;
        const bool keep = k < e && used[k] == 0;
        const uint64_t m = __ballot(keep);
        const int64_t pos = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (keep && pos < room) {
            const int64_t r = dst + pos;
            store_detection<VEC>(boxes_out, pts_out, r, load_detection<VEC>(boxes, pts, k));
            orig_out[r] = (int32_t)(k - b);
        }
        base += __builtin_popcountll(m);
    }
}

// ---- host: launch helpers -------------------------------------------------------
// every pointer on a 16-byte boundary (what the VEC kernels' 16-byte accesses need)
template <typename... T>
bool aligned16(const T *...p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// What an entry point over a batch of captures opens with.  false: `st` is its
// return value -- the refusal of a negative n_scenes, or MVM_OK for no capture.
bool some_captures(int32_t n_scenes, int &st) {
    mvm_clear_error();
    st = n_scenes < 0 ? mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative n_scenes") : MVM_OK;
    return n_scenes > 0;
}

// MVM_OK, or the refusal of n_cams outside [lo, MVM_MAX_CAMS]
int cams_within(int32_t n_cams, int32_t lo) {
    if (n_cams < lo || n_cams > MVM_MAX_CAMS)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_cams=%d outside [%d, %d]", n_cams, lo, MVM_MAX_CAMS);
    return MVM_OK;
}

// workgroups of a wave-per-item launch (wave_item)
int64_t wave_grid(int64_t n_items) { return (n_items + kCompactScenes - 1) / kCompactScenes; }

// The camera order of a seed pass, packed as the leftover kernels read it:
// (a, b, c), then the other cameras ascending.  MVM_OK, or the refusal of
// n_cams outside 4..MVM_MAX_CAMS or of a triple that is not three distinct
// cameras < n_cams.
int leftover_order(int32_t n_cams, int32_t a, int32_t b, int32_t c, uint32_t &order) {
    if (const int st = cams_within(n_cams, 4)) return st;
    const int32_t seed[3] = {a, b, c};
    for (int k = 0; k < 3; ++k)
        if (seed[k] < 0 || seed[k] >= n_cams)
            return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "seed (%d, %d, %d): camera %d outside [0, %d)", a, b,
                            c, seed[k], n_cams);
    if (a == b || a == c || b == c)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "seed (%d, %d, %d): a camera is repeated", a, b, c);
    order = (uint32_t)a | (uint32_t)b << 4 | (uint32_t)c << 8;
    int q = 3;
    for (int32_t d = 0; d < n_cams; ++d)
        if (d != a && d != b && d != c) order |= (uint32_t)d << (4 * q++);
    return MVM_OK;
}

// workgroups of a wave per (capture, slot) launch: MVM_OK, or the refusal beyond one launch
int leftover_grid(int32_t n_scenes, int32_t n_cams, unsigned &grid) {
    const int64_t g = wave_grid((int64_t)n_scenes * n_cams);
    grid = (unsigned)g;
    if (g > kMaxGridBlocks)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_scenes=%d: more views than one launch holds; split them",
                        n_scenes);
    return MVM_OK;
}

}  // namespace

extern "C" {

int mvm_rig_matrices(const float *K_dev, const double *RT_dev, const int32_t *pair_a,
                     const int32_t *pair_b, int32_t n_scenes, int32_t n_cams, int32_t n_pairs,
                     double *F_dev, double *proj_dev, int32_t *status_dev, mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    if ((rc = cams_within(n_cams, 2))) return rc;
    if (n_pairs < 1 || n_pairs > MVM_MAX_PAIRS)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_pairs=%d outside [1, %d]", n_pairs, MVM_MAX_PAIRS);
    if (const int st = mvm_require_ptrs({{K_dev, "K_dev"},   {RT_dev, "RT_dev"}, {pair_a, "pair_a"},
                                         {pair_b, "pair_b"}, {F_dev, "F_dev"},   {status_dev, "status_dev"}}))
        return st;
    RigPairs pairs{};
    for (int p = 0; p < n_pairs; ++p) {
        if (pair_a[p] < 0 || pair_a[p] >= n_cams || pair_b[p] < 0 || pair_b[p] >= n_cams ||
            pair_a[p] == pair_b[p])
            return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "pair %d = (%d, %d) invalid for %d cameras", p,
                            pair_a[p], pair_b[p], n_cams);
        pairs.a[p] = pair_a[p];
        pairs.b[p] = pair_b[p];
    }
    const int32_t per_scene = n_pairs + (proj_dev ? n_cams : 0);
    const int64_t n_items = (int64_t)n_scenes * per_scene;
    const int64_t grid = (n_items + kRigThreads - 1) / kRigThreads;
    if (grid > kMaxGridBlocks)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_scenes=%d: more work items than one launch holds",
                        n_scenes);
    rig_matrices_kernel<<<(unsigned)grid, kRigThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        K_dev, RT_dev, pairs, n_items, n_cams, n_pairs, per_scene, F_dev, proj_dev, status_dev);
    return mvm_check_launch("rig_matrices_kernel");
}

int mvm_compact_matches(const int32_t *match_dev, const float *cost_dev, const double *X_dev,
                        const int32_t *count_dev, const int64_t *seg_offs_dev, const double *pts_dev,
                        const int32_t *boxes_dev, const int64_t *cam_offs_dev, int32_t n_scenes,
                        int32_t scene_base, int64_t *dense_offs_dev, int32_t *scene_out_dev,
                        int32_t *match_out_dev, float *cost_out_dev, double *X_out_dev,
                        int32_t *boxes_out_dev, double *cent_out_dev, mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    if (const int st = mvm_require_ptrs({{match_dev, "match_dev"},         {cost_dev, "cost_dev"},
                                         {X_dev, "X_dev"},                 {count_dev, "count_dev"},
                                         {seg_offs_dev, "seg_offs_dev"},   {pts_dev, "pts_dev"},
                                         {boxes_dev, "boxes_dev"},         {cam_offs_dev, "cam_offs_dev"},
                                         {dense_offs_dev, "dense_offs_dev"}, {scene_out_dev, "scene_out_dev"},
                                         {match_out_dev, "match_out_dev"}, {cost_out_dev, "cost_out_dev"},
                                         {X_out_dev, "X_out_dev"},         {boxes_out_dev, "boxes_out_dev"},
                                         {cent_out_dev, "cent_out_dev"}}))
        return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    pack_scan_kernel<<<1, 1024, 0, s>>>(count_dev, n_scenes, dense_offs_dev);
    const int grid = (int)wave_grid(n_scenes);
    dispatch_bool(aligned16(pts_dev, boxes_dev, boxes_out_dev, cent_out_dev), [&](auto vec) {
        compact_matches_kernel<decltype(vec)::value><<<grid, kCompactThreads, 0, s>>>(
            match_dev, cost_dev, X_dev, count_dev, seg_offs_dev, dense_offs_dev, pts_dev, boxes_dev,
            cam_offs_dev, n_scenes, scene_base, scene_out_dev, match_out_dev, cost_out_dev, X_out_dev,
            boxes_out_dev, cent_out_dev);
    });
    return mvm_check_launch("compact_matches_kernel");
}

int mvm_compact_matches_views(const int32_t *views_dev, const float *cost_dev,
                              const float *ext_cost_dev, const double *X_dev, const int32_t *count_dev,
                              const int64_t *seg_offs_dev, const double *pts_dev,
                              const int32_t *boxes_dev, const int64_t *cam_offs_dev,
                              const double *proj_dev, int32_t n_scenes, int32_t n_cams,
                              int32_t scene_base, int64_t *dense_offs_dev, int32_t *scene_out_dev,
                              int32_t *views_out_dev, int32_t *n_views_out_dev, float *cost_out_dev,
                              float *ext_cost_out_dev, double *X_out_dev, int32_t *boxes_out_dev,
                              double *cent_out_dev, double *reproj_out_dev, mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    if ((rc = cams_within(n_cams, 3))) return rc;
    const bool ext = n_cams > 3;         // no extra view: the [cap, 0] arrays may be NULL
    if (const int st = mvm_require_ptrs({{views_dev, "views_dev"},
                                         {cost_dev, "cost_dev"},
                                         {ext ? (const void *)ext_cost_dev : views_dev, "ext_cost_dev"},
                                         {X_dev, "X_dev"},
                                         {count_dev, "count_dev"},
                                         {seg_offs_dev, "seg_offs_dev"},
                                         {pts_dev, "pts_dev"},
                                         {boxes_dev, "boxes_dev"},
                                         {cam_offs_dev, "cam_offs_dev"},
                                         {proj_dev, "proj_dev"},
                                         {dense_offs_dev, "dense_offs_dev"},
                                         {scene_out_dev, "scene_out_dev"},
                                         {views_out_dev, "views_out_dev"},
                                         {n_views_out_dev, "n_views_out_dev"},
                                         {cost_out_dev, "cost_out_dev"},
                                         {ext ? (const void *)ext_cost_out_dev : views_dev, "ext_cost_out_dev"},
                                         {X_out_dev, "X_out_dev"},
                                         {boxes_out_dev, "boxes_out_dev"},
                                         {cent_out_dev, "cent_out_dev"},
                                         {reproj_out_dev, "reproj_out_dev"}}))
        return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    pack_scan_kernel<<<1, 1024, 0, s>>>(count_dev, n_scenes, dense_offs_dev);
    const int grid = (int)wave_grid(n_scenes);
    dispatch_bool(aligned16(pts_dev, boxes_dev, boxes_out_dev, cent_out_dev), [&](auto vec) {
        compact_matches_views_kernel<decltype(vec)::value><<<grid, kCompactThreads, 0, s>>>(
            views_dev, cost_dev, ext_cost_dev, X_dev, count_dev, seg_offs_dev, dense_offs_dev, pts_dev,
            boxes_dev, cam_offs_dev, proj_dev, n_scenes, n_cams, scene_base, scene_out_dev,
            views_out_dev, n_views_out_dev, cost_out_dev, ext_cost_out_dev, X_out_dev, boxes_out_dev,
            cent_out_dev, reproj_out_dev);
    });
    return mvm_check_launch("compact_matches_views_kernel");
}

int mvm_prune_views_triangulate(const int64_t *match_offs_dev, const int32_t *count_dev,
                                int32_t n_scenes, int32_t n_cams, const double *pts_dev,
                                const int64_t *cam_offs_dev, const double *proj_dev, double gate,
                                int32_t *views_dev, float *ext_cost_dev, double *X_dev,
                                int32_t *pruned_dev, mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    if ((rc = cams_within(n_cams, 4))) return rc;
    if (!(gate >= 0.0))                  // NaN included
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "gate=%g: a number >= 0 (or +inf) required", gate);
    if (const int st = mvm_require_ptrs({{match_offs_dev, "match_offs_dev"}, {count_dev, "count_dev"},
                                         {pts_dev, "pts_dev"},               {cam_offs_dev, "cam_offs_dev"},
                                         {proj_dev, "proj_dev"},             {views_dev, "views_dev"},
                                         {ext_cost_dev, "ext_cost_dev"},     {X_dev, "X_dev"},
                                         {pruned_dev, "pruned_dev"}}))
        return st;
    const int grid = (int)wave_grid(n_scenes);
    prune_views_kernel<<<grid, kCompactThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        match_offs_dev, count_dev, pts_dev, cam_offs_dev, proj_dev, gate, n_scenes, n_cams, views_dev,
        ext_cost_dev, X_dev, pruned_dev);
    return mvm_check_launch("prune_views_kernel");
}

int mvm_refine_points(const int64_t *match_offs_dev, const int32_t *count_dev, int32_t n_scenes,
                      int32_t n_cams, const double *pts_dev, const int64_t *cam_offs_dev,
                      const double *proj_dev, const int32_t *views_dev, const double *X_dev,
                      int32_t max_evals, double *X_out_dev, double *rms_dev, int32_t *info_dev,
                      double *cov_dev, mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    if ((rc = cams_within(n_cams, 3))) return rc;
    if (max_evals < 1 || max_evals > 64)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "max_evals=%d outside [1, 64]", max_evals);
    if (const int st = mvm_require_ptrs({{match_offs_dev, "match_offs_dev"}, {count_dev, "count_dev"},
                                         {pts_dev, "pts_dev"},               {cam_offs_dev, "cam_offs_dev"},
                                         {proj_dev, "proj_dev"},             {views_dev, "views_dev"},
                                         {X_dev, "X_dev"},                   {X_out_dev, "X_out_dev"},
                                         {rms_dev, "rms_dev"},               {info_dev, "info_dev"}}))
        return st;                       // cov_dev may be NULL: no covariance is written
    const int grid = (int)wave_grid(n_scenes);
    refine_points_kernel<<<grid, kCompactThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        match_offs_dev, count_dev, pts_dev, cam_offs_dev, proj_dev, views_dev, X_dev, n_scenes, n_cams,
        max_evals, X_out_dev, rms_dev, info_dev, cov_dev);
    return mvm_check_launch("refine_points_kernel");
}

int mvm_mark_used(const int32_t *views_dev, const int64_t *match_offs_dev, const int32_t *count_dev,
                  int64_t n_rows, int32_t n_scenes, int32_t n_cams, int32_t seed_a, int32_t seed_b,
                  int32_t seed_c, const int64_t *sub_cam_offs_dev, const int32_t *orig_dev,
                  const int64_t *cam_offs_dev, int64_t n_det, int32_t *used_dev, mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    if (n_rows < 0 || n_det < 0) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative n_rows or n_det");
    uint32_t order = 0;
    if (const int st = leftover_order(n_cams, seed_a, seed_b, seed_c, order)) return st;
    if ((sub_cam_offs_dev == nullptr) != (orig_dev == nullptr))
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "sub_cam_offs_dev and orig_dev go together");
    if (n_rows == 0 || n_det == 0) return MVM_OK;
    if (const int st = mvm_require_ptrs({{views_dev, "views_dev"},
                                         {match_offs_dev, "match_offs_dev"},
                                         {count_dev, "count_dev"},
                                         {cam_offs_dev, "cam_offs_dev"},
                                         {used_dev, "used_dev"}}))
        return st;
    const int64_t grid = (n_rows * n_cams + kMarkThreads - 1) / kMarkThreads;
    if (grid > kMaxGridBlocks)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_rows=%lld: more rows than one launch holds; split them",
                        (long long)n_rows);
    mark_used_kernel<<<(unsigned)grid, kMarkThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        views_dev, match_offs_dev, count_dev, sub_cam_offs_dev, orig_dev, cam_offs_dev, n_rows, n_scenes,
        n_cams, order, n_det, used_dev);
    return mvm_check_launch("mark_used_kernel");
}

int mvm_leftover_counts(const int32_t *used_dev, const int64_t *cam_offs_dev, int32_t n_scenes,
                        int32_t n_cams, int32_t seed_a, int32_t seed_b, int32_t seed_c,
                        int32_t *counts_dev, mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    uint32_t order = 0;
    if (const int st = leftover_order(n_cams, seed_a, seed_b, seed_c, order)) return st;
    if (const int st = mvm_require_ptrs(
            {{used_dev, "used_dev"}, {cam_offs_dev, "cam_offs_dev"}, {counts_dev, "counts_dev"}}))
        return st;
    unsigned grid;
    if ((rc = leftover_grid(n_scenes, n_cams, grid))) return rc;
    leftover_count_kernel<<<grid, kCompactThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        used_dev, cam_offs_dev, (int64_t)n_scenes * n_cams, n_cams, order, counts_dev);
    return mvm_check_launch("leftover_count_kernel");
}

int mvm_leftover_gather(const int32_t *used_dev, const double *pts_dev, const int32_t *boxes_dev,
                        const int64_t *cam_offs_dev, const int64_t *sub_cam_offs_dev, int32_t n_scenes,
                        int32_t n_cams, int32_t seed_a, int32_t seed_b, int32_t seed_c,
                        double *pts_out_dev, int32_t *boxes_out_dev, int32_t *orig_out_dev,
                        mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    uint32_t order = 0;
    if (const int st = leftover_order(n_cams, seed_a, seed_b, seed_c, order)) return st;
    if (const int st = mvm_require_ptrs({{used_dev, "used_dev"},
                                         {pts_dev, "pts_dev"},
                                         {boxes_dev, "boxes_dev"},
                                         {cam_offs_dev, "cam_offs_dev"},
                                         {sub_cam_offs_dev, "sub_cam_offs_dev"},
                                         {pts_out_dev, "pts_out_dev"},
                                         {boxes_out_dev, "boxes_out_dev"},
                                         {orig_out_dev, "orig_out_dev"}}))
        return st;
    unsigned grid;
    if ((rc = leftover_grid(n_scenes, n_cams, grid))) return rc;
    dispatch_bool(aligned16(pts_dev, boxes_dev, pts_out_dev, boxes_out_dev), [&](auto vec) {
        leftover_gather_kernel<decltype(vec)::value>
            <<<grid, kCompactThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
                used_dev, pts_dev, boxes_dev, cam_offs_dev, sub_cam_offs_dev, (int64_t)n_scenes * n_cams,
                n_cams, order, pts_out_dev, boxes_out_dev, orig_out_dev);
    });
    return mvm_check_launch("leftover_gather_kernel");
}

int mvm_pack_detections(const float *boxes_dev, const float *conf_dev, const float *cls_dev,
                        const int64_t *img_offs_dev, int32_t n_img, float conf_thresh,
                        float class_id, int32_t *counts_dev, int64_t *cam_offs_dev,
                        double *pts_dev, int32_t *boxes_out_dev, int32_t *status_dev,
                        mvm_stream_t stream) {
    mvm_clear_error();
    if (n_img < 0) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative n_img");
    if (n_img == 0) return MVM_OK;
    // the row arrays may be NULL when every image is empty
    if (!img_offs_dev || !counts_dev || !cam_offs_dev || !status_dev)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "null pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(status_dev, 0, sizeof(int32_t), s) != hipSuccess)
        return mvm_fail(MVM_ERR_HIP, "hipMemsetAsync(status) failed");
    pack_count_kernel<<<n_img, kPackThreads, 0, s>>>(conf_dev, cls_dev, img_offs_dev, conf_thresh,
                                                     class_id, counts_dev);
    pack_scan_kernel<<<1, 1024, 0, s>>>(counts_dev, n_img, cam_offs_dev);
    pack_write_kernel<<<n_img, kPackThreads, 0, s>>>(boxes_dev, conf_dev, cls_dev, img_offs_dev,
                                                     conf_thresh, class_id, cam_offs_dev, pts_dev,
                                                     boxes_out_dev, status_dev);
    return mvm_check_launch("pack_detections");
}

int mvm_triangulate_dlt(const double *proj_dev, const int32_t *set_of_point_dev,
                        const double *pts2d_dev, int32_t n_points, int32_t n_views, double *X_dev,
                        mvm_stream_t stream) {
    mvm_clear_error();
    if (n_points < 0 || n_views < 2 || n_views > kMaxViews)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "n_points >= 0 and 2 <= n_views <= %d required",
                        kMaxViews);
    if (n_points == 0) return MVM_OK;
    if (!proj_dev || !pts2d_dev || !X_dev) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "null pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dispatch_int<2, 3, 4, 5, 6, 7, 8>(n_views, [&](auto nv) {
        dlt_kernel<decltype(nv)::value><<<(n_points + 255) / 256, 256, 0, s>>>(
            proj_dev, set_of_point_dev, pts2d_dev, n_points, X_dev);
    });
    return mvm_check_launch("dlt_kernel");
}

int mvm_select_triangulate(const float *cube_dev, const int64_t *cube_offs_dev,
                           const int64_t *cam_offs_dev, const int64_t *lsap_out_offs_dev,
                           const int64_t *row_ind_dev, const int64_t *col_ind_dev,
                           const double *pts_dev, const double *proj_dev, int32_t n_scenes,
                           double threshold, int32_t *match_dev, float *cost_dev, double *X_dev,
                           int32_t *count_dev, mvm_stream_t stream) {
    int rc;
    if (!some_captures(n_scenes, rc)) return rc;
    if (!cube_offs_dev || !cam_offs_dev || !lsap_out_offs_dev || !proj_dev || !count_dev)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "null pointer");
    select_triangulate_kernel<<<n_scenes, kSelThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        cube_dev, cube_offs_dev, cam_offs_dev, lsap_out_offs_dev, row_ind_dev, col_ind_dev, pts_dev,
        proj_dev, threshold, match_dev, cost_dev, X_dev, count_dev, nullptr, 0, 0, 0);
    return mvm_check_launch("select_triangulate_kernel");
}

int mvm_extend_select_triangulate(const float *E_dev, const int64_t *ext_offs_dev,
                                  const int64_t *lsap_out_offs_dev, const int64_t *row_ind_dev,
                                  const int64_t *col_ind_dev, const int32_t *match_dev,
                                  const int64_t *match_offs_dev, const int32_t *count_dev,
                                  const double *pts_dev, const int64_t *cam_offs_dev,
                                  const double *proj_dev, int32_t n_scenes, int32_t n_cams,
                                  double threshold, int32_t *views_dev, float *ext_cost_dev,
                                  double *X_dev, mvm_stream_t stream) {
    mvm_clear_error();
    if (n_scenes < 0) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative n_scenes");
    if (const int st = cams_within(n_cams, 3)) return st;      // refused for an empty batch too
    if (n_scenes == 0 || n_cams == 3) return MVM_OK;
    // E / row_ind / col_ind / pts may be NULL when every extra view or every
    // capture is empty (nothing then reads them)
    if (const int st = mvm_require_ptrs({{ext_offs_dev, "ext_offs_dev"}, {lsap_out_offs_dev, "lsap_out_offs_dev"},
                                         {match_dev, "match_dev"},       {match_offs_dev, "match_offs_dev"},
                                         {count_dev, "count_dev"},       {cam_offs_dev, "cam_offs_dev"},
                                         {proj_dev, "proj_dev"},         {views_dev, "views_dev"},
                                         {ext_cost_dev, "ext_cost_dev"}, {X_dev, "X_dev"}}))
        return st;
    extend_select_triangulate_kernel<<<n_scenes, kSelThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        E_dev, ext_offs_dev, lsap_out_offs_dev, row_ind_dev, col_ind_dev, match_dev, match_offs_dev,
        count_dev, pts_dev, cam_offs_dev, proj_dev, threshold, n_cams, views_dev, ext_cost_dev, X_dev);
    return mvm_check_launch("extend_select_triangulate_kernel");
}

int mvm_select_triangulate_resid(const double *resid_dev, int32_t max_n, const int64_t *cam_offs_dev,
                                 const int64_t *lsap_out_offs_dev, const int64_t *row_ind_dev,
                                 const int64_t *col_ind_dev, const double *pts_dev,
                                 const double *proj_dev, int32_t n_scenes, double threshold,
                                 int32_t *match_dev, float *cost_dev, double *X_dev, int32_t *count_dev,
                                 mvm_stream_t stream) {
    mvm_clear_error();
    if (n_scenes < 0 || max_n < 0) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative sizes");
    if (n_scenes == 0) return MVM_OK;
    if (!resid_dev || !cam_offs_dev || !lsap_out_offs_dev || !proj_dev || !count_dev)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "null pointer");
    const int32_t ld = (max_n + 3) / 4 * 4;
    select_triangulate_kernel<<<n_scenes, kSelThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        nullptr, nullptr, cam_offs_dev, lsap_out_offs_dev, row_ind_dev, col_ind_dev, pts_dev, proj_dev,
        threshold, match_dev, cost_dev, X_dev, count_dev, resid_dev, (int64_t)3 * max_n * ld, ld, max_n);
    return mvm_check_launch("select_triangulate_kernel");
}

}  // extern "C"
