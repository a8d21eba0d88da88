// mvm_extend.hip — the extension of three-view matches into the extra cameras
// of a 4..8 camera rig: the cost of giving detection l of extra
// view d to match w,
//   E_d[w][l] = float32(((e_0d(p0[i_w], q_l) + e_1d(p1[j_w], q_l)) + e_2d(p2[k_w], q_l)) / 3)
// with e_cd = epipolar_error under F_cd (epipolar_matching.py:5-28): a cube
// entry (epipolar_matching.py:78-81, :96) whose three anchors are the match's
// own detections.  The (n, n_d) matrices go to the assignment solver as they
// are; mvm_extend_select_triangulate (mvm_pipeline.hip) consumes its result.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "mvmatch.h"
#include "mvm_device.h"
#include "mvm_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int kExtRowsPerWave = 16;
constexpr int kExtRows = kWaves * kExtRowsPerWave;   // rows of one workgroup's tile
constexpr int kExtColTile = 2 * kChunk;              // columns of view d resident in LDS
constexpr int kExtAnchors = 3;                       // cameras 0, 1, 2

// Workgroup = 4 waves owning kExtRows matches of one (capture, extra camera
// d).  The row side (per match and anchor camera c: the anchor's centroid and
// its line F_cd p in view d) is computed once into LDS; the column side (per
// detection q of view d and anchor camera: the line F_cd^T q in view c) once
// per kExtColTile columns.  Per 256-column chunk a lane holds its 4 consecutive
// columns' three lines in registers and walks its wave's 16 rows: one 16-byte
// store per lane per row when rows are 16-byte aligned, element stores
// otherwise.  Every entry takes the generic arithmetic (the 9999 sentinel by
// select, cube_f32's division fallback): the matrices are n x n_d, small next
// to the cube.  The global loads of a tile (F, match, pts) all come before
// its first store.
__global__ __launch_bounds__(kThreads) void extend_cost_kernel(
    const double *__restrict__ pts, const int64_t *__restrict__ cam_offs,
    const double *__restrict__ F, const int32_t *__restrict__ match,
    const int64_t *__restrict__ match_offs, const int32_t *__restrict__ count,
    const int64_t *__restrict__ ext_offs, int32_t n_cams, int32_t row_blocks,
    float *__restrict__ E) {
    __shared__ double s_cl[kExtAnchors][3][kExtColTile];   // column lines l0, l1, l2
    __shared__ double s_cx[kExtColTile], s_cy[kExtColTile];
    __shared__ uint32_t s_cdeg[kExtColTile];               // bit c: line of anchor c degenerate
    __shared__ double s_rl[kExtRows][kExtAnchors][5];      // row line l0, l1, l2 and the anchor x, y
    __shared__ uint32_t s_rdeg[kExtRows][kExtAnchors];

    const int n_ext = n_cams - kExtAnchors;
    const int64_t sd = blockIdx.x / (uint32_t)row_blocks;
    const int rb = (int)(blockIdx.x % (uint32_t)row_blocks);
    const int64_t s = sd / n_ext;
    const int e = (int)(sd - s * n_ext);
    const int64_t *co = cam_offs + s * n_cams;
    const int64_t od = co[kExtAnchors + e];
    const int64_t nd64 = co[kExtAnchors + e + 1] - od;
    if (nd64 <= 0 || nd64 > 0x7FFFFFFF) return;
    const int nd = (int)nd64;
    const int64_t eo = ext_offs[sd];
    // the rows this matrix has room for bound the count (never written past)
    const int64_t room = (ext_offs[sd + 1] - eo) / nd;
    const int64_t mo = match_offs[s];
    const int n = (int)min<int64_t>(min<int64_t>(count[s], room), match_offs[s + 1] - mo);
    const int row0 = rb * kExtRows;
    if (row0 >= n) return;

    double f[kExtAnchors][9];
#pragma unroll
    for (int c = 0; c < kExtAnchors; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) f[c][k] = F[((s * n_ext + e) * kExtAnchors + c) * 9 + k];

    const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
    // row side: thread (row, anchor)
    if (t < kExtRows * kExtAnchors) {
        const int lr = t / kExtAnchors, c = t - lr * kExtAnchors;
        double x = 0, y = 0, l0 = 0, l1 = 0, l2 = 0;
        bool deg = true;
        if (row0 + lr < n) {
            const int64_t idx = match[3 * (mo + row0 + lr) + c];
            // an index outside its view names no detection: a NaN anchor
            x = y = __builtin_nan("");
            if (idx >= 0 && idx < co[c + 1] - co[c]) {
                x = pts[2 * (co[c] + idx)];
                y = pts[2 * (co[c] + idx) + 1];
            }
            // the three F of a thread are picked by select, not by a dynamic index
            double fc[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) fc[k] = c == 0 ? f[0][k] : (c == 1 ? f[1][k] : f[2][k]);
            deg = row_line(fc, x, y, l0, l1, l2);
        }
        s_rl[lr][c][0] = l0;
        s_rl[lr][c][1] = l1;
        s_rl[lr][c][2] = l2;
        s_rl[lr][c][3] = x;
        s_rl[lr][c][4] = y;
        s_rdeg[lr][c] = deg;
    }

    const bool vec = (nd % 4 == 0) && (eo % 4 == 0) && ((reinterpret_cast<uintptr_t>(E) & 15) == 0);
    const int wrow0 = wave * kExtRowsPerWave;
    for (int c0 = 0; c0 < nd; c0 += kExtColTile) {
        __syncthreads();   // the previous tile's readers are done (and the row side is written)
        for (int jj = t; jj < kExtColTile; jj += kThreads) {
            const int j = c0 + jj;
            double x = 0, y = 0;
            uint32_t dg = 0;
            if (j < nd) {
                x = pts[2 * (od + j)];
                y = pts[2 * (od + j) + 1];
            }
#pragma unroll
            for (int c = 0; c < kExtAnchors; ++c) {
                double l0 = 0, l1 = 0, l2 = 0;
                if (j < nd && col_line(f[c], x, y, l0, l1, l2)) dg |= 1u << c;
                s_cl[c][0][jj] = l0;
                s_cl[c][1][jj] = l1;
                s_cl[c][2][jj] = l2;
            }
            s_cx[jj] = x;
            s_cy[jj] = y;
            s_cdeg[jj] = dg;
        }
        __syncthreads();
        const int tile = min(kExtColTile, nd - c0);
        for (int ch = 0; ch < tile; ch += kChunk) {
            const int jl = ch + kColsPerLane * lane;   // the lane's strip within the tile
            const int j = c0 + jl;
            if (j >= nd) continue;
            double cl[kExtAnchors][3][kColsPerLane], cx[kColsPerLane], cy[kColsPerLane];
            uint32_t cdeg[kColsPerLane];
#pragma unroll
            for (int q = 0; q < kColsPerLane; ++q) {
#pragma unroll
                for (int c = 0; c < kExtAnchors; ++c)
#pragma unroll
                    for (int k = 0; k < 3; ++k) cl[c][k][q] = s_cl[c][k][jl + q];
                cx[q] = s_cx[jl + q];
                cy[q] = s_cy[jl + q];
                cdeg[q] = s_cdeg[jl + q];
            }
            for (int r = 0; r < kExtRowsPerWave; ++r) {
                const int lr = wrow0 + r;
                if (row0 + lr >= n) break;
                const uint32_t rdeg = s_rdeg[lr][0] | s_rdeg[lr][1] << 1 | s_rdeg[lr][2] << 2;
                float v[kColsPerLane];
#pragma unroll
                for (int q = 0; q < kColsPerLane; ++q) {
                    double ec[kExtAnchors];
#pragma unroll
                    for (int c = 0; c < kExtAnchors; ++c) {
                        const double rl0 = s_rl[lr][c][0], rl1 = s_rl[lr][c][1], rl2 = s_rl[lr][c][2];
                        const double rx = s_rl[lr][c][3], ry = s_rl[lr][c][4];
                        double d1 = line_dist(cl[c][0][q], cl[c][1][q], cl[c][2][q], rx, ry);
                        double d2 = line_dist(rl0, rl1, rl2, cx[q], cy[q]);
                        d1 = (cdeg[q] >> c & 1u) ? kSentinel : d1;   // epipolar_matching.py:25-26
                        d2 = (rdeg >> c & 1u) ? kSentinel : d2;
                        ec[c] = 0.5 * (d1 + d2);                     // :28
                    }
                    v[q] = cube_f32(ec[0], ec[1], ec[2]);
                }
                float *drow = E + eo + (int64_t)(row0 + lr) * nd + j;
                if (vec) {
                    *reinterpret_cast<f32x4 *>(drow) = f32x4{v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (int q = 0; q < kColsPerLane; ++q)
                        if (j + q < nd) drow[q] = v[q];
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int mvm_extend_costs(const double *pts_dev, const int64_t *cam_offs_dev, const double *F_ext_dev,
                     const int32_t *match_dev, const int64_t *match_offs_dev,
                     const int32_t *count_dev, const int64_t *ext_offs_dev, int32_t n_scenes,
                     int32_t n_cams, int32_t max_rows, float *E_dev, mvm_stream_t stream) {
    mvm_clear_error();
    if (n_scenes < 0 || max_rows < 0) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "negative sizes");
    if (n_cams < 3 || n_cams > MVM_MAX_CAMS)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_cams=%d outside [3, %d]", n_cams, MVM_MAX_CAMS);
    if (n_scenes == 0 || n_cams == 3 || max_rows == 0) return MVM_OK;
    if (const int st = mvm_require_ptrs({{pts_dev, "pts_dev"},               {cam_offs_dev, "cam_offs_dev"},
                                         {F_ext_dev, "F_ext_dev"},           {match_dev, "match_dev"},
                                         {match_offs_dev, "match_offs_dev"}, {count_dev, "count_dev"},
                                         {ext_offs_dev, "ext_offs_dev"},     {E_dev, "E_dev"}}))
        return st;
    const int64_t row_blocks = ((int64_t)max_rows + kExtRows - 1) / kExtRows;
    const int64_t grid = (int64_t)n_scenes * (n_cams - kExtAnchors) * row_blocks;
    if (grid > kMaxGridBlocks)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_scenes=%d, max_rows=%d: more row tiles than one launch holds",
                        n_scenes, max_rows);
    extend_cost_kernel<<<(unsigned)grid, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        pts_dev, cam_offs_dev, F_ext_dev, match_dev, match_offs_dev, count_dev, ext_offs_dev, n_cams,
        (int32_t)row_blocks, E_dev);
    return mvm_check_launch("extend_cost_kernel");
}

}  // extern "C"
