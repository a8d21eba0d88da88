/*
 * mvmatch.h — C ABI of the MI355X multi-view epipolar matcher.
 *
 * This is the drop-in boundary for the hot path of the reference's
 * bpc/inference/epipolar_matching.py.  The reference's boundary is a Python
 * function-call boundary (process_pose.py:24 binds compute_cost_matrix /
 * match_objects by name; camera_utils.compute_fundamental_matrix is bound at
 * process_pose.py:26); the entry points below are what that module's compute
 * reduces to once the O(n^2)/O(n^3) loops move to the GPU.  Python binds them
 * with ctypes (bpc_baseline_amd/_native.py) and registers them as PyTorch
 * custom ops (bpc_baseline_amd/ops.py); INTEGRATION.md shows the bindings.
 *
 * Conventions
 *   - every pointer argument named *_dev is a caller-allocated DEVICE pointer;
 *     pointers without the suffix are host pointers;
 *   - work is enqueued on `stream` (a hipStream_t; NULL = default stream) and
 *     nothing is synchronised: results are ready when the stream reaches them;
 *   - no allocation, no host<->device copy and no global mutable state in any
 *     launch function (safe to capture in a hipGraph, re-entrant per stream);
 *     the library reads no environment variables: kernel-path choices come
 *     only from an explicit mvm_options argument (the *_ex entry points);
 *   - return value: MVM_OK or an MVM_ERR_* code; mvm_last_error_string()
 *     gives a per-thread message for the last failing call.
 *
 * Detections use a CSR layout: pts_dev holds (x, y) float64 centroids of all
 * detections, scene-major then camera-minor; cam_offs_dev[s*C + c] ..
 * cam_offs_dev[s*C + c + 1] is the detection range of camera c in scene s.
 * Fundamental matrices are float64, row-major, one per (scene, pair):
 * F_dev[(s*P + p)*9 + 3*r + c] = F[r][c] with F mapping camera pair_a[p]
 * points to camera pair_b[p] epipolar lines (camera_utils.py:23-46).
 */
#ifndef MVMATCH_H
#define MVMATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVM_ABI_VERSION 8
#define MVM_HAS_RIG_MATRICES 1 /* mvm_rig_matrices: an addition to ABI 8 (no existing
                                  signature or struct changed) */
#define MVM_HAS_EXTEND 1 /* mvm_extend_costs, mvm_extend_select_triangulate: additions to
                            ABI 8 (no existing signature or struct changed) */
#define MVM_HAS_VIEW_TABLE 1 /* mvm_compact_matches_views: an addition to ABI 8 (no existing
                                signature or struct changed) */
#define MVM_HAS_VIEW_PRUNE 1 /* mvm_prune_views_triangulate: an addition to ABI 8 (no existing
                                signature or struct changed) */
#define MVM_HAS_LEFTOVERS 1 /* mvm_mark_used, mvm_leftover_counts, mvm_leftover_gather: additions
                               to ABI 8 (no existing signature or struct changed) */
#define MVM_HAS_REFINE 1 /* mvm_refine_points: an addition to ABI 8 (no existing signature or
                            struct changed) */
#define MVM_HAS_CROPS 1 /* mvm_crop_views: an addition to ABI 8 (no existing signature or struct
                           changed) */
#define MVM_HAS_POSES 1 /* mvm_fuse_rotations: an addition to ABI 8 (no existing signature or
                           struct changed) */
#define MVM_HAS_SCORES 1 /* mvm_score_poses, mvm_match_scores: additions to ABI 8 (no existing
                            signature or struct changed) */
#define MVM_HAS_SYM_FUSE 1 /* mvm_fuse_rotations_sym: an addition to ABI 8 (no existing signature
                              or struct changed) */
#define MVM_HAS_BOX_FIT 1 /* mvm_fit_boxes: an addition to ABI 8 (no existing signature or struct
                             changed) */
#define MVM_MAX_CAMS 8
#define MVM_MAX_PAIRS 28 /* MVM_MAX_CAMS choose 2 */

typedef struct ihipStream_t *mvm_stream_t; /* == hipStream_t */

enum {
    MVM_OK = 0,
    MVM_ERR_INVALID_ARGUMENT = 1, /* null pointer, negative size, bad pair index */
    MVM_ERR_UNSUPPORTED = 2,      /* more cameras/pairs than MVM_MAX_* */
    MVM_ERR_WORKSPACE = 3,        /* workspace smaller than required */
    MVM_ERR_HIP = 4               /* a HIP runtime call or kernel launch failed */
};

/* Element types of mvm_lsap_*_ex cost matrices. */
enum { MVM_F32 = 0, MVM_F64 = 1 };

/* Library version string ("mvmatch <semver> gfx950"). */
const char *mvm_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char *mvm_last_error_string(void);
/* Static description of a status code. */
const char *mvm_status_string(int status);

/*
 * Kernel-path selection.  Every choice below selects among kernels that
 * compute the SAME outputs bit for bit (the parity tests run each path); none
 * changes what is computed, only how.  The plain entry points use the
 * compiled-in defaults, which are what mvm_options_init writes (every field
 * 0 = "default"); the *_ex entry points take a const mvm_options * (NULL =
 * defaults).  `size` must be sizeof(mvm_options) as the caller compiled it
 * (mvm_options_init sets it), so the struct can grow without breaking callers.
 */
enum {
    MVM_PAIRWISE_ARGMIN_DEFAULT = 0,     /* = LAZY_TRANSPOSED */
    MVM_PAIRWISE_ARGMIN_LAZY_TRANSPOSED, /* clean row groups: per-chunk minimum bits,
                                            one LDS transpose per row group */
    MVM_PAIRWISE_ARGMIN_LAZY_ROWS,       /* since ABI 3 an alias of LAZY_TRANSPOSED (the
                                            per-row DPP form was removed) */
    MVM_PAIRWISE_ARGMIN_EAGER            /* best value + index per pair */
};
enum {
    MVM_CUBE_DEFAULT = 0,   /* by the batch's largest view: SMALL <= 16, FUSED above */
    MVM_CUBE_SMALL,         /* one workgroup per scene (views < 64; FUSED otherwise) */
    MVM_CUBE_FUSED,         /* 16 i x 32 j tiles, pair residuals in the prologue
                               (views <= 256; k-chunked above) */
    MVM_CUBE_WORKSPACE,     /* fp64 pair matrices to the workspace, then tiles
                               (views <= 256; GENERIC above) */
    MVM_CUBE_GENERIC        /* fp64 workspace + one (i, j) row per wave */
};
typedef struct mvm_options {
    int32_t size;                   /* sizeof(mvm_options) */
    int32_t pairwise_argmin;        /* MVM_PAIRWISE_ARGMIN_* */
    int32_t pairwise_rows_per_wave; /* 0 default (16); 4, 8 or 16 */
    int32_t pairwise_row_groups;    /* 0 default (~256 rows per workgroup, ~128 for small grids); 1..16 */
    int32_t cube_kernel;            /* MVM_CUBE_* */
    int32_t cube_rows_per_instr;    /* FUSED: 0 default (by view size: 8 up to 32,
                                       then 4 / 2 / 1); 1, 2, 4 or 8 (i, j) rows per
                                       wave instruction, capped by the view size
                                       (2: <= 128, 4: <= 64, 8: <= 32) */
    int32_t lsap_wave_max_cols;     /* 0 default (1024); -1 never the one-wave
                                       kernel; else a long-side limit <= 1024 */
    int32_t lsap_multi_g;           /* 0 default (auto: as many co-resident
                                       workgroups per problem as fit, <= 16);
                                       -1 off; 2..16 forced */
    int32_t lsap_lds_max_cols;      /* 0 default (4096); -1 off: column state in LDS
                                       for long sides up to this */
    int32_t lsap_lds_small_cols;    /* 0 default (2048): ... of which up to this
                                       with 256 threads (1024 above) */
    int32_t lsap_mid_max_cols;      /* 0 default (8192): workspace-state long sides
                                       up to this with 256 threads (1024 above) */
    int32_t lsap_reg_max_cols;      /* 0 default (4096); -1 off: long sides up to this
                                       (short sides <= 1024) in one workgroup with the
                                       column state in registers (ABI 3) */
    int32_t lsap_reg_threads;       /* 0 default (512 threads, 8 columns each); 1024
                                       (4 each) */
    int32_t lsap_mreg_max_cols;     /* 0 default (65536); -1 off: long sides above
                                       lsap_reg_max_cols up to this (short sides <= 1024)
                                       over ceil(long / 4096) co-resident workgroups with
                                       the column state in registers (ABI 3) */
    int32_t pairwise_row_interleave; /* 0 default (by view size: on for views of more
                                       than 256); 1 a row group's rows interleave over
                                       the workgroup's 4 waves (at each row step they
                                       store 4 adjacent rows); -1 each wave's rows
                                       contiguous (ABI 3) */
    int32_t cube_cols_per_lane;     /* FUSED (views <= 256): 0 default (3 where the view
                                       fits 3 k per lane: <= 48 / 96 / 192 at four / two /
                                       one rows per instruction, else 4; then 5-8 k per
                                       lane at four or two rows per instruction where
                                       that keeps >= 8% more lanes busy, ABI 6); 3..8.
                                       3 lowers the rows per instruction until the view
                                       fits; 5-8 take the most rows per instruction
                                       (4 or 2) that hold the view; an error where no
                                       shape holds it (3: > 192; 5-8: > 32 k) or with a
                                       forced cube_rows_per_instr it does not fit, and
                                       for views > 256 (the k-chunked kernel) */
    int32_t pairwise_xcd_fronts;    /* 0 default (4 when the launch may write >= 8 GB of
                                       matrices -- judged from the padded bound
                                       n_scenes * n_pairs * max_n^2 * 4 B; the Python
                                       plan passes the real size's choice -- else 1);
                                       1..16: each XCD writes its eighth of the grid as
                                       this many concurrent contiguous ranges (ABI 5;
                                       +0.8-1.9% on C3, a margin of one box) */
    int32_t lsap_sparse_min_cols;   /* 0 default (4096); -1 off: problems with a long
                                       side >= this (and > the one-wave limit, <= 65536)
                                       and a short side <= 1024 are solved one workgroup
                                       each through per-row candidate lists (ABI 6) */
    int32_t lsap_sparse_blocks;     /* 0 default (16): candidate blocks (of 32 columns)
                                       per row of that class, 1..64 (ABI 6) */
    int32_t cube_tile_rows;         /* FUSED at two, four or eight rows per
                                       instruction: i rows per tile, 0 default (32 at
                                       eight rows per instruction, else 16), 16 or 32
                                       (the tile's prologue over twice the rows; ABI 6) */
} mvm_options;

/* Fill *opts with the defaults (all 0) and opts->size. */
void mvm_options_init(mvm_options *opts);

/*
 * Pairwise symmetric epipolar residuals + per-row argmin, batched over
 * (scene, camera pair).  Replaces the per-pair epipolar_error calls
 * (bpc/inference/epipolar_matching.py:5-28) with one launch; the per-row
 * argmin is SURVEY §8a row a5 (oracle: np.argmin(e_ab, axis=1)).
 *
 * For scene s and pair p = (a, b), with n_a, n_b detections in cameras a, b:
 *   e[i][j] = float32(epipolar_error(p_a[i], p_b[j], F[s, p]))       (fp64 math)
 *   dist_dev[dist_offs_dev[s*P + p] + i*n_b + j] = e[i][j]
 *   argmin_dev[row_offs_dev[s*P + p] + i] = lowest j minimising e[i][:]
 *                                             (NaN counts as smallest; -1 if n_b == 0)
 *   minval_dev[...]                         = e[i][argmin] (NaN if n_b == 0)
 * dist_dev, argmin_dev and minval_dev may each be NULL (not produced).
 * dist_offs_dev and row_offs_dev are the caller's: entry s*P + p is read on
 * its own, so the matrices may lie in any order, with gaps between them and at
 * any offset (a matrix whose offset or row length is not a multiple of 4 floats
 * is stored element by element, the others 16 bytes per lane); nothing outside
 * the matrices and row blocks is written.  dist_dev must be 16-byte aligned
 * (MVM_ERR_INVALID_ARGUMENT before any launch otherwise: the store width is
 * chosen from the offsets alone); argmin_dev and minval_dev need only their
 * element's alignment.
 * pair_a / pair_b are HOST arrays of n_pairs camera indices (a != b).
 * max_n is a host-known upper bound on every view's detection count (n_a and
 * n_b over all (scene, pair)): it sizes the grid and the LDS column tile;
 * rows/columns beyond the real counts are skipped on the device.
 */
int mvm_pairwise_residual_argmin(const double *pts_dev, const int64_t *cam_offs_dev,
                                 const double *F_dev, const int32_t *pair_a,
                                 const int32_t *pair_b, int32_t n_scenes, int32_t n_cams,
                                 int32_t n_pairs, int32_t max_n, const int64_t *dist_offs_dev,
                                 const int64_t *row_offs_dev, float *dist_dev,
                                 int32_t *argmin_dev, float *minval_dev, mvm_stream_t stream);
/* ... with explicit kernel-path options (NULL = defaults). */
int mvm_pairwise_residual_argmin_ex(const double *pts_dev, const int64_t *cam_offs_dev,
                                    const double *F_dev, const int32_t *pair_a,
                                    const int32_t *pair_b, int32_t n_scenes, int32_t n_cams,
                                    int32_t n_pairs, int32_t max_n, const int64_t *dist_offs_dev,
                                    const int64_t *row_offs_dev, float *dist_dev,
                                    int32_t *argmin_dev, float *minval_dev,
                                    const mvm_options *opts, mvm_stream_t stream);

/*
 * The same with pitched rows (ABI 3): row i of matrix (s, p) starts at
 *   dist_dev[dist_offs_dev[s*P + p] + i*ld],  ld = roundup(n_b, row_align),
 * so with row_align 32 (and matrix offsets that are multiples of 32) every
 * row starts on a 128-byte line and every store of a ragged view writes whole
 * lines.  Columns n_b .. ld-1 of a row are padding and hold +inf.  row_align
 * is a power of two in
 * [1, 256]; 1 is the unpitched layout of mvm_pairwise_residual_argmin_ex.
 * The caller sizes dist_dev and dist_offs_dev with the pitched sizes n_a*ld.
 * Matrix offsets that are not multiples of row_align are taken as they are
 * (rows then start off the lines; the results are the same).
 */
int mvm_pairwise_residual_argmin_pitched(const double *pts_dev, const int64_t *cam_offs_dev,
                                         const double *F_dev, const int32_t *pair_a,
                                         const int32_t *pair_b, int32_t n_scenes, int32_t n_cams,
                                         int32_t n_pairs, int32_t max_n, int32_t row_align,
                                         const int64_t *dist_offs_dev, const int64_t *row_offs_dev,
                                         float *dist_dev, int32_t *argmin_dev, float *minval_dev,
                                         const mvm_options *opts, mvm_stream_t stream);

/*
 * Same residuals kept in float64 (no cast), written with a uniform layout:
 * matrix (s, p) starts at e_dev + (s*P + p) * mat_stride and has row stride
 * ld (>= every n_b; use a multiple of 4 for vectorised stores).  This is the
 * exact fp64 value of epipolar_error (epipolar_matching.py:28) and the input
 * of the three-camera cube.  Of a matrix's padding, columns n_b ..
 * min(ld, roundup(n_b, 256)) - 1 of the rows i < n_a hold +inf; nothing else
 * is written: not the rows from n_a on, the columns from roundup(n_b, 256) on,
 * the rest of mat_stride, or anything past n_scenes * n_pairs * mat_stride.
 * e_dev must be 16-byte aligned (MVM_ERR_INVALID_ARGUMENT otherwise).
 */
int mvm_pairwise_residual_f64(const double *pts_dev, const int64_t *cam_offs_dev,
                              const double *F_dev, const int32_t *pair_a, const int32_t *pair_b,
                              int32_t n_scenes, int32_t n_cams, int32_t n_pairs,
                              int32_t max_n, int64_t mat_stride, int64_t ld, double *e_dev,
                              mvm_stream_t stream);

/*
 * Three-camera cost cube + per-(i,j) argmin over k, batched over scenes.
 * Replaces compute_cost_matrix (epipolar_matching.py:83-98):
 *   cube[i][j][k] = float32(((e12[i][j] + e13[i][k]) + e23[j][k]) / 3)
 * with e_ab the fp64 residuals of pairs (0,1), (0,2), (1,2); F_dev holds
 * F12, F13, F23 for every scene ([S*3, 9]); cam_offs_dev has S*3+1 entries.
 *   cube_dev[cube_offs_dev[s] + (i*M + j)*P + k]
 *   argmin_dev[row_offs_dev[s] + i*M + j]   (argmin over k of the flattened
 *                                            (N*M, P) cube row; -1 if P == 0)
 * max_n bounds every view's detection count.  workspace_dev must hold
 * mvm_triplet_workspace_bytes(n_scenes, max_n) bytes (16-byte aligned).
 * cube_offs_dev and row_offs_dev are the caller's: entry s is read on its own
 * (any order, gaps, any residue: a cube whose offset or P is not a multiple of
 * 4 floats is stored in dword-aligned pieces); nothing outside the cubes and
 * row blocks is written.  cube_dev must be 16-byte aligned
 * (MVM_ERR_INVALID_ARGUMENT before any launch otherwise: the access width is
 * chosen from the offsets alone); argmin_dev and minval_dev need only their
 * element's alignment.
 */
size_t mvm_triplet_workspace_bytes(int32_t n_scenes, int32_t max_n);
int mvm_triplet_cost_argmin(const double *pts_dev, const int64_t *cam_offs_dev,
                            const double *F_dev, int32_t n_scenes, int32_t max_n,
                            const int64_t *cube_offs_dev, const int64_t *row_offs_dev,
                            float *cube_dev, int32_t *argmin_dev, float *minval_dev,
                            void *workspace_dev, size_t workspace_bytes, mvm_stream_t stream);
/* ... with explicit kernel-path options (NULL = defaults). */
int mvm_triplet_cost_argmin_ex(const double *pts_dev, const int64_t *cam_offs_dev,
                               const double *F_dev, int32_t n_scenes, int32_t max_n,
                               const int64_t *cube_offs_dev, const int64_t *row_offs_dev,
                               float *cube_dev, int32_t *argmin_dev, float *minval_dev,
                               void *workspace_dev, size_t workspace_bytes,
                               const mvm_options *opts, mvm_stream_t stream);
/*
 * ... also writing, for the assignment that follows (mvm_lsap_solve_ex3), the
 * minimum over every group of 8 consecutive j of every (i, k) (ABI 6): for
 * scene s with view sizes N, M, P, row i * ceil(M/8) + g of P uint16 keys at
 * bmin8_dev + bmin8_offs_dev[s] holds, per k, the upper 16 bits of the
 * order-preserving key (float bits | 0x80000000) of min over j in [8g, 8g+8)
 * of cube[i][j][k] -- a lower bound of that minimum to 1/128 -- or 0 when any
 * of the eight is NaN.  The fused kernel (views of 17-256 detections, its
 * default shapes; with them requested, views of 33-48 take 32-j instead of
 * 48-j tiles) writes them itself; every other path reads them back from the
 * cube (cube_dev required).  Offsets that are multiples of 4 keys let the
 * kernel store 8 bytes per lane; any other offset is stored key by key.
 * bmin8_offs_dev is the caller's (entry s read on its own), and bmin8_dev must
 * be 8-byte aligned (MVM_ERR_INVALID_ARGUMENT before any launch otherwise).
 */
int mvm_triplet_cost_argmin_bmin8(const double *pts_dev, const int64_t *cam_offs_dev,
                                  const double *F_dev, int32_t n_scenes, int32_t max_n,
                                  const int64_t *cube_offs_dev, const int64_t *row_offs_dev,
                                  float *cube_dev, int32_t *argmin_dev, float *minval_dev,
                                  uint16_t *bmin8_dev, const int64_t *bmin8_offs_dev,
                                  void *workspace_dev, size_t workspace_bytes,
                                  const mvm_options *opts, mvm_stream_t stream);

/*
 * Cube-free association input (ABI 7): for an assignment of every scene's
 * flattened (N*M, P) cube that never reads the cube itself
 * (mvm_lsap_solve_resid, mvm_select_triangulate_resid), write only what
 * those need:
 *   bmin8_dev  optional (NULL: not written): the same 16-bit 8-row minima
 *              mvm_triplet_cost_argmin_bmin8 writes (bit for bit, same layout
 *              and offsets; stored key by key, so any offset and a base
 *              with a key's alignment);
 *   bm32_dev   the candidate-list kernels' 32-column block minima as 16-bit
 *              keys: for short-side column k of scene s, nb = ceil(M/32) *
 *              npad keys at bm32_dev + bm32_offs_dev[s] + k * nb (npad =
 *              roundup(N, 16)), block (jt, i) at jt * npad + i holding h, the
 *              smallest 8-row key (upper half of the order-preserving float32
 *              key, NaN 0) of columns i * M + 32 jt .. + 31; rows i >= N
 *              0xFFFF; offsets multiples of 16 (32-byte runs), bm32_dev
 *              16-byte aligned;
 *   resid_dev  every scene's float64 pair residuals, from which the
 *              assignment recomputes the entries it reads as
 *              float32(((e12 + e13) + e23) / 3), the cube's own arithmetic:
 *                resid_dev + s * stride             e12  [N][ld]  (i, j)
 *                resid_dev + s * stride + max_n*ld  e13T [P][ld]  (k, i)
 *                resid_dev + s * stride + 2*max_n*ld e23T [P][ld] (k, j)
 *              with ld = roundup(max_n, 4), stride = 3 * max_n * ld;
 *              resid_bytes >= mvm_triplet_workspace_bytes(n_scenes, max_n)
 *              (16-byte aligned).
 * Views of at most 256 detections.  Replaces the cube's 4 B per triple of HBM
 * writes with 2 B per 32 triples (+ 2 B per 8 with bmin8_dev)
 * (epipolar_matching.py:83-98 feeding :100-116).  The group and block
 * minima are taken in float32 and every one within 8 units of a 16-bit carry
 * is recomputed exactly in fp64, so the keys are those of the cube's own
 * values bit for bit.
 */
int mvm_triplet_minima(const double *pts_dev, const int64_t *cam_offs_dev, const double *F_dev,
                       int32_t n_scenes, int32_t max_n, uint16_t *bmin8_dev,
                       const int64_t *bmin8_offs_dev, uint16_t *bm32_dev, const int64_t *bm32_offs_dev,
                       double *resid_dev, size_t resid_bytes, const mvm_options *opts,
                       mvm_stream_t stream);

/*
 * Batched rectangular linear-sum assignment, identical to
 * scipy.optimize.linear_sum_assignment (the association step of
 * match_objects, bpc/inference/epipolar_matching.py:100-116, scipy 1.14's
 * shortest-augmenting-path algorithm, same tie-breaking and output order).
 * Problem p is the row-major float32 matrix at cost_dev + cost_offs_dev[p]
 * (cost_offs_dev is the caller's, entry p read on its own; cost_dev needs only
 * its element's alignment; ws_offs / out_offs are mvm_lsap_plan's)
 * with dims_dev[2p] rows and dims_dev[2p+1] columns (e.g. the flattened
 * (N*M, P) cube of mvm_triplet_cost_argmin).  Its min(rows, cols) assigned
 * (row, col) pairs go to row_ind_dev/col_ind_dev at out_offs_dev[p], sorted
 * by row; status_dev[p] = 0 ok, 1 NaN/-inf entries, 2 infeasible.
 * mvm_lsap_plan (HOST arrays, n+1 entries each) fills the per-problem
 * workspace byte offsets and output offsets and returns the workspace size
 * (or -1); copy both offset arrays to the device for mvm_lsap_solve.
 */
int64_t mvm_lsap_plan(int32_t n_problems, const int64_t *rows, const int64_t *cols,
                      int64_t *ws_offs, int64_t *out_offs);
int mvm_lsap_solve(const float *cost_dev, const int64_t *cost_offs_dev, const int64_t *dims_dev,
                   int32_t n_problems, const int64_t *ws_offs_dev, const int64_t *out_offs_dev,
                   void *workspace_dev, size_t workspace_bytes, int64_t *row_ind_dev,
                   int64_t *col_ind_dev, int32_t *status_dev, mvm_stream_t stream);
/*
 * mvm_lsap_solve with host-known bounds on max(rows, cols) over the non-empty
 * problems (long_max < 1: every problem is empty): kernel classes that cannot
 * have work are not launched, which matters for small batches of small
 * problems.  The bounds must hold; mvm_lsap_solve passes (1, INT64_MAX).
 */
int mvm_lsap_solve_bounded(const float *cost_dev, const int64_t *cost_offs_dev,
                           const int64_t *dims_dev, int32_t n_problems,
                           const int64_t *ws_offs_dev, const int64_t *out_offs_dev,
                           void *workspace_dev, size_t workspace_bytes, int64_t *row_ind_dev,
                           int64_t *col_ind_dev, int32_t *status_dev, int64_t long_min,
                           int64_t long_max, mvm_stream_t stream);
/*
 * Cost matrices of element type cost_dtype (MVM_F32 or MVM_F64: scipy
 * assigns a float64 matrix in float64, so a float64 caller must not be
 * narrowed), with explicit kernel-path options (NULL = defaults).  The
 * workspace must come from mvm_lsap_plan_ex with the same cost_dtype.
 */
int64_t mvm_lsap_plan_ex(int32_t n_problems, const int64_t *rows, const int64_t *cols,
                         int32_t cost_dtype, int64_t *ws_offs, int64_t *out_offs);
int mvm_lsap_solve_ex(const void *cost_dev, int32_t cost_dtype, const int64_t *cost_offs_dev,
                      const int64_t *dims_dev, int32_t n_problems, const int64_t *ws_offs_dev,
                      const int64_t *out_offs_dev, void *workspace_dev, size_t workspace_bytes,
                      int64_t *row_ind_dev, int64_t *col_ind_dev, int32_t *status_dev,
                      int64_t long_min, int64_t long_max, const mvm_options *opts,
                      mvm_stream_t stream);
/*
 * ... with a host-known bound on min(rows, cols) as well (ABI 6): it sizes the
 * candidate-list kernels' LDS (a workgroup per problem holds state for every
 * short-side row).  mvm_lsap_solve_ex passes short_max = long_max.
 */
int mvm_lsap_solve_ex2(const void *cost_dev, int32_t cost_dtype, const int64_t *cost_offs_dev,
                       const int64_t *dims_dev, int32_t n_problems, const int64_t *ws_offs_dev,
                       const int64_t *out_offs_dev, void *workspace_dev, size_t workspace_bytes,
                       int64_t *row_ind_dev, int64_t *col_ind_dev, int32_t *status_dev,
                       int64_t long_min, int64_t long_max, int64_t short_max,
                       const mvm_options *opts, mvm_stream_t stream);
/*
 * ... taking the block minima of cubes from mvm_triplet_cost_argmin_bmin8
 * (ABI 6): problem p's cost is a flattened (N*M, P) cube (segs_dev[p] = M)
 * whose 8-row minima are at bmin8_dev + bmin8_offs_dev[p].  The candidate-list
 * kernels then read those (N * ceil(M/8) * P keys) instead of the whole cost
 * once more; results are the same.  Ignored for float64 costs and for
 * problems outside the class; all three pointers NULL = mvm_lsap_solve_ex2.
 */
int mvm_lsap_solve_ex3(const void *cost_dev, int32_t cost_dtype, const int64_t *cost_offs_dev,
                       const int64_t *dims_dev, int32_t n_problems, const int64_t *ws_offs_dev,
                       const int64_t *out_offs_dev, void *workspace_dev, size_t workspace_bytes,
                       int64_t *row_ind_dev, int64_t *col_ind_dev, int32_t *status_dev,
                       int64_t long_min, int64_t long_max, int64_t short_max,
                       const uint16_t *bmin8_dev, const int64_t *bmin8_offs_dev,
                       const int64_t *segs_dev, const mvm_options *opts, mvm_stream_t stream);

/*
 * Cube-free assignment (ABI 7): mvm_lsap_solve_ex3 for the flattened (N*M, P)
 * cubes of a mvm_triplet_minima batch, without the cubes.  Problem p is
 * scene p: dims (N*M, P), segs_dev[p] = M, its pair residuals at resid_dev
 * (max_n as given to mvm_triplet_minima); the kernels recompute every entry
 * they read with the cube's arithmetic, so the result is that of
 * mvm_lsap_solve_ex3 on the cubes (and scipy's).  The candidate lists start
 * from bm32_dev (mvm_triplet_minima's 16-bit block minima, no reduction pass)
 * and, when bmin8_dev is not NULL, refine each candidate block to its 8-column
 * groups by the 8-row minima at bmin8_dev + bmin8_offs_dev[p] (without them
 * they gather whole blocks).  There is no cost for the dense classes to read, so every
 * non-empty problem must be of the candidate-list class (long sides >=
 * mvm_options.lsap_sparse_min_cols (default 4096) and > lsap_wave_max_cols
 * (1024), <= 65536; short sides <= 1024): the host bounds are checked
 * (MVM_ERR_INVALID_ARGUMENT), and a problem outside them on the device gets
 * status 4.  The workspace comes from mvm_lsap_plan_resid (the class's
 * candidate lists only: ~0.3 MB per 256^3 scene).
 * Statuses of every mvm_lsap_solve* entry point: 0 ok, 1 NaN / -inf entries
 * (scipy's ValueError), 2 infeasible, 3 internal (a co-resident wait timed
 * out), 4 refused by the candidate-list class (below).
 * The host bounds (long_min / long_max / short_max) are a contract, not a
 * check: long_min <= every non-empty problem's long side <= long_max and every
 * short side <= short_max.  They may be as loose as the caller likes (a
 * capacity instead of the batch's maxima; mvm_lsap_solve passes (1,
 * INT64_MAX)): the classes are then all launched, each problem is still
 * solved by exactly one of them, and the results are the same.  What happens
 * to a problem past them depends on the class that owns it:
 *   - the candidate-list class (mvm_lsap_sparse.hip) sizes its LDS from
 *     min(short_max, 1024) and min(long_max, 65536) and REFUSES a problem of
 *     its class past either with status 4 (no assignment, its counters 0); in
 *     mvm_lsap_solve_resid it also gives status 4 to a problem outside the
 *     class, which no other kernel could solve without a cube;
 *   - the dense classes (mvm_lsap.hip: one wave, register state, split
 *     register state, split workspace state, LDS state, workspace state)
 *     contain no such refusal: they size dynamic LDS from the bounds and skip
 *     launches by them, so for their problems the bounds MUST HOLD -- a problem
 *     past them may be left unsolved (its status not written) or run a kernel
 *     with too little LDS.
 */
int64_t mvm_lsap_plan_resid(int32_t n_problems, const int64_t *rows, const int64_t *cols,
                            int64_t *ws_offs, int64_t *out_offs);
/* The candidate-list class's limits (ABI 7): the default lower bound of its
 * long sides (mvm_options.lsap_sparse_min_cols 0), its largest long side and
 * its largest short side.  Any pointer may be NULL. */
void mvm_lsap_sparse_bounds(int32_t *min_cols, int32_t *max_cols, int32_t *max_short);
/* Byte offset, inside a (rows x cols) problem's workspace region, of the
 * candidate-list solver's counters for it (ABI 7): int32 [4] = dense scans for
 * a row's free minimum (no list, or no free entry left in it), dense scans for
 * the free ties at a search's end, rows whose candidate list overflowed,
 * Dijkstra steps.  Written by every solve of a problem of that class; one that
 * ends with a status other than 0 leaves all four 0. */
int64_t mvm_lsap_sparse_stats_offset(int64_t rows, int64_t cols);
int mvm_lsap_solve_resid(const int64_t *dims_dev, int32_t n_problems, const int64_t *ws_offs_dev,
                         const int64_t *out_offs_dev, void *workspace_dev, size_t workspace_bytes,
                         int64_t *row_ind_dev, int64_t *col_ind_dev, int32_t *status_dev,
                         int64_t long_min, int64_t long_max, int64_t short_max,
                         const uint16_t *bmin8_dev, const int64_t *bmin8_offs_dev,
                         const uint16_t *bm32_dev, const int64_t *bm32_offs_dev,
                         const int64_t *segs_dev, const double *resid_dev, int32_t max_n,
                         const mvm_options *opts, mvm_stream_t stream);

/*
 * On-device detection packing, replacing the per-box loop of
 * PoseEstimator._detect (bpc/inference/process_pose.py:122-140).  Input:
 * the detector's boxes of n_img images in CSR form: boxes_dev f32 [n, 4]
 * (xyxy), conf_dev f32 [n], cls_dev f32 [n], image k owning rows
 * [img_offs_dev[k], img_offs_dev[k+1]).  A box is kept when cls == class_id
 * and conf >= conf_thresh (both float32 compares, :130), in input order.
 * Output, the matcher's CSR input: counts_dev int32 [n_img],
 * cam_offs_dev int64 [n_img+1] (exclusive prefix of counts), boxes_out_dev
 * int32 [kept, 4] = int(box) (truncation toward zero, :134) and pts_dev f64
 * [kept, 2] = 0.5 * (x1 + x2), 0.5 * (y1 + y2) (:135-136).  Capacity of the
 * two row outputs must be img_offs[n_img] rows.  status_dev[0] = 1 if a kept
 * box had a non-finite coordinate or one with |x| >= 2^30 (stored as 0).
 */
int mvm_pack_detections(const float *boxes_dev, const float *conf_dev, const float *cls_dev,
                        const int64_t *img_offs_dev, int32_t n_img, float conf_thresh,
                        float class_id, int32_t *counts_dev, int64_t *cam_offs_dev,
                        double *pts_dev, int32_t *boxes_out_dev, int32_t *status_dev,
                        mvm_stream_t stream);

/*
 * Batched DLT triangulation, replacing triangulate_multi_view
 * (bpc/inference/epipolar_matching.py:118-127) as called per match by
 * PosePrediction.triangulate (process_pose.py:86-94).  Point p uses the
 * n_views projection matrices (f64, row-major 3x4) of set
 * set_of_point_dev[p] (or set p when NULL) at proj_dev + set*n_views*12 and
 * its 2-D points pts2d_dev [n_points, n_views, 2]; X_dev [n_points, 3] =
 * X[:3] / X[3] of the right singular vector of the smallest singular value
 * of the 2V x 4 system.  fp64; agrees with LAPACK to rounding (the vector is
 * unique up to sign, which the division cancels).  2 <= n_views <= 8.
 */
int mvm_triangulate_dlt(const double *proj_dev, const int32_t *set_of_point_dev,
                        const double *pts2d_dev, int32_t n_points, int32_t n_views, double *X_dev,
                        mvm_stream_t stream);

/*
 * The tail of PoseEstimator._match (process_pose.py:182-187) for a batch of
 * 3-camera scenes, after mvm_triplet_cost_argmin and mvm_lsap_solve: scene
 * s's assignment (row_ind/col_ind at lsap_out_offs_dev[s], the flattened
 * (N*M, P) cube at cube_offs_dev[s]) is filtered by cube value < threshold
 * (match_objects :111; compared in float64, as numpy 1.26 compares a float32
 * scalar with a Python number: (double)value < threshold, so under threshold
 * 0.7 a cost of float32(0.7) is kept; NaN on either side keeps nothing; the
 * CPU restatements oracle/lsap.match_objects and oracle/pipeline.select_sort
 * compare the same way under any NumPy), decoded i = r / M, j = r % M, k = c
 * (:112-114), stably sorted by cost (:183) and triangulated from the
 * centroids pts_dev (CSR cam_offs_dev, 3 views per scene) with the scene's
 * projection matrices proj_dev [S, 3, 3, 4] (K @ RT[:3], :86-94).  Match w
 * of scene s (w < count_dev[s]) is written at lsap_out_offs_dev[s] + w:
 * match_dev int32 [.., 3] = (i, j, k), cost_dev f32, X_dev f64 [.., 3]; rows
 * from count_dev[s] on are not written.
 * A pair (r, c) that is not an index of the scene's problem (r outside
 * [0, N*M) or c outside [0, P)) is ignored, as one over the threshold is: no
 * index is used unchecked.  A problem whose status is not 0 got no
 * assignment, and its row_ind / col_ind region holds what it held before
 * (uninitialised memory, an earlier batch's indices): the launch stays inside
 * its buffers whatever that is, and the pairs among it that are indices are
 * selected like any other, so a caller looks at status_dev before it uses
 * that scene's matches.
 */
int mvm_select_triangulate(const float *cube_dev, const int64_t *cube_offs_dev,
                           const int64_t *cam_offs_dev, const int64_t *lsap_out_offs_dev,
                           const int64_t *row_ind_dev, const int64_t *col_ind_dev,
                           const double *pts_dev, const double *proj_dev, int32_t n_scenes,
                           double threshold, int32_t *match_dev, float *cost_dev, double *X_dev,
                           int32_t *count_dev, mvm_stream_t stream);
/* ... cube-free (ABI 7): each assigned entry recomputed from the pair
 * residuals of mvm_triplet_minima (resid_dev, max_n as given there) with the
 * cube's arithmetic -- the same costs, matches and order as from the cube. */
int mvm_select_triangulate_resid(const double *resid_dev, int32_t max_n, const int64_t *cam_offs_dev,
                                 const int64_t *lsap_out_offs_dev, const int64_t *row_ind_dev,
                                 const int64_t *col_ind_dev, const double *pts_dev,
                                 const double *proj_dev, int32_t n_scenes, double threshold,
                                 int32_t *match_dev, float *cost_dev, double *X_dev, int32_t *count_dev,
                                 mvm_stream_t stream);

/*
 * The dense match table (ABI 8): the matches the select kernels left at
 * seg_offs_dev[s] (the lsap_out_offs_dev they were given), with unused rows
 * behind each scene and as per-view indices, copied to consecutive rows that
 * stand on their own -- what PosePrediction holds (process_pose.py:79-94:
 * boxes, centroids, t) plus the scene id, so a table can leave the device
 * or the rank that made it.  Inputs (read only, not aliasing the outputs):
 * match_dev int32 [cap, 3], cost_dev f32 [cap], X_dev f64 [cap, 3],
 * count_dev int32 [S] as mvm_select_triangulate(_resid) wrote them under
 * seg_offs_dev int64 [S+1]; pts_dev f64 [n, 2], boxes_dev int32 [n, 4],
 * cam_offs_dev int64 [3S+1] as mvm_pack_detections wrote them.
 * Precondition: 0 <= count[s] <= seg_offs[s+1] - seg_offs[s] (true of
 * everything the select kernels produce; not checked).
 * Outputs, each with room for seg_offs[S] rows: dense_offs_dev int64 [S+1] =
 * the exclusive prefix sum of count; for match w of scene s, at row
 * r = dense_offs[s] + w: scene_out_dev[r] = scene_base + s (int32),
 * match_out_dev[r] = (i, j, k) (int32 [3]), cost_out_dev[r] (f32),
 * X_out_dev[r] (f64 [3]), boxes_out_dev[r] = boxes[cam_offs[3s+c] + idx_c],
 * c = 0..2 (int32 [3, 4]) and cent_out_dev[r] = the same rows of pts
 * (f64 [3, 2]).  Every value is a copy (bit-exact); rows at and beyond
 * dense_offs[S] are not written.  Two launches (the prefix sum, the copy);
 * n_scenes == 0 launches nothing.
 */
int mvm_compact_matches(const int32_t *match_dev, const float *cost_dev, const double *X_dev,
                        const int32_t *count_dev, const int64_t *seg_offs_dev, const double *pts_dev,
                        const int32_t *boxes_dev, const int64_t *cam_offs_dev, int32_t n_scenes,
                        int32_t scene_base, int64_t *dense_offs_dev, int32_t *scene_out_dev,
                        int32_t *match_out_dev, float *cost_out_dev, double *X_out_dev,
                        int32_t *boxes_out_dev, double *cent_out_dev, mvm_stream_t stream);

/*
 * Fundamental and projection matrices on the device (an addition to ABI 8,
 * announced by MVM_HAS_RIG_MATRICES): compute_fundamental_matrix
 * (camera_utils.py:23-46) for every (capture, pair) and P = K @ RT[:3]
 * (process_pose.py:91) for every (capture, camera), replacing the host's
 * per-capture numpy products.  K_dev f32 [S, C, 3, 3], RT_dev f64 [S, C, 4, 4]
 * (row-major [R|t] over (0, 0, 0, 1)); pair_a / pair_b are HOST arrays of
 * n_pairs camera indices (a != b, validated here and passed by value), F
 * mapping camera pair_a[p] points to camera pair_b[p] lines.  Outputs:
 * F_dev f64 [S * n_pairs, 9] (the layout every matcher entry point reads),
 * proj_dev f64 [S, C, 3, 4] (NULL: not produced; mvm_select_triangulate's and
 * mvm_triangulate_dlt's input) and status_dev int32 [S].
 * Arithmetic: the reference's, step by step and dtype by dtype, every dot
 * product in index order k = 0, 1, 2.  The fp64 products of F are FMA chains
 * (a0 * b0, then one fma per further term), as the OpenBLAS FMA kernels behind
 * numpy's matmul evaluated them in the reference run; the float32 inverse and
 * P round every product and sum on their own:
 *   R_rel = R2 R1^T, t_rel = t2 - R_rel t1                      fp64 (:27-28)
 *   skew(t_rel) cast to float32, promoted back                   (:31-35)
 *   E = skew R_rel                                               fp64 (:37)
 *   Kinv in float32 by back substitution dividing by the diagonal,
 *     x[r] = (b[r] - sum_{q>r} K[r][q] x[q]) / K[r][r], promoted (:38-39)
 *   F = (K2inv^T E) K1inv, left to right                         fp64 (:40)
 *   F /= F[2][2] only when fabs(F[2][2]) > 1e-8                  (:43-44)
 *   P = (double)K RT[:3, :]                           (process_pose.py:91)
 * The back substitution is np.linalg.inv's result bit for bit only for a
 * PINHOLE K: K[1][0] == K[2][0] == K[2][1] == 0, K[0][1] == 0, K[2][2] == 1,
 * K[0][0] != 0 and K[1][1] != 0 (every BOP cam_K).  F and P then equal the
 * host function's bit for bit where the host BLAS evaluates as above (the
 * reference's recorded F does), and F to a few 1e-14 relative on a BLAS that
 * sums otherwise.  status_dev[s] = 0: every K of capture
 * s is pinhole and its rows are written; 1: some K is not, and NONE of that
 * capture's F or proj rows is written -- the caller computes them
 * (camera_utils.compute_fundamental_matrix).  One launch of S * (n_pairs + C)
 * work items; n_scenes == 0 launches nothing.
 */
int mvm_rig_matrices(const float *K_dev, const double *RT_dev, const int32_t *pair_a,
                     const int32_t *pair_b, int32_t n_scenes, int32_t n_cams, int32_t n_pairs,
                     double *F_dev, double *proj_dev, int32_t *status_dev, mvm_stream_t stream);

/*
 * Extension of three-view matches into the extra cameras of a C-camera rig,
 * 4 <= C <= MVM_MAX_CAMS (additions to ABI 8, announced by MVM_HAS_EXTEND).
 * Cameras 0, 1, 2 of every capture go through the three-camera chain above,
 * which leaves capture s's count_dev[s] matches (i, j, k) at rows
 * match_offs_dev[s] + w of match_dev (the lsap_out_offs_dev given to
 * mvm_select_triangulate).  For each extra camera d = 3 .. C-1 with n_d
 * detections q_l, mvm_extend_costs writes the float32 matrix
 *   E_d[w][l] = float32(((e_0d(p0[i_w], q_l) + e_1d(p1[j_w], q_l)) + e_2d(p2[k_w], q_l)) / 3)
 * with e_cd(p, q) = epipolar_error(p, q, F_cd) in fp64, the 9999 sentinel
 * included (epipolar_matching.py:5-28): the arithmetic of a cube entry
 * (:78-81, :96) with the match's own detections as the three anchors, NaN /
 * inf propagated as the cube does.  An (i, j, k) outside its view counts as a
 * NaN centroid.
 *   pts_dev / cam_offs_dev   the C-camera CSR (cam_offs_dev int64 [C*S + 1]);
 *   F_ext_dev   f64 [S, C-3, 3, 9]: per capture F_0d, F_1d, F_2d for d = 3, 4, ..
 *               (pairs (0,3), (1,3), (2,3), (0,4), ...), F_cd mapping camera c
 *               points to camera d lines;
 *   ext_offs_dev int64 [S*(C-3) + 1]: E_d of capture s starts at float
 *               ext_offs[s*(C-3) + d-3] of E_dev, row-major [count[s]][n_d],
 *               contiguous -- what mvm_lsap_solve* reads through cost_offs /
 *               dims.  The region must hold count[s] * n_d floats; rows it has
 *               no room for are not written.  Rows of a matrix with n_d % 4 ==
 *               0 that starts on a 16-byte boundary are stored 16 bytes per
 *               lane, others element by element;
 *   max_rows    a host bound on count[s] (sizes the grid; rows at and beyond
 *               count[s] are never written, nor is anything outside the
 *               matrices).
 * One launch, a workgroup per 64 rows of one (capture, d).  n_scenes == 0,
 * C == 3 or max_rows == 0 launch nothing.
 */
int mvm_extend_costs(const double *pts_dev, const int64_t *cam_offs_dev, const double *F_ext_dev,
                     const int32_t *match_dev, const int64_t *match_offs_dev,
                     const int32_t *count_dev, const int64_t *ext_offs_dev, int32_t n_scenes,
                     int32_t n_cams, int32_t max_rows, float *E_dev, mvm_stream_t stream);
/*
 * ... its tail, after the assignment of every E_d (mvm_lsap_solve* over the
 * S*(C-3) problems (count[s], n_d): row_ind_dev / col_ind_dev under
 * lsap_out_offs_dev int64 [S*(C-3) + 1]).  For match w of capture s, at row
 * r = match_offs[s] + w: views_dev int32 [.., C] = (i, j, k, -1, ...) and
 * ext_cost_dev f32 [.., C-3] = +inf; then each assigned pair (w, l) of camera
 * d with (double)E_d[w][l] < threshold (mvm_select_triangulate's compare:
 * NaN on either side keeps nothing) sets views[r][d] = l and
 * ext_cost[r][d-3] = E_d[w][l].  X_dev f64 [.., 3] is in/out: a match that
 * kept an extra view gets the DLT (mvm_triangulate_dlt's) over cameras
 * {0, 1, 2} and its kept ones in ascending order with proj_dev [S, C, 3, 4];
 * a match that kept none keeps the value X_dev held, bit for bit.  Rows
 * outside [match_offs[s], match_offs[s] + count[s]) of views / ext_cost / X
 * are not written.  Assigned pairs that are not indices of E_d (a failed
 * assignment's) are ignored.  One workgroup per capture; n_scenes == 0 or
 * C == 3 launch nothing.
 */
int mvm_extend_select_triangulate(const float *E_dev, const int64_t *ext_offs_dev,
                                  const int64_t *lsap_out_offs_dev, const int64_t *row_ind_dev,
                                  const int64_t *col_ind_dev, const int32_t *match_dev,
                                  const int64_t *match_offs_dev, const int32_t *count_dev,
                                  const double *pts_dev, const int64_t *cam_offs_dev,
                                  const double *proj_dev, int32_t n_scenes, int32_t n_cams,
                                  double threshold, int32_t *views_dev, float *ext_cost_dev,
                                  double *X_dev, mvm_stream_t stream);

/*
 * The dense match table of a C-camera batch, 3 <= C <= MVM_MAX_CAMS, with the
 * reprojection residual of every kept view (an addition to ABI 8, announced
 * by MVM_HAS_VIEW_TABLE): mvm_compact_matches over the C view slots.  Inputs
 * (read only, not aliasing the outputs): views_dev int32 [cap, C], cost_dev
 * f32 [cap], ext_cost_dev f32 [cap, C-3], X_dev f64 [cap, 3], count_dev int32
 * [S] under seg_offs_dev int64 [S+1], as mvm_select_triangulate(_resid) and
 * mvm_extend_select_triangulate left them (C == 3: match_dev is views_dev, and
 * ext_cost_dev / ext_cost_out_dev, arrays of no element, may be NULL);
 * pts_dev f64 [n, 2], boxes_dev int32 [n, 4], cam_offs_dev int64 [C*S + 1]:
 * the C-camera CSR of mvm_pack_detections; proj_dev f64 [S, C, 3, 4].
 * Preconditions (not checked): 0 <= count[s] <= seg_offs[s+1] - seg_offs[s],
 * and every views entry is -1 or a detection of its view.
 * Outputs, each with room for seg_offs[S] rows: dense_offs_dev int64 [S+1] =
 * the exclusive prefix sum of count; for match w of capture s, at row
 * r = dense_offs[s] + w, with v_c = views[seg_offs[s] + w][c]:
 *   scene_out_dev[r]     int32         scene_base + s
 *   views_out_dev[r]     int32 [C]     the v_c (-1: no detection in that view)
 *   n_views_out_dev[r]   int32         the number of v_c >= 0
 *   cost_out_dev[r]      f32           copied
 *   ext_cost_out_dev[r]  f32 [C-3]     copied
 *   X_out_dev[r]         f64 [3]       copied
 *   boxes_out_dev[r]     int32 [C, 4]  boxes[cam_offs[C*s + c] + v_c], or
 *                                      (-1, -1, -1, -1) where v_c < 0
 *   cent_out_dev[r]      f64 [C, 2]    the same rows of pts, or quiet NaN
 *   reproj_out_dev[r]    f64 [C]       the residual below, or quiet NaN
 * Reprojection residual of view c, with P = proj[s][c], X the row's X and
 * (cx, cy) its centroid in that view -- fp64, in exactly this order, every
 * product and sum rounded on its own (no FMA), IEEE division and square root:
 *   h_q = ((P[q][0]*X0 + P[q][1]*X1) + P[q][2]*X2) + P[q][3]      q = 0, 1, 2
 *   u = h_0 / h_2;  v = h_1 / h_2;  du = u - cx;  dv = v - cy
 *   reproj = sqrt(du*du + dv*dv)
 * (h_2 == 0 gives inf or NaN as IEEE does.)  Copied values are bit-exact;
 * rows at and beyond dense_offs[S] are not written.  Two launches (the prefix
 * sum, the copy) on `stream`, no allocation, copy or synchronisation;
 * n_scenes == 0 launches nothing.  A NULL pointer other than the two optional
 * ones, or n_cams outside 3..MVM_MAX_CAMS, is refused before any launch.
 */
int mvm_compact_matches_views(const int32_t *views_dev, const float *cost_dev,
                              const float *ext_cost_dev, const double *X_dev, const int32_t *count_dev,
                              const int64_t *seg_offs_dev, const double *pts_dev,
                              const int32_t *boxes_dev, const int64_t *cam_offs_dev,
                              const double *proj_dev, int32_t n_scenes, int32_t n_cams,
                              int32_t scene_base, int64_t *dense_offs_dev, int32_t *scene_out_dev,
                              int32_t *views_out_dev, int32_t *n_views_out_dev, float *cost_out_dev,
                              float *ext_cost_out_dev, double *X_out_dev, int32_t *boxes_out_dev,
                              double *cent_out_dev, double *reproj_out_dev, mvm_stream_t stream);

/*
 * Pruning of extra views by reprojection residual, with re-triangulation, for
 * a C-camera batch, 4 <= C <= MVM_MAX_CAMS (an addition to ABI 8, announced by
 * MVM_HAS_VIEW_PRUNE).  In/out, as mvm_extend_select_triangulate left them:
 * views_dev int32 [.., C], ext_cost_dev f32 [.., C-3], X_dev f64 [.., 3], with
 * capture s's count_dev[s] matches at rows match_offs_dev[s] + w (never more
 * rows than match_offs[s+1] - match_offs[s]); pts_dev / cam_offs_dev the
 * C-camera CSR, proj_dev f64 [S, C, 3, 4].  gate: pixels, 0 <= gate <= +inf.
 * For match w, with the kept set K = {0, 1, 2} + {d >= 3 : views[w][d] >= 0}:
 *   1. X = the DLT over K in ascending camera order (mvm_triangulate_dlt's);
 *      on the first pass, nothing dropped yet, the value X_dev holds;
 *   2. r_d, d in K, d >= 3: the reprojection residual of
 *      mvm_compact_matches_views, in that order of operations;
 *   3. the candidates are the d with !(r_d <= gate) (a NaN residual is one);
 *      none: stop.  Else the worst is dropped -- NaN above every number, then
 *      the largest r_d, ties to the lowest camera: views[w][d] = -1,
 *      ext_cost[w][d-3] = +inf, bit d of pruned_dev[w] set;
 *   4. back to 1 (at most C-3 drops).
 * Cameras 0-2 are never dropped; a detection a drop releases is not offered
 * to another match.  A row that drops nothing has views / ext_cost / X not
 * written and pruned_dev[w] = 0; so has a row whose (i, j, k) are outside
 * their views, or with an extra-view entry that is neither negative (no
 * detection) nor a detection of its view: no index is used unchecked.
 * pruned_dev int32 [..] is written for the count_dev[s] rows of every
 * capture; no row outside them is written in any array.
 * One launch on `stream`, a wave per capture; no allocation, copy or
 * synchronisation.  n_scenes == 0 launches nothing.  A NULL pointer, n_cams
 * outside 4..MVM_MAX_CAMS, a NaN or a negative gate is refused before the launch.
 */
int mvm_prune_views_triangulate(const int64_t *match_offs_dev, const int32_t *count_dev,
                                int32_t n_scenes, int32_t n_cams, const double *pts_dev,
                                const int64_t *cam_offs_dev, const double *proj_dev, double gate,
                                int32_t *views_dev, float *ext_cost_dev, double *X_dev,
                                int32_t *pruned_dev, mvm_stream_t stream);

/*
 * The leftovers of a C-camera batch, 4 <= C <= MVM_MAX_CAMS: what an extra
 * seed pass is run on (additions to ABI 8, announced by MVM_HAS_LEFTOVERS).
 * Every function takes the pass's seed triple (seed_a, seed_b, seed_c), three
 * distinct cameras < C, which fixes the camera order pi = (seed_a, seed_b,
 * seed_c, then the other cameras ascending): slot q stands for camera pi[q].
 * cam_offs_dev int64 [C S + 1] is the batch's C-camera CSR in original camera
 * order, used_dev int32 [n_det] a flag per detection of it.
 *
 * mvm_mark_used: for every match row w < count_dev[s] of capture s (rows
 * match_offs_dev[s] + w of views_dev int32 [n_rows, C]; never more rows than
 * match_offs[s+1] - match_offs[s]) and every slot q, the detection
 * l = views[w][q] of camera pi[q] gets used_dev[cam_offs[s C + pi[q]] + l] = 1.
 * With sub_cam_offs_dev (int64 [C S + 1], slot order) and orig_dev (int32, one
 * per detection of that CSR) -- both or neither -- l indexes slot q's view of
 * that CSR and orig_dev[sub_cam_offs[s C + q] + l] is the index in the original
 * view: the result of an earlier extra pass.  An l that is negative or not an
 * index of its view marks nothing; no other word of used_dev is written, so
 * the caller zeroes it once and marks pass after pass.  The triple (0, 1, 2)
 * is the identity order of a first pass.
 *
 * mvm_leftover_counts: counts_dev int32 [C S], slot order: counts[s C + q] =
 * the detections of camera pi[q] of capture s whose flag is 0.
 *
 * mvm_leftover_gather: those detections, in ascending index order, to rows
 * sub_cam_offs_dev[s C + q] + 0, 1, ... of pts_out_dev (f64 [.., 2]),
 * boxes_out_dev (int32 [.., 4]) and orig_out_dev (int32: the index in the
 * original view); sub_cam_offs_dev is the prefix sum of mvm_leftover_counts'
 * result, and never more rows are written than it leaves a view.
 *
 * One launch each on `stream`; no allocation, copy or synchronisation.
 * n_scenes == 0 launches nothing (and mvm_mark_used none for n_rows == 0 or
 * n_det == 0).  A NULL pointer, n_cams outside 4..MVM_MAX_CAMS, a triple with a
 * repeated or out-of-range camera is refused before the launch.
 */
int mvm_mark_used(const int32_t *views_dev, const int64_t *match_offs_dev, const int32_t *count_dev,
                  int64_t n_rows, int32_t n_scenes, int32_t n_cams, int32_t seed_a, int32_t seed_b,
                  int32_t seed_c, const int64_t *sub_cam_offs_dev, const int32_t *orig_dev,
                  const int64_t *cam_offs_dev, int64_t n_det, int32_t *used_dev, mvm_stream_t stream);
int mvm_leftover_counts(const int32_t *used_dev, const int64_t *cam_offs_dev, int32_t n_scenes,
                        int32_t n_cams, int32_t seed_a, int32_t seed_b, int32_t seed_c,
                        int32_t *counts_dev, mvm_stream_t stream);
int mvm_leftover_gather(const int32_t *used_dev, const double *pts_dev, const int32_t *boxes_dev,
                        const int64_t *cam_offs_dev, const int64_t *sub_cam_offs_dev, int32_t n_scenes,
                        int32_t n_cams, int32_t seed_a, int32_t seed_b, int32_t seed_c,
                        double *pts_out_dev, int32_t *boxes_out_dev, int32_t *orig_out_dev,
                        mvm_stream_t stream);

/*
 * Refinement of triangulated points by reprojection error, with covariance,
 * for a C-camera batch, 3 <= C <= MVM_MAX_CAMS (an addition to ABI 8,
 * announced by MVM_HAS_REFINE).  Inputs, none written:
 * views_dev int32 [.., C] (a three-camera batch passes its match array) and
 * X_dev f64 [.., 3] with capture s's count_dev[s] matches at rows
 * match_offs_dev[s] + w (never more rows than match_offs[s+1] - match_offs[s]);
 * pts_dev / cam_offs_dev the C-camera CSR, proj_dev f64 [S, C, 3, 4].
 * For match w the kept set is K = {d < C : views[w][d] >= 0}, ascending.  From
 * X the summed squared reprojection error over K is minimised by damped
 * Gauss-Newton steps: the normal matrix A and gradient g of the residuals
 * (u - cx, v - cy), (A + lambda diag A) delta = -g solved by a 3 x 3 LDL^T,
 * a step taken only where it lowers the cost (lambda / 10, floor 1e-15;
 * else lambda * 10; lambda starts at 1e-3), until
 * delta.delta <= 1e-20 X.X or max_evals (1..64) trial costs were evaluated.
 * Every operation and its order are stated by tests/refine_model.py, whose
 * bits the kernel returns.  Outputs per row:
 *   X_out_dev f64 [.., 3]   the refined point (never a higher cost than X);
 *   rms_dev   f64 [.., 2]   sqrt(cost / |K|) at X and at X_out, pixels;
 *   info_dev  int32 [.., 2] (status, trial costs evaluated); status 0:
 *             converged, 1: stopped at max_evals, 2: a non-finite cost, A, g or
 *             delta, or a pivot that is not > 0 (X_out = X), 3: skipped, since
 *             |K| < 2 or an entry of K is no detection of its view (X_out = X,
 *             rms and cov NaN): no index is used unchecked;
 *   cov_dev   f64 [.., 6]   may be NULL; the upper triangle, row-major, of the
 *             inverse of the undamped A at X_out (mm^2 / px^2: times the
 *             caller's pixel variance), NaN where a pivot is not > 0.
 * Status 2 after accepted steps undoes them: X_out = X, rms[1] = rms[0], cov
 * is that of the A at X, and the count keeps the trial costs evaluated until
 * then.  Status 1 met after rejected steps returns the last accepted point
 * with the count at max_evals.
 * Only the count_dev[s] rows of every capture are written.  X_out_dev must not
 * overlap X_dev.  One launch on `stream`, a wave per capture; no allocation,
 * copy or synchronisation.  n_scenes == 0 launches nothing.  A NULL pointer
 * other than cov_dev, n_cams outside 3..MVM_MAX_CAMS or max_evals outside
 * 1..64 is refused before the launch.
 */
int mvm_refine_points(const int64_t *match_offs_dev, const int32_t *count_dev, int32_t n_scenes,
                      int32_t n_cams, const double *pts_dev, const int64_t *cam_offs_dev,
                      const double *proj_dev, const int32_t *views_dev, const double *X_dev,
                      int32_t max_evals, double *X_out_dev, double *rms_dev, int32_t *info_dev,
                      double *cov_dev, mvm_stream_t stream);

/*
 * The pose head's input crops of every match view (an addition to ABI 8,
 * announced by MVM_HAS_CROPS).  Inputs, none written:
 *   images_dev uint8 [n_scenes * n_cams, img_h, img_w, 3], contiguous, channel
 *              order B, G, R; image (s, c) at index s * n_cams + c;
 *   scene_dev  int32 [>= row0 + n_rows], views_dev int32 [.., n_cams] and
 *              boxes_dev int32 [.., n_cams, 4] (x1, y1, x2, y2): a match
 *              table's scene, views (a three-camera table passes its match
 *              array) and boxes;
 *   cams_host  n_sel cameras < n_cams on the host, copied into the kernel's
 *              arguments (never dereferenced on the device);
 *   lut_dev    float32 [3, 256] (out_kind 0) or float16 [3, 256] (out_kind 1):
 *              plane c's value of level v, planes in R, G, B order.
 * A slot is (row r of the n_rows rows from row0, k-th selected camera c).  Its
 * box is clipped to the image: xa = min(max(x1, 0), img_w), xb, ya, yb alike,
 * w = xb - xa, h = yb - ya.  With scale = double(size) / max(h, w):
 * new_w = max(1, rint(w * scale)), new_h alike (fp64, ties to even).  The w x h
 * crop is resampled to new_w x new_h by the exact box integral: destination
 * pixel (X, Y) weighs source pixel (i, j) by ox * oy, ox the integer overlap
 * of [X w, (X + 1) w) with [i new_w, (i + 1) new_w), oy alike; the level is
 * (2 s + w h) / (2 w h) rounded down, s the weighted sum, in integers (32-bit
 * while 2 * 255 * w * h < 2^32, else 64-bit: the same value).  The result sits
 * at ((size - new_h) / 2, (size - new_w) / 2) of a size x size canvas of
 * `fill`, and out[c][y][x] = lut[c][canvas[y][x][2 - c]].  tests/crop_model.py
 * states every step; the kernel returns its bits.  Outputs per slot:
 *   out_dev  [n_rows, n_sel, 3, size, size] of the table's element type;
 *   geom_dev int32 [n_rows, n_sel, 8], may be NULL: (status, xa, ya, w, h,
 *            new_w, new_h, image index).  Status 0: crop made; 1: made from a
 *            clipped box; 2: empty after clipping; 3: no view (views < 0); 4:
 *            scene - scene_base is no index < n_scenes (checked first).  For 2,
 *            3 and 4 the canvas is all fill, the fields after the status are 0
 *            (the image index -1 for status 4) and no image byte is read; no
 *            entry of views is used as an index.
 * Every slot of the range is written whole, nothing else.  One launch on
 * `stream`; no allocation, copy or synchronisation.  n_rows == 0 is MVM_OK
 * whatever the other arguments are.  Refused before the launch: a NULL pointer
 * other than geom_dev; n_cams outside 3..MVM_MAX_CAMS; n_sel outside 1..n_cams
 * or a camera >= n_cams; size outside 1..1024; img_h or img_w outside 1..16384;
 * fill outside 0..255; out_kind other than 0 or 1; a negative row0, n_rows or
 * n_scenes; more slots than one launch holds (split the rows).
 */
int mvm_crop_views(const uint8_t *images_dev, int32_t n_scenes, int32_t n_cams, int32_t img_h,
                   int32_t img_w, const int32_t *scene_dev, int32_t scene_base,
                   const int32_t *views_dev, const int32_t *boxes_dev, int64_t row0, int64_t n_rows,
                   const int32_t *cams_host, int32_t n_sel, int32_t size, int32_t fill,
                   const void *lut_dev, int32_t out_kind, void *out_dev, int32_t *geom_dev,
                   mvm_stream_t stream);

/*
 * From the rotation head's raw outputs to a pose per match (an addition to
 * ABI 8, announced by MVM_HAS_POSES).  Inputs, none
 * written:
 *   raw_dev    float32 [n_rows, n_sel, D]: the head's output per slot; D = 3
 *              (mode 0, Euler angles in radians), 4 (mode 1, quaternion x, y,
 *              z, w) or 6 (mode 2, the 6-D representation);
 *   scene_dev  int32 [>= row0 + n_rows], views_dev int32 [.., n_cams] and X_dev
 *              f64 [.., 3]: a match table's scene, views (a three-camera table
 *              passes its match array) and X;
 *   RTs_dev    f64 [n_scenes, n_cams, 4, 4]: world -> camera;
 *   cams_host  n_sel cameras < n_cams on the host, copied into the kernel's
 *              arguments (never dereferenced on the device).
 * A slot is (row r of the n_rows rows from row0, k-th selected camera c).  Its
 * raw vector is decoded in float32 as the reference decodes it: mode 0 wraps
 * each angle to ((a + pi) mod 2 pi) - pi, takes the float64 sine and cosine
 * rounded once and forms rotmat_from_euler's entries; mode 1 divides by
 * (norm + 1e-8), then by the norm, and forms quat_to_rotmat's entries; mode 2
 * is rotmat_from_6d's Gram-Schmidt step with norms clamped at 1e-8.  The
 * float32 matrix M goes to the world in float64: W = RTs[s][c][:3][:3]^T M.
 * Slot status: 2 where scene - scene_base is no index < n_scenes (checked
 * first), 1 where views < 0, 4 where M has a non-finite entry (a zero
 * quaternion, a NaN or infinite input) or W an entry that is not below 2^500
 * in magnitude (a NaN, an infinity or an absurd value in the extrinsic
 * rotation), else 0.  So R is NaN only for row status 1 and
 * rot_views only where the slot's status is not 0, whatever RTs holds.  A row
 * is fused over its slots of status 0, in the order of cams_host:
 *   fuse 0  the rotation of camera fuse_cam, which must be selected; row
 *           status 1 where that slot's status is not 0;
 *   fuse 1  the chordal mean: the rotation nearest the sum of the W, as the
 *           largest eigenvector of Horn's symmetric 4 x 4 matrix (8 sweeps of
 *           cyclic Jacobi rotations and one shifted power step, float64); row
 *           status 1 where no slot is usable, 2 where the two largest
 *           eigenvalues differ by no more than 1e-9 times the usable slots (for
 *           example two views half a turn apart; R is still written).
 * tests/pose_model.py states every step; the kernel returns its bits.  Outputs
 * per row or slot of the range:
 *   rot_views_dev   f64 [n_rows, n_sel, 3, 3], may be NULL: W, NaN where the
 *                   slot's status is not 0;
 *   R_dev           f64 [n_rows, 3, 3]: the fused rotation, NaN for row status 1;
 *   pose_dev        f64 [n_rows, 4, 4]: [[R, X], [0, 0, 0, 1]];
 *   spread_dev      f64 [n_rows, n_sel], may be NULL: the squared Frobenius
 *                   distance of W to R (0 .. 8), NaN where either is NaN;
 *   slot_status_dev int32 [n_rows, n_sel]; row_status_dev int32 [n_rows].
 * No entry of views is used as an index.  One launch on `stream`, a thread per
 * row; no allocation, copy or synchronisation.  n_rows == 0 is MVM_OK whatever
 * the other arguments are.  Refused before the launch: a NULL pointer other
 * than rot_views_dev and spread_dev; n_cams outside 3..MVM_MAX_CAMS; n_sel
 * outside 1..n_cams or a camera >= n_cams; a mode or fuse not listed; D that
 * is not the mode's; fuse 0 with fuse_cam not selected; a negative row0,
 * n_rows or n_scenes.
 */
int mvm_fuse_rotations(const float *raw_dev, int32_t D, const int32_t *scene_dev, int32_t scene_base,
                       const int32_t *views_dev, const double *X_dev, const double *RTs_dev,
                       int32_t n_scenes, int32_t n_cams, int64_t row0, int64_t n_rows,
                       const int32_t *cams_host, int32_t n_sel, int32_t mode, int32_t fuse,
                       int32_t fuse_cam, double *rot_views_dev, double *R_dev, double *pose_dev,
                       double *spread_dev, int32_t *slot_status_dev, int32_t *row_status_dev,
                       mvm_stream_t stream);

/*
 * Poses against ground truth (additions to ABI 8, announced by
 * MVM_HAS_SCORES).  tests/score_model.py states every
 * step of both; the kernels return its bits.
 *
 * mvm_score_poses: the BOP pose error MSSD (maximum symmetry-aware surface
 * distance) of every (estimate, ground-truth object) pair of a capture.
 * Inputs, none written:
 *   pose_dev     f64 [>= row0 + n_rows, 4, 4] and scene_dev int32 [same]: the
 *                estimates in the world frame and each one's capture id;
 *   gt_pose_dev  f64 [G, 4, 4]: the ground-truth poses in the world frame;
 *   gt_offs_dev  int64 [n_scenes + 1]: capture s owns ground-truth rows
 *                gt_offs[s] : gt_offs[s + 1] (non-decreasing, within 0 .. G: it
 *                is trusted as every offset table here is);
 *   verts_dev    f64 [n_verts, 3] and syms_dev f64 [n_syms, 4, 4]: the model's
 *                vertices and its symmetry transforms, finite and below 2^200
 *                in magnitude.
 * Only the top three rows of a pose or a symmetry are read.  For row r of the
 * n_rows rows from row0, s = scene - scene_base, and column g < g_max, each
 * rule applying only where the one before did not:
 *   s is no index < n_scenes     err = t_err = +inf, rot_cos = NaN, sym = -2;
 *   g >= capture s's row count   the same with sym = -1 (padding);
 *   one of the 12 read entries of either pose is not below 2^200 in magnitude
 *   (a NaN is not)               the same with sym = -3;
 *   otherwise, with (Rp, tp) the estimate, (Rg, tg) the ground truth and
 *   (Sk, sk) symmetry k: M = Rg Sk, A = Rp - M, b = tp - (Rg sk + tg),
 *   m_k = max over the vertices v of |A v + b|^2; sym = the lowest k with the
 *   smallest m_k, err = sqrt(m_sym), t_err = |tp - tg|, rot_cos =
 *   (sum_ij Rp_ij M_sym_ij - 1) / 2 (the cosine of the rotation between the
 *   two; its arccosine is the caller's).  Products, sums and square roots are
 *   single float64 operations in the model's order, nothing contracted.
 * Outputs, [n_rows, g_max] each, every entry written: err_dev f64, sym_dev
 * int32, t_err_dev f64 (may be NULL) and rot_cos_dev f64 (may be NULL).  One
 * launch on `stream`, a thread per pair; no allocation, copy or
 * synchronisation.  n_rows == 0 is MVM_OK whatever the other arguments are.
 * Refused before the launch: a NULL pointer other than t_err_dev and
 * rot_cos_dev; n_syms outside 1..64; n_verts < 1; g_max < 1; a negative row0,
 * n_rows or n_scenes; more pairs than one grid holds (n_rows g_max >= 2^32:
 * split the rows).
 */
int mvm_score_poses(const double *pose_dev, const int32_t *scene_dev, int32_t scene_base,
                    const double *gt_pose_dev, const int64_t *gt_offs_dev, int32_t n_scenes,
                    int32_t g_max, const double *verts_dev, int32_t n_verts, const double *syms_dev,
                    int32_t n_syms, int64_t row0, int64_t n_rows, double *err_dev, int32_t *sym_dev,
                    double *t_err_dev /* may be NULL */, double *rot_cos_dev /* may be NULL */,
                    mvm_stream_t stream);

/*
 * mvm_match_scores: the greedy matching of each capture's rows to its ground
 * truth, once per threshold.  Inputs, none written:
 *   err_dev          f64 [n_rows_total, g_max]: mvm_score_poses's err over the
 *                    whole table;
 *   row_offs_dev     int64 [n_scenes + 1]: capture s owns table rows
 *                    row_offs[s] : row_offs[s + 1] (non-decreasing);
 *   gt_offs_dev      int64 [n_scenes + 1]: as above; only the counts are read;
 *   thresholds_host  n_thresholds values on the host, copied into the kernel's
 *                    arguments (never dereferenced on the device).
 * For threshold t and capture s the rows are walked in table order; row r takes
 * the not-yet-taken g < min(count of s, g_max) with the smallest err[r][g]
 * among those with err[r][g] < thresholds[t] (strict; the lowest g wins a tie),
 * or -1.  +inf and NaN never match.  Outputs:
 *   gt_index_dev  int32 [n_thresholds, n_rows_total]: the g taken, or -1; the
 *                 rows no capture owns are written -1 by the same launch;
 *   tp_dev        int32 [n_thresholds, n_scenes]: the rows of s that took one.
 * Every offset read from row_offs is clamped into 0 .. n_rows_total (and an
 * end below its begin up to it) before a row is touched, and a count into
 * 0 .. g_max.  One launch on `stream`, a wave per (capture, threshold); no
 * allocation, copy or synchronisation.  n_scenes == 0 with n_rows_total == 0 is
 * MVM_OK whatever the other arguments are.  Refused before the launch: g_max
 * outside 1..1024 (MVM_ERR_UNSUPPORTED); n_thresholds outside 1..16; a
 * negative n_scenes or n_rows_total; a NULL pointer that would be read or
 * written (err_dev and gt_index_dev may be NULL without rows, row_offs_dev,
 * gt_offs_dev and tp_dev without captures).
 */
int mvm_match_scores(const double *err_dev, int32_t g_max, const int64_t *row_offs_dev,
                     const int64_t *gt_offs_dev, int32_t n_scenes, const double *thresholds_host,
                     int32_t n_thresholds, int32_t *gt_index_dev, int32_t *tp_dev,
                     int64_t n_rows_total, mvm_stream_t stream);

/*
 * The chordal mean of a row's views under the object's symmetries (an addition
 * to ABI 8, announced by MVM_HAS_SYM_FUSE).  A head that
 * sees a symmetric part may answer, per view, any of the rotations R S_k that
 * look alike from there; mvm_fuse_rotations' mean of such views is none of
 * them.  Here every view is first multiplied by the symmetry that takes it
 * nearest a reference, and the mean is taken of the aligned views.
 * raw_dev .. mode are mvm_fuse_rotations' arguments and mean the same: slots,
 * decoding, W = RTs[s][c][:3][:3]^T M and the slot statuses 1, 2 and 4.
 *   syms_dev  f64 [n_syms, 4, 4]: the symmetry transforms as mvm_score_poses
 *             takes them; only the top-left 3 x 3 block S_k of each is read.
 *             Any length from 1 (a discretised continuous symmetry is long);
 *   rounds    1..4 (2 is the usual choice).
 * Per row, with its slots in the order of cams_host:
 *   1. the reference R_ref is the W of the first slot of status 0; a row
 *      without one has row status 1;
 *   2. per slot of status 0: B = R_ref^T W, s_k = sum_ij B_ij S_k,ji (the trace
 *      of B S_k; (i, j) row-major, left to right) for k ascending; s_k > best (from -inf) moves best to
 *      second and takes k, else s_k > second replaces second: the lowest index
 *      wins a tie and a NaN is never taken.  W' = W S_k.  A slot where no k was
 *      taken, or whose W' has an entry that is not below 2^500 in magnitude,
 *      gets slot status 8 and is not used again;
 *   3. R = the chordal mean of the W' of the slots still of status 0, exactly
 *      as mvm_fuse_rotations' fuse 1 takes it; a row that has lost every slot
 *      has row status 1;
 *   4. steps 2 and 3 again with R_ref = R, `rounds` times in all: the first
 *      round is aligned to one view, the later ones to the mean of all.
 * tests/pose_sym_model.py states every step; the kernel returns its bits.
 * With the identity as the only symmetry every output shared with
 * mvm_fuse_rotations' fuse 1 equals it as a number.  Outputs per row or slot:
 *   rot_views_dev   f64 [n_rows, n_sel, 3, 3], may be NULL: W' of the last
 *                   round, NaN where the slot's status is not 0;
 *   R_dev, pose_dev, row_status_dev: as mvm_fuse_rotations writes them; row
 *                   status 2 by the eigenvalue gap of the last mean;
 *   spread_dev      f64 [n_rows, n_sel], may be NULL: the squared Frobenius
 *                   distance of W' to R, NaN where the slot's status is not 0;
 *   slot_status_dev int32 [n_rows, n_sel]: 0, 1, 2, 4 or 8;
 *   sym_index_dev   int32 [n_rows, n_sel]: the k of the last round, -1 where
 *                   the slot's status is not 0;
 *   sym_margin_dev  f64 [n_rows, n_sel], may be NULL: best - second of the last
 *                   round (+inf where one score was taken), NaN where the
 *                   slot's status is not 0: small for a view that sits between
 *                   two symmetry elements;
 *   n_changed_dev   int32 [n_rows], may be NULL: the slots of status 0 whose k
 *                   of the last round is not that of the round before (0 for
 *                   rounds 1, 0 once converged).
 * slot_status_dev and sym_index_dev also carry a row's state from round to
 * round: each thread reads back what it wrote.  One launch on `stream`, a
 * thread per row; no allocation, copy or synchronisation.  n_rows == 0 is
 * MVM_OK whatever the other arguments are.  Refused before the launch:
 * everything mvm_fuse_rotations refuses of the shared arguments; n_syms < 1;
 * rounds outside 1..4; a NULL pointer other than rot_views_dev, spread_dev,
 * sym_margin_dev and n_changed_dev.
 */
int mvm_fuse_rotations_sym(const float *raw_dev, int32_t D, const int32_t *scene_dev, int32_t scene_base,
                           const int32_t *views_dev, const double *X_dev, const double *RTs_dev,
                           int32_t n_scenes, int32_t n_cams, int64_t row0, int64_t n_rows,
                           const int32_t *cams_host, int32_t n_sel, int32_t mode, const double *syms_dev,
                           int32_t n_syms, int32_t rounds, double *rot_views_dev /* may be NULL */,
                           double *R_dev, double *pose_dev, double *spread_dev /* may be NULL */,
                           int32_t *slot_status_dev, int32_t *row_status_dev, int32_t *sym_index_dev,
                           double *sym_margin_dev /* may be NULL */, int32_t *n_changed_dev /* may be NULL */,
                           mvm_stream_t stream);

/*
 * The translation of a pose fitted to the detected boxes, given the model (an
 * addition to ABI 8, announced by MVM_HAS_BOX_FIT).  The
 * table's X is the triangulation of the views' box centres, and a box centre
 * is not the projection of the object's origin; with the rotation known, the
 * box extents say where the origin is.  Inputs, none written, row w of n_rows:
 *   pose_dev  f64 [n_rows, 4, 4]: R = pose[w][:3][:3] (for example
 *             mvm_fuse_rotations' pose_dev) and the start t0 = pose[w][:3][3];
 *   scene_dev int32 [n_rows], scene_base: s = scene[w] - scene_base;
 *   views_dev int32 [n_rows, n_cams] (a three-camera table passes its match
 *             array): the kept set is K = {d < n_cams : views[w][d] >= 0},
 *             ascending.  Only the sign is read;
 *   boxes_dev int32 [n_rows, n_cams, 4]: (x1, y1, x2, y2) of every view;
 *   proj_dev  f64 [n_scenes, n_cams, 3, 4], row-major;
 *   verts_dev f64 [n_verts, 3]: the model's vertices in the object's frame.
 * Per view of K and point t the vertices are projected, h = P[:, :3] R v +
 * (P[:, :3] t + P[:, 3]), u = h0 / h2, v = h1 / h2, and their extremes umin,
 * vmin, umax, vmax are taken (strict compares in ascending vertex order: the
 * lowest vertex wins a tie), each with its vertex's depth h2.  The residuals
 * are (umin - x1, vmin - y1, umax - x2, vmax - y2), the cost their summed
 * squares over K, +inf where some vertex's h2 is not > 0.  An edge's row of the
 * Jacobian is that of its extreme vertex, (P[q][j] - p P[2][j]) / h2.  From t0
 * the cost is minimised by mvm_refine_points' damped Gauss-Newton steps and
 * loop (lambda from 1e-3, factors of 10, floor 1e-15, a step taken only where
 * it lowers the cost, until delta.delta <= 1e-20 t.t or max_evals (1..64) trial
 * costs were evaluated).  Every operation and its order are stated by
 * tests/box_fit_model.py, whose bits the kernel returns.  Outputs per row:
 *   pose_out_dev f64 [n_rows, 4, 4]  the input pose with the fitted t (never a
 *                higher cost than t0); R and the bottom row bit for bit;
 *   rms_dev      f64 [n_rows, 2]     sqrt(cost / (4 |K|)) at t0 and at the
 *                result, pixels;
 *   info_dev     int32 [n_rows, 2]   (status, trial costs evaluated); status
 *                0: converged, 1: stopped at max_evals, 2: a non-finite cost
 *                (a vertex behind a camera at t0), A, g or delta, or a pivot
 *                that is not > 0 (the result is t0, as for mvm_refine_points),
 *                3: skipped, since s is no capture of proj_dev or K is empty
 *                (pose_out = pose; rms, cov and resid NaN).  One view is
 *                enough: four edges constrain three unknowns;
 *   cov_dev      f64 [n_rows, 6]     may be NULL; the upper triangle,
 *                row-major, of the inverse of the undamped A at the result,
 *                NaN where a pivot is not > 0;
 *   resid_dev    f64 [n_rows, n_cams, 4]  may be NULL; the four residuals at
 *                the result, NaN in the views outside K.
 * One launch on `stream`, a wave per row; no allocation, copy or
 * synchronisation.  n_rows == 0 is MVM_OK whatever the other arguments are.
 * Refused before the launch: a NULL pointer other than cov_dev and resid_dev,
 * n_cams outside 3..MVM_MAX_CAMS, n_verts < 1, max_evals outside 1..64, a
 * negative n_rows or n_scenes, and pose_out_dev overlapping pose_dev.
 */
int mvm_fit_boxes(const double *pose_dev, const int32_t *scene_dev, int32_t scene_base,
                  const int32_t *views_dev, const int32_t *boxes_dev, int64_t n_rows, int32_t n_cams,
                  const double *proj_dev, int32_t n_scenes, const double *verts_dev, int32_t n_verts,
                  int32_t max_evals, double *pose_out_dev, double *rms_dev, int32_t *info_dev,
                  double *cov_dev /* may be NULL */, double *resid_dev /* may be NULL */,
                  mvm_stream_t stream);

/*
 * Diagnostic: fill `bytes` (multiple of 16, 16-byte aligned) of device memory
 * with the fastest 16-byte nontemporal store stream measured on MI355X: 8 KiB
 * per workgroup, workgroups remapped so each XCD writes its own contiguous
 * eighth in order.  bench.py times it to report the achievable HBM write
 * bandwidth next to the kernels' roofline fraction (the other store patterns
 * studied in DESIGN.md §3.5 live in tools/probes/write_probes.hip).
 */
int mvm_hbm_write_probe(void *dst_dev, size_t bytes, mvm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MVMATCH_H */
