// mvm_crops.hip — the pose head's input crops of every match view (DESIGN
// §3.18): per (table row, selected camera) slot, the row's box in that camera
// clipped to the image, area-resampled onto a size x size canvas of `fill`
// with exact integer weights, and every level sent through a 3 x 256 table
// (BGR -> RGB planes, scale and normalise in one look-up).  Every step and its
// order are stated by tests/crop_model.py, whose bits the kernel returns.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "mvmatch.h"
#include "mvm_device.h"
#include "mvm_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int kCropIters = 4;        // pixel groups a thread walks: one workgroup's share of a canvas
constexpr int kCropMaxSize = 1024;   // canvas side
constexpr int kCropMaxImage = 16384; // image side

enum : int32_t { kCropOk = 0, kCropClipped = 1, kCropEmpty = 2, kCropNoView = 3, kCropNoScene = 4 };

// One slot's geometry: the same in every lane (scalar registers).
struct CropGeom {
    int32_t status, xa, ya, w, h, new_w, new_h, image;
    int32_t dx, dy;
};

__device__ __forceinline__ int32_t clamp_to(int32_t v, int32_t hi) { return min(max(v, 0), hi); }

// max(1, rint(side * (T / longest))) in fp64: Python's round() of the double product
__device__ __forceinline__ int32_t scaled_side(int32_t side, double scale) {
    return max(1, (int32_t)__builtin_rint((double)side * scale));
}

// floor(n / d) for n / d < 256: a float32 estimate (off by one at the most:
// both conversions and the division are within 2^-23 relative of a quotient
// below 256) put right against the exact products
template <typename Acc>
__device__ __forceinline__ uint32_t exact_level(Acc n, Acc d) {
    uint32_t q = (uint32_t)((float)n / (float)d);
    while ((Acc)q * d > n) --q;
    while ((Acc)(q + 1) * d <= n) ++q;
    return q;
}

// The three levels (source channel order) of canvas pixel (X, Y) of the placed
// rectangle: the box integral of the crop over the pixel's footprint, in units
// of 1 / (new_w new_h) source pixels, rounded half up.
//   (2 s + w h) // (2 w h) == (s + (w h) // 2) // (w h)  for either parity of w h
template <typename Acc>
__device__ __forceinline__ void area_levels(const uint8_t *__restrict__ src, int64_t pitch, const CropGeom &g,
                                            int32_t X, int32_t Y, uint32_t lv[3]) {
    const int32_t x_lo = X * g.w, x_hi = x_lo + g.w;      // < 2^24 + 2^14
    const int32_t y_lo = Y * g.h, y_hi = y_lo + g.h;
    const int32_t i0 = x_lo / g.new_w, i1 = (x_hi - 1) / g.new_w;
    const int32_t j0 = y_lo / g.new_h, j1 = (y_hi - 1) / g.new_h;
    Acc s0 = 0, s1 = 0, s2 = 0;
    for (int32_t j = j0; j <= j1; ++j) {
        const uint32_t oy = (uint32_t)(min(y_hi, (j + 1) * g.new_h) - max(y_lo, j * g.new_h));
        const uint8_t *row = src + (int64_t)j * pitch;
        uint32_t r0 = 0, r1 = 0, r2 = 0;                  // a row's share: <= 255 w < 2^22
        for (int32_t i = i0; i <= i1; ++i) {
            const uint32_t ox = (uint32_t)(min(x_hi, (i + 1) * g.new_w) - max(x_lo, i * g.new_w));
            const uint8_t *p = row + 3 * i;
            r0 += ox * p[0];
            r1 += ox * p[1];
            r2 += ox * p[2];
        }
        s0 += (Acc)oy * r0;
        s1 += (Acc)oy * r1;
        s2 += (Acc)oy * r2;
    }
    const Acc area = (Acc)g.w * (Acc)g.h, half = area / 2;
    lv[0] = exact_level<Acc>(s0 + half, area);
    lv[1] = exact_level<Acc>(s1 + half, area);
    lv[2] = exact_level<Acc>(s2 + half, area);
}

// Workgroup = 256 threads owning kCropIters * 256 * PIX consecutive pixels
// (y T + x) of one slot's canvas; a thread owns PIX consecutive ones per step
// and writes them to each of the three planes with one store, consecutive
// lanes at consecutive addresses.  PIX 4: 16-byte (float32) or 8-byte
// (float16) nontemporal stores, taken when every plane starts on such a
// boundary; PIX 1: element stores.  E is the raw element (the table is only
// copied).  The slot's scene, view, box, clip and sizes come from the block
// index alone: uniform loads and scalar arithmetic.  The table sits in LDS.
template <typename E, int PIX>
__global__ __launch_bounds__(kThreads) void crop_views_kernel(
    const uint8_t *__restrict__ images, int32_t n_scenes, int32_t n_cams, int32_t img_h, int32_t img_w,
    const int32_t *__restrict__ scene, int32_t scene_base, const int32_t *__restrict__ views,
    const int32_t *__restrict__ boxes, int64_t row0, uint32_t cams_packed, int32_t n_sel, int32_t T,
    int32_t fill, const E *__restrict__ lut, uint32_t blocks_per_slot, E *__restrict__ out,
    int32_t *__restrict__ geom) {
    __shared__ E s_lut[3 * 256];
    for (int t = threadIdx.x; t < 3 * 256; t += kThreads) s_lut[t] = lut[t];

    const uint32_t slot = blockIdx.x / blocks_per_slot;
    const uint32_t part = blockIdx.x - slot * blocks_per_slot;
    const uint32_t r = slot / (uint32_t)n_sel, k = slot - r * (uint32_t)n_sel;
    const int32_t cam = (int32_t)((cams_packed >> (4 * k)) & 15u);
    const int64_t row = row0 + r;

    CropGeom g = {};
    const int64_t sc = (int64_t)scene[row] - scene_base;
    if (sc < 0 || sc >= n_scenes) {
        g.status = kCropNoScene;
        g.image = -1;
    } else if (views[row * n_cams + cam] < 0) {
        g.status = kCropNoView;
    } else {
        const int32_t *b = boxes + (row * n_cams + cam) * 4;
        const int32_t x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
        const int32_t xa = clamp_to(x1, img_w), xb = clamp_to(x2, img_w);
        const int32_t ya = clamp_to(y1, img_h), yb = clamp_to(y2, img_h);
        const int32_t w = xb - xa, h = yb - ya;
        if (w <= 0 || h <= 0) {
            g.status = kCropEmpty;
        } else {
            g.status = (xa != x1 || xb != x2 || ya != y1 || yb != y2) ? kCropClipped : kCropOk;
            const double scale = (double)T / (double)max(h, w);
            g.xa = xa, g.ya = ya, g.w = w, g.h = h;
            g.new_w = scaled_side(w, scale);
            g.new_h = scaled_side(h, scale);
            g.image = (int32_t)(sc * n_cams + cam);
            g.dx = (T - g.new_w) / 2;
            g.dy = (T - g.new_h) / 2;
        }
    }
    if (geom && part == 0 && threadIdx.x == 0) {
        int32_t *q = geom + (int64_t)slot * 8;
        q[0] = g.status, q[1] = g.xa, q[2] = g.ya, q[3] = g.w;
        q[4] = g.h, q[5] = g.new_w, q[6] = g.new_h, q[7] = g.image;
    }
    __syncthreads();

    const bool made = g.status <= kCropClipped;
    const int64_t pitch = (int64_t)img_w * 3;
    // the crop's first byte; an empty slot reads nothing
    const uint8_t *src = images + (made ? ((int64_t)g.image * img_h + g.ya) * pitch + (int64_t)g.xa * 3 : 0);
    const bool wide = made && 2ull * 255ull * (uint64_t)g.w * (uint64_t)g.h >= (1ull << 32);
    const E f0 = s_lut[fill], f1 = s_lut[256 + fill], f2 = s_lut[512 + fill];

    const uint32_t n_pix = (uint32_t)T * (uint32_t)T;
    E *planes = out + (int64_t)slot * 3 * n_pix;
    const uint32_t first = part * (uint32_t)(kCropIters * kThreads * PIX);
    for (int it = 0; it < kCropIters; ++it) {
        const uint32_t p0 = first + (uint32_t)(it * kThreads + (int)threadIdx.x) * PIX;
        if (p0 >= n_pix) break;
        E v0[PIX], v1[PIX], v2[PIX];
#pragma unroll
        for (int e = 0; e < PIX; ++e) {
            const uint32_t p = p0 + e;           // PIX 4: n_pix is a multiple of 4, so p < n_pix
            const int32_t y = (int32_t)(p / (uint32_t)T), x = (int32_t)(p - (uint32_t)y * (uint32_t)T);
            const int32_t X = x - g.dx, Y = y - g.dy;
            E a = f0, b = f1, c = f2;
            if (made && X >= 0 && X < g.new_w && Y >= 0 && Y < g.new_h) {
                uint32_t lv[3];
                if (wide)
                    area_levels<uint64_t>(src, pitch, g, X, Y, lv);
                else
                    area_levels<uint32_t>(src, pitch, g, X, Y, lv);
                a = s_lut[lv[2]], b = s_lut[256 + lv[1]], c = s_lut[512 + lv[0]];   // plane 0 is R
            }
            v0[e] = a, v1[e] = b, v2[e] = c;
        }
        if constexpr (PIX == 1) {
            planes[p0] = v0[0];
            planes[n_pix + p0] = v1[0];
            planes[2 * (int64_t)n_pix + p0] = v2[0];
        } else {
            typedef E V __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(V{v0[0], v0[1], v0[2], v0[3]}, reinterpret_cast<V *>(planes + p0));
            __builtin_nontemporal_store(V{v1[0], v1[1], v1[2], v1[3]}, reinterpret_cast<V *>(planes + n_pix + p0));
            __builtin_nontemporal_store(V{v2[0], v2[1], v2[2], v2[3]},
                                        reinterpret_cast<V *>(planes + 2 * (int64_t)n_pix + p0));
        }
    }
}

template <typename E, int PIX>
int launch_crops(const uint8_t *images, int32_t n_scenes, int32_t n_cams, int32_t img_h, int32_t img_w,
                 const int32_t *scene, int32_t scene_base, const int32_t *views, const int32_t *boxes,
                 int64_t row0, int64_t n_rows, uint32_t cams_packed, int32_t n_sel, int32_t size, int32_t fill,
                 const void *lut, void *out, int32_t *geom, mvm_stream_t stream) {
    const int64_t per_block = (int64_t)kCropIters * kThreads * PIX;
    const int64_t blocks_per_slot = ((int64_t)size * size + per_block - 1) / per_block;
    const int64_t grid = n_rows * n_sel * blocks_per_slot;
    if (grid > kMaxGridBlocks)
        return mvm_fail(MVM_ERR_UNSUPPORTED, "n_rows=%lld: more crops than one launch holds; split the rows",
                        (long long)n_rows);
    crop_views_kernel<E, PIX><<<(unsigned)grid, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        images, n_scenes, n_cams, img_h, img_w, scene, scene_base, views, boxes, row0, cams_packed, n_sel,
        size, fill, static_cast<const E *>(lut), (uint32_t)blocks_per_slot, static_cast<E *>(out), geom);
    return mvm_check_launch("crop_views_kernel");
}

}  // namespace

extern "C" {

int mvm_crop_views(const uint8_t *images_dev, int32_t n_scenes, int32_t n_cams, int32_t img_h, int32_t img_w,
                   const int32_t *scene_dev, int32_t scene_base, const int32_t *views_dev,
                   const int32_t *boxes_dev, int64_t row0, int64_t n_rows, const int32_t *cams_host,
                   int32_t n_sel, int32_t size, int32_t fill, const void *lut_dev, int32_t out_kind,
                   void *out_dev, int32_t *geom_dev, mvm_stream_t stream) {
    mvm_clear_error();
    if (n_rows == 0) return MVM_OK;
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
    if (size < 1 || size > kCropMaxSize)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "size=%d outside [1, %d]", size, kCropMaxSize);
    if (img_h < 1 || img_h > kCropMaxImage)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "img_h=%d outside [1, %d]", img_h, kCropMaxImage);
    if (img_w < 1 || img_w > kCropMaxImage)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "img_w=%d outside [1, %d]", img_w, kCropMaxImage);
    if (fill < 0 || fill > 255) return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "fill=%d outside [0, 255]", fill);
    if (out_kind != 0 && out_kind != 1)
        return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "out_kind=%d: 0 (float32) or 1 (float16)", out_kind);
    if (const int st = mvm_require_ptrs({{images_dev, "images_dev"},
                                         {scene_dev, "scene_dev"},
                                         {views_dev, "views_dev"},
                                         {boxes_dev, "boxes_dev"},
                                         {cams_host, "cams_host"},
                                         {lut_dev, "lut_dev"},
                                         {out_dev, "out_dev"}}))
        return st;                       // geom_dev may be NULL: no geometry is written
    uint32_t cams_packed = 0;
    for (int k = 0; k < n_sel; ++k) {
        if (cams_host[k] < 0 || cams_host[k] >= n_cams)
            return mvm_fail(MVM_ERR_INVALID_ARGUMENT, "cams_host[%d]=%d is no camera < %d", k, cams_host[k],
                            n_cams);
        cams_packed |= (uint32_t)cams_host[k] << (4 * k);
    }
    // a plane is size^2 elements: with an even size and an aligned base every
    // plane of every slot starts on a 4-element boundary
    const size_t elem = out_kind == 0 ? 4 : 2;
    const bool vec = size % 2 == 0 && (reinterpret_cast<uintptr_t>(out_dev) & (4 * elem - 1)) == 0;
#define MVM_CROPS(E, PIX)                                                                                   \
    launch_crops<E, PIX>(images_dev, n_scenes, n_cams, img_h, img_w, scene_dev, scene_base, views_dev,     \
                         boxes_dev, row0, n_rows, cams_packed, n_sel, size, fill, lut_dev, out_dev, geom_dev, \
                         stream)
    if (out_kind == 0) return vec ? MVM_CROPS(uint32_t, 4) : MVM_CROPS(uint32_t, 1);
    return vec ? MVM_CROPS(uint16_t, 4) : MVM_CROPS(uint16_t, 1);
#undef MVM_CROPS
}

}  // extern "C"
