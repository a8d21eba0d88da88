// mvm_wave.h — the one place wave (64-lane) reductions are spelled.  Device
// only; internal to the library.  The scheme: four DPP steps reduce each
// 16-lane row in registers (quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror), then the four row results are read with
// v_readlane (lanes 0, 16, 32, 48) and combined on the scalar unit.  No LDS
// round trips (a shuffle is a bpermute).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

// ---- words: the value of the lane DPP control CTRL selects, of lane l, of
// the first active lane (both uniform).  A double moves lo word, then hi.
template <int CTRL>
__device__ __forceinline__ int32_t dpp_mov(int32_t x) {
    return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t x) { return (uint32_t)dpp_mov<CTRL>((int32_t)x); }
__device__ __forceinline__ int32_t read_lane(int32_t x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ uint32_t read_lane(uint32_t x, int l) { return (uint32_t)read_lane((int32_t)x, l); }
__device__ __forceinline__ float first_lane(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

__device__ __forceinline__ uint32_t f64_lo(double x) { return (uint32_t)(uint64_t)__double_as_longlong(x); }
__device__ __forceinline__ uint32_t f64_hi(double x) { return (uint32_t)((uint64_t)__double_as_longlong(x) >> 32); }
__device__ __forceinline__ double f64_of(uint32_t lo, uint32_t hi) {
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double x) {
    const uint32_t lo = dpp_mov<CTRL>(f64_lo(x)), hi = dpp_mov<CTRL>(f64_hi(x));
    return f64_of(lo, hi);
}
__device__ __forceinline__ double read_lane(double x, int l) {
    const uint32_t lo = read_lane(f64_lo(x), l), hi = read_lane(f64_hi(x), l);
    return f64_of(lo, hi);
}
__device__ __forceinline__ double first_lane(double x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)f64_lo(x));
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)f64_hi(x));
    return f64_of(lo, hi);
}

// ---- records.  A record type R moves itself:
//   template <int CTRL> static R dpp(const R &r);   r of the lane CTRL selects
//   static R lane(const R &r, int l);                r of lane l, uniform
// and combine(a, b) is commutative and associative.  One DPP step (r by
// value: the form the kernels were tuned with), then the whole wave, uniform.
template <int CTRL, typename R, typename F>
__device__ __forceinline__ R wave_reduce_step(R r, F combine) {
    return combine(r, R::template dpp<CTRL>(r));
}
template <typename R, typename F>
__device__ __forceinline__ R wave_reduce(R r, F combine) {
    r = wave_reduce_step<0xB1>(r, combine);
    r = wave_reduce_step<0x4E>(r, combine);
    r = wave_reduce_step<0x141>(r, combine);
    r = wave_reduce_step<0x140>(r, combine);
    R a = R::lane(r, 0);
    a = combine(a, R::lane(r, 16));
    a = combine(a, R::lane(r, 32));
    return combine(a, R::lane(r, 48));
}

// ---- scalars: the same steps, the four rows combined pairwise.
template <typename T, typename F>
__device__ __forceinline__ T wave_reduce_word(T x, F op) {
    x = op(x, dpp_mov<0xB1>(x));
    x = op(x, dpp_mov<0x4E>(x));
    x = op(x, dpp_mov<0x141>(x));
    x = op(x, dpp_mov<0x140>(x));
    return op(op(read_lane(x, 0), read_lane(x, 16)), op(read_lane(x, 32), read_lane(x, 48)));
}
__device__ __forceinline__ double wave_min_f64(double x) {   // values are never NaN
    return wave_reduce_word(x, [](double a, double b) { return fmin(a, b); });
}
__device__ __forceinline__ int32_t wave_min_i32(int32_t x) {
    return wave_reduce_word(x, [](int32_t a, int32_t b) { return min(a, b); });
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
    return wave_reduce_word(x, [](uint32_t a, uint32_t b) { return max(a, b); });
}

// The unsigned minimum keeps a move of its own: old = UINT_MAX (its identity),
// not old = x, lets the DPP-combine pass fold the move into v_min_u32_dpp.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_from(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_min(uint32_t v) {
    const uint32_t o = dpp_from<CTRL>(v);
    return o < v ? o : v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    const auto umin = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    v = dpp_min<0xB1>(v);
    v = dpp_min<0x4E>(v);
    v = dpp_min<0x141>(v);
    v = dpp_min<0x140>(v);
    return umin(umin(read_lane(v, 0), read_lane(v, 16)), umin(read_lane(v, 32), read_lane(v, 48)));
}

}  // namespace
