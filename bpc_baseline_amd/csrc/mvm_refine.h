// mvm_refine.h — the 3 x 3 factorisation the damped Gauss-Newton kernels share
// (refine_points_kernel in mvm_pipeline.hip; fit_boxes_kernel in
// mvm_boxfit.hip): one statement of tests/refine_model.py's
// ``ldlt``.  Device only; internal to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool refine_finite(double x) { return __builtin_fabs(x) < INFINITY; }

// M = L D L^T of the symmetric M (upper triangle, row-major) in the model's
// order -> every pivot > 0 (a NaN is not); the factors mean nothing otherwise
struct RefineLdlt {
    double d0, d1, d2, l10, l20, l21;
};

__device__ __forceinline__ bool refine_ldlt(double M00, double M01, double M02, double M11,
                                            double M12, double M22, RefineLdlt &f) {
    f.d0 = M00;
    f.l10 = M01 / f.d0;
    f.l20 = M02 / f.d0;
    f.d1 = M11 - f.l10 * M01;
    const double t = M12 - f.l20 * M01;
    f.l21 = t / f.d1;
    f.d2 = (M22 - f.l20 * M02) - f.l21 * t;
    return f.d0 > 0.0 && f.d1 > 0.0 && f.d2 > 0.0;
}

}  // namespace
