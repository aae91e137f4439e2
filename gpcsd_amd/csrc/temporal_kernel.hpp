// The stationary temporal kernels, in one place: unit-variance value k(d; ell) and its ell-derivative per GPCSD_KIND_*.
// Every site that evaluates a temporal kernel on the device goes through these two templates (gram.hip: temporal_gram_kernel
// and tset_eval; grad.hip: temporal_grad_kernel; fisher.hip: temporal_dgram_kernel), so a kind exists everywhere or nowhere.
//
//   kind                  a              k                          dk / d ell
//   GPCSD_KIND_SE         --             exp(-d^2 / (2 ell^2))      k d^2 / ell^3
//   GPCSD_KIND_MATERN     |d| / ell      exp(-a)                    k |d| / ell^2
//   GPCSD_KIND_MATERN32   sqrt3 |d|/ell  (1 + a) exp(-a)            a^2 exp(-a) / ell
//   GPCSD_KIND_MATERN52   sqrt5 |d|/ell  (1 + a + a^2/3) exp(-a)    a^2 (1 + a) exp(-a) / (3 ell)
//
// The SE and Matern-1/2 branches are the expressions their sites have always had, operation for operation (the value-only form
// takes |d| as sqrt(d * d), as covariances.py:304 does; the form with the derivative takes fabs(d)): the results keep their bits.
// T = float is the fp32 Gram mode (gpcsd_set_gram_precision).
// The two new kinds take exp(-a) as h * h with h = exp(-a / 2), the polynomial multiplied into the first factor: where exp(-a)
// is subnormal (a > 708) its absolute rounding error would otherwise be multiplied by the polynomial (~ a, a^2 / 3); this way
// the only rounding in the subnormal range is the last product's.
//
// The kind is uniform per component, so the switch is wave-uniform.  It has NO default evaluation: the entry points reject a
// kind outside {SE, MATERN, MATERN32, MATERN52} before anything is launched (temporal_kind_on_device), and one that got
// through regardless comes out as NaN, never as some other kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <limits>

#include "../../include/gpcsd_hip.h"

namespace gpcsd {

// the kinds the device evaluates itself (GPCSD_KIND_HOST is the caller's Gram, never a kernel's)
__host__ __device__ inline bool temporal_kind_on_device(int kind) {
    return kind == GPCSD_KIND_SE || kind == GPCSD_KIND_MATERN || kind == GPCSD_KIND_MATERN32 || kind == GPCSD_KIND_MATERN52;
}

template <typename T>
struct TemporalConst {
    static constexpr T sqrt3 = T(1.7320508075688772935);
    static constexpr T sqrt5 = T(2.2360679774997896964);
};

// unit-variance k(d; ell)
template <typename T>
__host__ __device__ __forceinline__ T temporal_kernel_value(const int kind, const T d, const T ell) {
    switch (kind) {
    case GPCSD_KIND_SE:
        return exp(T(-0.5) * (d * d) / (ell * ell));                       // covariances.py:270
    case GPCSD_KIND_MATERN:
        return exp(-sqrt(d * d) / ell);                                    // covariances.py:304
    case GPCSD_KIND_MATERN32: {
        const T a = TemporalConst<T>::sqrt3 * fabs(d) / ell;
        const T h = exp(T(-0.5) * a);
        return ((T(1) + a) * h) * h;
    }
    case GPCSD_KIND_MATERN52: {
        const T a = TemporalConst<T>::sqrt5 * fabs(d) / ell;
        const T h = exp(T(-0.5) * a);
        return ((T(1) + a + a * a / T(3)) * h) * h;
    }
    }
    return std::numeric_limits<T>::quiet_NaN();
}

// unit-variance k(d; ell) and dk / d ell together
template <typename T>
__host__ __device__ __forceinline__ void temporal_kernel_value_dell(const int kind, const T d, const T ell, T &k, T &dk) {
    switch (kind) {
    case GPCSD_KIND_SE:
        k = exp(T(-0.5) * (d * d) / (ell * ell));
        dk = k * (d * d) / (ell * ell * ell);
        return;
    case GPCSD_KIND_MATERN: {
        const T ad = fabs(d);
        k = exp(-ad / ell);
        dk = k * ad / (ell * ell);
        return;
    }
    case GPCSD_KIND_MATERN32: {
        const T a = TemporalConst<T>::sqrt3 * fabs(d) / ell;
        const T h = exp(T(-0.5) * a);
        k = ((T(1) + a) * h) * h;
        dk = ((a * a / ell) * h) * h;
        return;
    }
    case GPCSD_KIND_MATERN52: {
        const T a = TemporalConst<T>::sqrt5 * fabs(d) / ell;
        const T h = exp(T(-0.5) * a);
        k = ((T(1) + a + a * a / T(3)) * h) * h;
        dk = ((a * a * (T(1) + a) / (T(3) * ell)) * h) * h;
        return;
    }
    }
    k = dk = std::numeric_limits<T>::quiet_NaN();
}

}  // namespace gpcsd
