// Device-side pieces of the celerite likelihood kernel (gp.hip): the software exp(-x) of the propagator, the packed
// index of the symmetric state matrix, the running product that stands in for a sum of logarithms.
#pragma once
#include <hip/hip_runtime.h>

namespace pdc {

constexpr int kGpMaxTerms = 4;   // J: celerite terms of a candidate (the state is 2J x 2J)

// exp(-x) for x >= 0: x = k ln 2 - r with k = rint(x / ln 2), |r| <= ln 2 / 2, e^r by its Taylor series to r^13
// (remainder below 5e-18 of e^r), scaled by 2^-k through ldexp, which rounds into the denormals once.  x is clamped at
// 750: 2^-1082 e^r is 0 in double, as is everything from x = 745.14 on (e^-745.14 < 2^-1075), and a NaN comes out of
// the clamp as 750 - the result is never NaN.  exp_neg(0) is exactly 1.
__device__ __forceinline__ double exp_neg(double x) {
    x = __builtin_fmin(x, 750.0);
    const double k = __builtin_rint(x * 1.44269504088896338700e+00);
    double r = __builtin_fma(k, 6.93147180369123816490e-01, -x);    // ln 2, high part: 32 trailing zero bits
    r = __builtin_fma(k, 1.90821492927058770002e-10, r);            //       low part
    double p = 1.0 / 6227020800.0;
    p = __builtin_fma(p, r, 1.0 / 479001600.0);
    p = __builtin_fma(p, r, 1.0 / 39916800.0);
    p = __builtin_fma(p, r, 1.0 / 3628800.0);
    p = __builtin_fma(p, r, 1.0 / 362880.0);
    p = __builtin_fma(p, r, 1.0 / 40320.0);
    p = __builtin_fma(p, r, 1.0 / 5040.0);
    p = __builtin_fma(p, r, 1.0 / 720.0);
    p = __builtin_fma(p, r, 1.0 / 120.0);
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, -(int)k);
}

// Entry (i, k) of a symmetric R x R matrix kept as its upper triangle, row by row: R (R + 1) / 2 values.
template <int R>
__host__ __device__ constexpr int sym_index(int i, int k) {
    return i <= k ? i * R - i * (i - 1) / 2 + (k - i) : k * R - k * (k - 1) / 2 + (i - k);
}

// sum ln D_n without a logarithm per sample: the product of the mantissas, renormalised into [1/2, 1) after every
// factor, and the sum of the exponents.  A factor is split before it is multiplied in, so no product leaves
// [1/4, 1): a denormal D loses nothing.  ln of the product = ln(mant) + exp ln 2, one log at the end.
struct LogProduct {
    double mant = 0.5;
    int exp_chunk = 1;       // (0.5 x 2^1 = 1) exponents since the last carry(): a chunk of samples cannot overflow it
    long long exp_sum = 0;
    __device__ __forceinline__ void times(double d) {
        const double m = mant * __builtin_amdgcn_frexp_mant(d);
        exp_chunk += __builtin_amdgcn_frexp_exp(d) + __builtin_amdgcn_frexp_exp(m);
        mant = __builtin_amdgcn_frexp_mant(m);
    }
    __device__ __forceinline__ void carry() {
        exp_sum += exp_chunk;
        exp_chunk = 0;
    }
    __device__ __forceinline__ double log() const {   // after carry()
        return __builtin_fma((double)exp_sum, 6.93147180559945286227e-01, ::log(mant));
    }
};

}  // namespace pdc
