// What the harmonic-sum scans add to the skeleton of gls_sums.h, one copy: the Chebyshev ladder from the (sin, cos) of
// a (sample, frequency) pair to those of its harmonics, the running sums of a truncated Fourier fit, the entry of its
// normal matrix from those sums, and the unrolled Cholesky that turns matrix and right-hand side into b^T M^-1 b.
// mhgls.hip and mbgls.hip use all of it, htest_common.h the ladder.  Everything is inlined into its caller.
#pragma once
#include "gls_sums.h"

#include <cmath>

namespace pdc {

// Harmonics 1 .. M of one (sample, frequency) pair from the UNscaled (sin, cos) of the first, by the Chebyshev
// recurrence x[m+1] = 2 cos(theta) x[m] - x[m-1]: per_harmonic(m, sin(m theta), cos(m theta)) in ascending m, 2 M - 2 fma.
template <int M, class PerHarmonic>
__device__ __forceinline__ void harmonic_ladder(const double s, const double c, PerHarmonic per_harmonic) {
    const double c2 = c + c;
    double sm = s, cm = c, sl = 0.0, cl = 1.0;   // harmonic m and m - 1
#pragma unroll
    for (int m = 1; m <= M; ++m) {
        per_harmonic(m, sm, cm);
        if (m < M) {
            const double cn = __builtin_fma(c2, cm, -cl), sn = __builtin_fma(c2, sm, -sl);
            cl = cm;
            sl = sm;
            cm = cn;
            sm = sn;
        }
    }
}

// The 6 H running sums of frequency k of a thread for a fit of H harmonics, one fma each per sample:
// Cm[m-1] = sum w cos(m theta), Sm[m-1] = sum w sin(m theta), m = 1 .. 2H; YC[h-1] = sum w y cos(h theta),
// YS[h-1] = sum w y sin(h theta), h = 1 .. H.
template <int H, int K>
__device__ __forceinline__ void add_fourier_sums(double (&Cm)[2 * H][K], double (&Sm)[2 * H][K], double (&YC)[H][K],
                                                 double (&YS)[H][K], const int k, const double w, const double wy,
                                                 const double s, const double c) {
    harmonic_ladder<2 * H>(s, c, [&](const int m, const double sm, const double cm) {
        Cm[m - 1][k] = __builtin_fma(w, cm, Cm[m - 1][k]);
        Sm[m - 1][k] = __builtin_fma(w, sm, Sm[m - 1][k]);
        if (m <= H) {
            YC[m - 1][k] = __builtin_fma(wy, cm, YC[m - 1][k]);
            YS[m - 1][k] = __builtin_fma(wy, sm, YS[m - 1][k]);
        }
    });
}

// Frequency k's sums as the epilogue takes them: Cs[m] = sum w cos(m theta), Ss[m] = sum w sin(m theta) for
// m = 0 .. 2H (Cs[0] = sum w, Ss[0] = 0) and b[0 .. 2H) = {YC_1, YS_1, ..., YC_H, YS_H}; a longer b keeps its tail.
template <int H, int K, int NB>
__device__ __forceinline__ void gather_fourier_sums(const double (&Cm)[2 * H][K], const double (&Sm)[2 * H][K],
                                                    const double (&YC)[H][K], const double (&YS)[H][K], const int k,
                                                    const double Wsum, double (&Cs)[2 * H + 1], double (&Ss)[2 * H + 1],
                                                    double (&b)[NB]) {
    static_assert(NB >= 2 * H, "b holds the 2H harmonic terms");
    Cs[0] = Wsum;
    Ss[0] = 0.0;
#pragma unroll
    for (int m = 1; m <= 2 * H; ++m) {
        Cs[m] = Cm[m - 1][k];
        Ss[m] = Sm[m - 1][k];
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        b[2 * h] = YC[h][k];
        b[2 * h + 1] = YS[h][k];
    }
}

// Entry (r, c), r >= c, of the normal matrix over the basis (cos th, sin th, ..., cos H th, sin H th), r, c < 2H, by
// the product-to-sum rules.
template <int H>
__device__ __forceinline__ double fourier_entry(const double (&Cs)[2 * H + 1], const double (&Ss)[2 * H + 1], int r,
                                                int c) {
    const int hr = r / 2 + 1, hc = c / 2 + 1;
    if ((r & 1) == (c & 1)) {
        const double far = Cs[hr + hc], near = Cs[hr - hc];
        return (r & 1) ? 0.5 * (near - far) : 0.5 * (near + far);
    }
    // sin(hr th) cos(hc th) = (sin((hr + hc) th) + sin((hr - hc) th)) / 2;  cos(hr th) sin(hc th): minus
    return (r & 1) ? 0.5 * (Ss[hr + hc] + Ss[hr - hc]) : 0.5 * (Ss[hr + hc] - Ss[hr - hc]);
}

// b^T M^-1 b over the first `cols` of D columns by an unrolled Cholesky in registers (as bglst_loglik in gls.hip does
// it for 4 x 4); entry(r, c), r >= c, is M.  A pivot that is not > 0, or is not finite, makes the result NaN (the fit
// is singular there to rounding).
template <int D, class Entry>
__device__ __forceinline__ double cholesky_quadratic(Entry entry, const double (&b)[D], int cols) {
    double L[D][D], z[D];
    double quad = 0.0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (j < cols) {
            double d = entry(j, j);
#pragma unroll
            for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
            bad = bad || !(d > 0.0) || !(d < HUGE_VAL);
            const double inv = 1.0 / __builtin_sqrt(d);
            double zj = b[j];
#pragma unroll
            for (int q = 0; q < j; ++q) zj -= L[j][q] * z[q];
            z[j] = zj * inv;
            quad += z[j] * z[j];
#pragma unroll
            for (int i = j + 1; i < D; ++i) {
                double v = entry(i, j);
#pragma unroll
                for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q];
                L[i][j] = v * inv;
            }
        }
    }
    return bad ? __builtin_nan("") : quad;
}

// the two normalisations of GLS (gls_epilogue.h)
__device__ __forceinline__ double normalised_power(double p, int psd, double Werr, double YY) {
    return psd ? p * (0.5 * Werr) : p / YY;
}

}  // namespace pdc
