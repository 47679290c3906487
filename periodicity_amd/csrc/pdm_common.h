// Shared by pdm.hip and pdm_ragged.hip (inside an anonymous namespace of each): the staging chunk, the
// workgroup reduction, the statistics' epilogues and the LDS size rule of the phase-binning scans.
#pragma once

// samples staged per barrier (256 = the staging area a 256-thread workgroup owns anyway; 128 measured 2 %,
// 64 10 % slower at C5)
#ifndef PDC_PDM_CHUNK
#define PDC_PDM_CHUNK 256
#endif
constexpr int kChunk = PDC_PDM_CHUNK;

template <int BLOCK>
__device__ __forceinline__ double block_reduce(double v, double *red, bool take_max) {
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_down(v, o, 64);
        v = take_max ? (u > v ? u : v) : v + u;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < BLOCK / 64; ++w) r = take_max ? (red[w] > r ? red[w] : r) : r + red[w];
    return r;
}

// theta from one period's fine-bin histogram (phase.py:137-148); sum_at / cnt_at read bin b.
template <typename SumAt, typename CntAt>
__device__ __forceinline__ double theta_from_bins(SumAt sum_at, CntAt cnt_at, int m0, int nc, double q_total,
                                                  double q_nan, double q_over, double sigma) {
    double num = (double)nc * (q_total - q_nan) - q_over;
    long long n_sum = 0;
    int good = 0;
    for (int k = 0; k < m0; ++k) {
        double s = 0.0;
        long long c = 0;
        for (int j = 0; j < nc; ++j) {
            int b = k + j;
            if (b >= m0) {
                if (b == m0) {  // [1.0, (m0+1)/m0): only phi == 1.0 can live here
                    s += sum_at(m0);
                    c += cnt_at(m0);
                }
                b -= m0;
            }
            s += sum_at(b);
            c += cnt_at(b);
        }
        if (c > 1) {
            num -= s * s / (double)c;
            n_sum += c;
            ++good;
        } else if (c == 1) {
            num -= s * s;  // a singleton contributes x^2 - x^2 = 0 and is not a "good" bin
        }
    }
    // no cover with two or more members: the reference divides an empty sum by zero -> NaN
    // (phase.py:147); here `num` would only hold the rounding residue of the singletons
    return good == 0 ? __builtin_nan("") : (num / (double)(n_sum - good)) / sigma;
}

// Analysis of Variance (Schwarzenberg-Czerny 1989, MNRAS 241, 153, eq. 1-3) from the same histogram:
// r = m0 phase bins [k/r, (k+1)/r) (phi == 1.0 joins the last one), n valid samples,
//     s1^2 = sum_i n_i (xbar_i - xbar)^2 / (r - 1),   s2^2 = sum_i sum_j (x_ij - xbar_i)^2 / (n - r),
// Theta_AoV = s1^2 / s2^2.  With S_i = sum of the (mean-shifted) samples of bin i and Q their total
// square: between = sum S_i^2 / n_i - (sum S_i)^2 / n,  within = Q - sum S_i^2 / n_i.
template <typename SumAt, typename CntAt>
__device__ __forceinline__ double aov_from_bins(SumAt sum_at, CntAt cnt_at, int m0, double q_valid) {
    double per_bin = 0.0, s_all = 0.0;
    long long n = 0;
    for (int k = 0; k < m0; ++k) {
        double s = sum_at(k);
        long long c = cnt_at(k);
        if (k == m0 - 1) {
            s += sum_at(m0);
            c += cnt_at(m0);
        }
        if (c > 0) per_bin += s * s / (double)c;
        s_all += s;
        n += c;
    }
    if (n <= m0 || m0 < 2) return __builtin_nan("");
    const double between = per_bin - s_all * s_all / (double)n;
    const double within = q_valid - per_bin;
    return ((double)(n - m0) * between) / ((double)(m0 - 1) * within);
}

// Conditional entropy (Graham et al. 2013, MNRAS 434, 2629, eq. 1): H_c = sum_ij p(m_j, phi_i)
// ln(p(phi_i) / p(m_j, phi_i)) over the occupied cells of an m0 x mag (phase x magnitude) partition;
// cnt_at(i * mag + j) reads cell (i, j), row m0 (phi == 1.0) joins row m0 - 1.
template <typename CntAt>
__device__ __forceinline__ double ce_from_bins(CntAt cnt_at, int m0, int mag) {
    long long n = 0;
    for (int c = 0; c < (m0 + 1) * mag; ++c) n += cnt_at(c);
    if (n == 0) return __builtin_nan("");
    double h = 0.0;
    for (int i = 0; i < m0; ++i) {
        long long row = 0;
        for (int j = 0; j < mag; ++j) row += cnt_at(i * mag + j) + (i == m0 - 1 ? cnt_at(m0 * mag + j) : 0);
        for (int j = 0; j < mag; ++j) {
            const long long c = cnt_at(i * mag + j) + (i == m0 - 1 ? cnt_at(m0 * mag + j) : 0);
            if (c > 0) h += ((double)c / (double)n) * log((double)row / (double)c);
        }
    }
    return h;
}

// Gregory & Loredo (1992, ApJ 398, 146): arrival times t_i, model M_m = a periodic rate that is constant in
// each of m phase bins.  For trial frequency w and phase offset phi the likelihood depends on the data only
// through the multiplicity W_m(w, phi) = N! / (n_1! ... n_m!) of the bin counts (their eq. 5.13-5.14), and
// the marginal over the offset,
//     S_m(w) = (1 / 2 pi) Int dphi  m^N / W_m(w, phi),
// is what the odds ratio O_m1 (eq. 5.28) integrates over dw / w.  Here: ln S_m(w) with the offset integral as
// the mean over `offsets` equally spaced shifts of the bin boundaries by 1 / (m offsets) of a cycle - the
// counts of every shift are sums of `offsets` consecutive FINE bins of a histogram over F = m offsets bins
// [f / F, (f + 1) / F) (phi == 1.0 joins the last), cnt_at(f).  Log-sum-exp over the shifts, lgamma for the
// factorials.
template <typename CntAt>
__device__ __forceinline__ double gl_from_bins(CntAt cnt_at, int F, int m) {
    const int offsets = F / m;
    long long n = 0;
    for (int f = 0; f <= F; ++f) n += cnt_at(f);
    if (n == 0 || offsets < 1) return __builtin_nan("");
    const double base = (double)n * log((double)m) - lgamma((double)n + 1.0);
    double top = 0.0, sum = 0.0;
    for (int k = 0; k < offsets; ++k) {
        double lw = base;
        int f = k;
        for (int j = 0; j < m; ++j) {
            long long c = 0;
            for (int i = 0; i < offsets; ++i) {
                c += cnt_at(f) + (f == F - 1 ? cnt_at(F) : 0);
                f = f + 1 == F ? 0 : f + 1;
            }
            lw += lgamma((double)c + 1.0);
        }
        if (k == 0 || lw > top) {   // running log-sum-exp
            sum = k == 0 ? 1.0 : sum * exp(top - lw) + 1.0;
            top = lw;
        } else {
            sum += exp(lw - top);
        }
    }
    return top + log(sum / (double)offsets);
}

// `last` = highest histogram bin; bytes_per_bin 12: sum + count, 4: counts only (two 16-bit cells per word)
size_t lds_bytes(int last, int block, int bytes_per_bin = 12) {
    const size_t stage = (size_t)(kChunk > block ? kChunk : block) * 16;
    const size_t nbins = (size_t)last + 1;
    const size_t hist = bytes_per_bin == 4 ? ((nbins + 1) / 2 + 1) * block * 4 : nbins * block * 12;
    return stage + hist + (size_t)(last + 2) * 8 + 64;
}

constexpr int64_t kCellSamples = 65280;   // samples a workgroup of a counts-only kind may bin: its cells are 16-bit
