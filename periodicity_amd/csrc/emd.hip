// Empirical mode decomposition (Rilling, Flandrin & Goncalves 2003) and the ensemble stage of CEEMDAN (Torres et al. 2011,
// Colominas et al. 2014): DESIGN.md 4.1s.  One workgroup per row; the whole sift loop and the loop over modes run inside
// the kernel with the working mode resident - in LDS for rows of at most kLdsSamples samples, in a per-workgroup slab of
// the workspace for longer ones.  The two routes are the same code over the same carve of a byte range, so a row's bytes
// do not depend on the route, on its place in the batch or on the call.
//
// One sift evaluation:
//   scan      extrema as scipy.signal.find_peaks(prominence=0) finds them (a flat top counts once, at its midpoint; a
//             plateau that touches an edge is none) and sign-bit changes, one sample per lane, BLOCK samples per trip.  A
//             ballot per wave and an ordered carry over the waves compact the two index lists in ascending order; the
//             ballot masks and the carries are kept per 64 samples and give every sample its spline interval later.
//   knots     times and values of both envelopes (p reflected extrema on either side), then the right-hand sides of the
//             two not-a-knot systems in the slope form (tridiagonal), one knot per lane.
//   solve     one Thomas sweep per envelope, lane 0 of wave 0 (upper) and lane 0 of wave 1 (lower) side by side.  The order
//             of elimination is fixed, so the slopes are the same bits whatever else runs.
//   evaluate  every sample in its interval (the piecewise cubic in scipy's CubicSpline form), mu, sigma, the three
//             decisions.  If the mode is no IMF yet, a second pass forms the same mu again and subtracts it.
// Every value that steers control flow (counts, monotonic, is_imf) is read by all threads from LDS words written before a
// barrier: each barrier is reached by all waves or by none.  No atomics, no grid synchronisation.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "pdc_internal.h"

namespace pdc {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxModes = 64;
constexpr int64_t kMaxIter = 1000000;
constexpr int64_t kMaxSamples = (int64_t)1 << 24;
constexpr int kMaxPad = 1 << 20;
// The LDS route: rows of at most kLdsSamples samples with pad_width <= kLdsPad.  emd_bytes(kLdsSamples, kLdsPad) =
// 159 232 bytes of the CU's 163 840, beside 160 bytes of static words (DESIGN.md 4.1s has the sum).
constexpr int64_t kLdsSamples = 4352;
constexpr int kLdsPad = 8;
constexpr int kLdsLimit = 160 * 1024;

struct EmdView {   // the working arrays of one row, carved from LDS or from the row's slab
    double *mode;                      // [n]
    double *kx, *kb, *kc;              // [knots]: knot times | values, then Thomas c' | right-hand sides, then slopes
    unsigned long long *maskM, *maskD; // [tiles]: the ballot of each 64 samples
    int *baseM, *baseD;                // [tiles]: extrema before those 64 samples
    int *idxM, *idxD;                  // [n / 2 + 1]: the index lists
};

__host__ __device__ inline int64_t up8(int64_t x) { return (x + 7) & ~(int64_t)7; }

// knots: |M| + |D| <= n - 2 interior extrema and 2 p reflected ones per envelope.  Every part starts on a multiple of 8.
struct EmdLayout {
    int64_t mode, kx, kb, kc, maskM, maskD, baseM, baseD, idxM, idxD, total;
};
__host__ __device__ __forceinline__ EmdLayout emd_layout(int64_t n, int64_t p) {
    const int64_t knots = n + 4 * p, tiles = (n + 63) / 64, half = n / 2 + 1;
    EmdLayout l;
    l.mode = 0;
    l.kx = l.mode + 8 * n;
    l.kb = l.kx + 8 * knots;
    l.kc = l.kb + 8 * knots;
    l.maskM = l.kc + 8 * knots;
    l.maskD = l.maskM + 8 * tiles;
    l.baseM = l.maskD + 8 * tiles;
    l.baseD = l.baseM + up8(4 * tiles);
    l.idxM = l.baseD + up8(4 * tiles);
    l.idxD = l.idxM + up8(4 * half);
    l.total = (l.idxD + up8(4 * half) + 255) & ~(int64_t)255;
    return l;
}
template <typename Byte>
__device__ __forceinline__ EmdView emd_view(Byte *base, int n, int p) {
    const EmdLayout l = emd_layout(n, p);
    EmdView v;
    v.mode = reinterpret_cast<double *>(base + l.mode);
    v.kx = reinterpret_cast<double *>(base + l.kx);
    v.kb = reinterpret_cast<double *>(base + l.kb);
    v.kc = reinterpret_cast<double *>(base + l.kc);
    v.maskM = reinterpret_cast<unsigned long long *>(base + l.maskM);
    v.maskD = reinterpret_cast<unsigned long long *>(base + l.maskD);
    v.baseM = reinterpret_cast<int *>(base + l.baseM);
    v.baseD = reinterpret_cast<int *>(base + l.baseD);
    v.idxM = reinterpret_cast<int *>(base + l.idxM);
    v.idxD = reinterpret_cast<int *>(base + l.idxD);
    return v;
}
inline int64_t emd_bytes(int64_t n, int64_t p) { return emd_layout(n, p).total; }

struct EmdArgs {
    const double *t, *x;        // [n], [rows][n]
    int n, p, max_modes, rows;
    int64_t max_iter;
    double theta1, theta2, alpha;
    double *modes, *residue;    // [rows][max_modes][n], [rows][n]
    int64_t *n_modes, *sifts, *flags, *evals;   // [rows], [rows][max_modes], [rows], [rows] (evals may be NULL)
    char *slab;                 // global route: gridDim.x slabs of slab_bytes
    int64_t slab_bytes;
    // one sift evaluation of row 0 (pdc_emd_sift) instead of the decomposition
    double *upper, *lower;
    int32_t *idx_max, *idx_min;
    int64_t *counts;            // [4]: maxima, minima, sign changes, 1 if monotonic
};

struct ScanCounts {
    int nM, nD, nZ;
};

// words[2][kWaves][3]: the waves' counts of one trip, double-buffered so that a trip costs one barrier.
__device__ __forceinline__ ScanCounts emd_scan(const EmdView &v, int n, int *words) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = (n + 63) / 64, trips = (n + kBlock - 1) / kBlock;
    const unsigned long long below = (1ull << lane) - 1ull;
    ScanCounts c = {0, 0, 0};
    for (int trip = 0; trip < trips; ++trip) {
        const int i = trip * kBlock + tid;
        bool fM = false, fD = false, fZ = false;
        int mid = 0;
        if (i + 1 < n) {
            const double here = v.mode[i], right = v.mode[i + 1];
            fZ = (__double_as_longlong(here) < 0) != (__double_as_longlong(right) < 0);
            if (i >= 1) {
                const double left = v.mode[i - 1];
                if (left < here) {          // a rise: a maximum if the flat stretch that starts here ends in a fall
                    int a = i + 1;
                    while (a < n - 1 && v.mode[a] == here) ++a;
                    fM = v.mode[a] < here;
                    mid = (i + a - 1) >> 1;
                } else if (left > here) {
                    int a = i + 1;
                    while (a < n - 1 && v.mode[a] == here) ++a;
                    fD = v.mode[a] > here;
                    mid = (i + a - 1) >> 1;
                }
            }
        }
        const unsigned long long bM = __ballot(fM), bD = __ballot(fD), bZ = __ballot(fZ);
        int *w = words + (trip & 1) * kWaves * 3;
        if (lane == 0) {
            w[wave * 3 + 0] = __popcll(bM);
            w[wave * 3 + 1] = __popcll(bD);
            w[wave * 3 + 2] = __popcll(bZ);
        }
        __syncthreads();
        int oM = c.nM, oD = c.nD;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const int m = w[k * 3 + 0], d = w[k * 3 + 1], z = w[k * 3 + 2];
            if (k < wave) {
                oM += m;
                oD += d;
            }
            c.nM += m;
            c.nD += d;
            c.nZ += z;
        }
        const int slot = trip * kWaves + wave;   // = i / 64
        if (lane == 0 && slot < tiles) {
            v.maskM[slot] = bM;
            v.maskD[slot] = bD;
            v.baseM[slot] = oM;
            v.baseD[slot] = oD;
        }
        if (fM) v.idxM[oM + __popcll(bM & below)] = mid;   // (a list holds at most (n - 1) / 2 entries: starts lie 2 apart)
        if (fD) v.idxD[oD + __popcll(bD & below)] = mid;
    }
    __syncthreads();
    return c;
}

// The sample behind knot j of an envelope with `cnt` extrema, and which side's reflection it is (-1, 0, +1).
__device__ __forceinline__ int knot_source(const int *idx, int cnt, int p, int j, int *side) {
    if (j < p) {
        *side = -1;
        return idx[p - 1 - j];
    }
    if (j < p + cnt) {
        *side = 0;
        return idx[j - p];
    }
    *side = 1;
    return idx[cnt - 1 - (j - p - cnt)];
}

__device__ __forceinline__ void emd_knot_times(const EmdView &v, const double *t, int n, int p, int nM, int nD) {
    const int Ku = nM + 2 * p, Kl = nD + 2 * p;
    for (int j = threadIdx.x; j < Ku + Kl; j += kBlock) {
        int side;
        const int src = j < Ku ? knot_source(v.idxM, nM, p, j, &side) : knot_source(v.idxD, nD, p, j - Ku, &side);
        const double ts = t[src];
        v.kx[j] = side < 0 ? 2.0 * t[0] - ts : (side > 0 ? 2.0 * t[n - 1] - ts : ts);
    }
}

__device__ __forceinline__ void emd_knot_values(const EmdView &v, int p, int nM, int nD) {
    const int Ku = nM + 2 * p, Kl = nD + 2 * p;
    for (int j = threadIdx.x; j < Ku + Kl; j += kBlock) {
        int side;
        const int src = j < Ku ? knot_source(v.idxM, nM, p, j, &side) : knot_source(v.idxD, nD, p, j - Ku, &side);
        v.kb[j] = v.mode[src];
    }
}

// Right-hand sides of the slope form: row j of the interior is h_j s_{j-1} + 2 (h_{j-1} + h_j) s_j + h_{j-1} s_{j+1}
// = 3 (h_j d_{j-1} + h_{j-1} d_j) with d the divided differences; the two not-a-knot rows as scipy's CubicSpline writes them.
__device__ __forceinline__ void emd_rhs(const double *x, const double *y, double *r, int K, int j) {
    if (j == 0) {
        const double h0 = x[1] - x[0], h1 = x[2] - x[1], d = x[2] - x[0];
        const double s0 = (y[1] - y[0]) / h0, s1 = (y[2] - y[1]) / h1;
        r[0] = ((h0 + 2.0 * d) * h1 * s0 + h0 * h0 * s1) / d;
    } else if (j == K - 1) {
        const double ha = x[K - 2] - x[K - 3], hb = x[K - 1] - x[K - 2], d = x[K - 1] - x[K - 3];
        const double sa = (y[K - 2] - y[K - 3]) / ha, sb = (y[K - 1] - y[K - 2]) / hb;
        r[K - 1] = (hb * hb * sa + (2.0 * d + hb) * ha * sb) / d;
    } else {
        const double ha = x[j] - x[j - 1], hb = x[j + 1] - x[j];
        const double sa = (y[j] - y[j - 1]) / ha, sb = (y[j + 1] - y[j]) / hb;
        r[j] = 3.0 * (hb * sa + ha * sb);
    }
}

// Thomas sweep of one envelope by one lane: cp (the scaled super-diagonal) replaces the values, the slopes replace the
// right-hand sides.  K >= 4.
__device__ __forceinline__ void emd_thomas(const double *x, double *cp, double *r, int K) {
    double xm = x[0], xc = x[1], xn = x[2];
    double c_prev = (xn - xm) / (xn - xc);
    double r_prev = r[0] / (xn - xc);
    cp[0] = c_prev;
    r[0] = r_prev;
    for (int j = 1; j <= K - 2; ++j) {
        xn = x[j + 1];
        const double ha = xc - xm, hb = xn - xc;
        const double m = 2.0 * (ha + hb) - hb * c_prev;
        c_prev = ha / m;
        r_prev = (r[j] - hb * r_prev) / m;
        cp[j] = c_prev;
        r[j] = r_prev;
        xm = xc;
        xc = xn;
    }
    // now xm = x[K - 2], xc = x[K - 1]
    {
        const double a = xc - x[K - 3], b = xm - x[K - 3];
        const double m = b - a * c_prev;
        r_prev = (r[K - 1] - a * r_prev) / m;
        r[K - 1] = r_prev;
    }
    for (int j = K - 2; j >= 0; --j) {
        r_prev = r[j] - cp[j] * r_prev;
        r[j] = r_prev;
    }
}

__device__ __forceinline__ double emd_spline(const double *x, const double *y, const double *s, int j, double tau) {
    const double x0 = x[j], h = x[j + 1] - x0, y0 = y[j], s0 = s[j], s1 = s[j + 1];
    const double slope = (y[j + 1] - y0) / h;
    const double tt = (s0 + s1 - 2.0 * slope) / h;
    const double c2 = (slope - s0) / h - tt, c3 = tt / h, dx = tau - x0;
    return ((c3 * dx + c2) * dx + s0) * dx + y0;
}

// Extrema at or before sample i, from the scan's masks: a flat top is listed at its midpoint but flagged where it
// starts, so between the two the last flagged one does not count yet.
__device__ __forceinline__ int emd_rank(const unsigned long long *mask, const int *base, const int *idx, int i) {
    const int lane = i & 63;
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    int q = base[i >> 6] + __popcll(mask[i >> 6] & upto);
    if (q > 0 && idx[q - 1] > i) --q;
    return q;
}

__device__ __forceinline__ void emd_envelopes(const EmdView &v, const double *t, int p, int nM, int nD, int i, double *up,
                                               double *lo) {
    const int Ku = nM + 2 * p, Kl = nD + 2 * p;
    int ju = p - 1 + emd_rank(v.maskM, v.baseM, v.idxM, i), jl = p - 1 + emd_rank(v.maskD, v.baseD, v.idxD, i);
    ju = ju < 0 ? 0 : (ju > Ku - 2 ? Ku - 2 : ju);   // (beyond the outermost knots, p = 0 only, the end polynomial goes on)
    jl = jl < 0 ? 0 : (jl > Kl - 2 ? Kl - 2 : jl);
    const double tau = t[i];
    *up = emd_spline(v.kx, v.kb, v.kc, ju, tau);
    *lo = emd_spline(v.kx + Ku, v.kb + Ku, v.kc + Ku, jl, tau);
}

// Scan + knots + solve; false (for every thread alike) if the row is monotonic.  `c` comes back either way.
__device__ __forceinline__ bool emd_prepare(const EmdView &v, const double *t, int n, int p, int *words, ScanCounts *c) {
    *c = emd_scan(v, n, words);
    const int nM = c->nM, nD = c->nD;
    if (nM < p || nD < p || nM + 2 * p < 4 || nD + 2 * p < 4) return false;
    const int Ku = nM + 2 * p, Kl = nD + 2 * p;
    emd_knot_times(v, t, n, p, nM, nD);
    emd_knot_values(v, p, nM, nD);
    __syncthreads();
    for (int j = threadIdx.x; j < Ku + Kl; j += kBlock) {
        if (j < Ku) emd_rhs(v.kx, v.kb, v.kc, Ku, j);
        else emd_rhs(v.kx + Ku, v.kb + Ku, v.kc + Ku, Kl, j - Ku);
    }
    __syncthreads();
    if (threadIdx.x == 0) emd_thomas(v.kx, v.kb, v.kc, Ku);
    if (threadIdx.x == 64) emd_thomas(v.kx + Ku, v.kb + Ku, v.kc + Ku, Kl);
    __syncthreads();
    emd_knot_values(v, p, nM, nD);   // (the sweep used the values' place)
    __syncthreads();
    return true;
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void emd_kernel(EmdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char emd_lds[];
    __shared__ int words[2 * kWaves * 3];
    __shared__ int votes[2 * kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, p = a.p;
    const EmdView v = LDS ? emd_view(emd_lds, n, p) : emd_view(a.slab + (int64_t)blockIdx.x * a.slab_bytes, n, p);
    const int trips = (n + kBlock - 1) / kBlock;

    if (a.counts) {   // ---- one sift evaluation of row 0
        if (blockIdx.x != 0) return;
        for (int i = tid; i < n; i += kBlock) v.mode[i] = a.x[i];
        __syncthreads();
        ScanCounts c;
        const bool ok = emd_prepare(v, a.t, n, p, words, &c);
        if (tid == 0) {
            a.counts[0] = c.nM;
            a.counts[1] = c.nD;
            a.counts[2] = c.nZ;
            a.counts[3] = ok ? 0 : 1;
        }
        for (int j = tid; j < c.nM; j += kBlock) a.idx_max[j] = v.idxM[j];
        for (int j = tid; j < c.nD; j += kBlock) a.idx_min[j] = v.idxD[j];
        if (!ok) return;
        for (int i = tid; i < n; i += kBlock) {
            double up, lo;
            emd_envelopes(v, a.t, p, c.nM, c.nD, i, &up, &lo);
            a.upper[i] = up;
            a.lower[i] = lo;
        }
        return;
    }

    for (int row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const double *x = a.x + (int64_t)row * n;
        double *residue = a.residue + (int64_t)row * n;
        double *modes = a.modes + (int64_t)row * a.max_modes * n;
        for (int i = tid; i < n; i += kBlock) residue[i] = x[i];
        int n_modes = 0;
        int64_t evals = 0, flags = 0;
        bool monotonic = false;
        while (!monotonic && n_modes < a.max_modes) {
            __syncthreads();
            for (int i = tid; i < n; i += kBlock) v.mode[i] = residue[i];
            __syncthreads();
            int64_t sifts = 0;
            bool is_imf = false;
            for (int64_t it = 0; it < a.max_iter; ++it) {
                ScanCounts c;
                if (!emd_prepare(v, a.t, n, p, words, &c)) {
                    monotonic = true;
                    break;
                }
                evals += 1;
                int over = 0;        // samples with sigma > theta_1 (the same number in every lane of a wave)
                bool broke = false;  // some sample without sigma < theta_2
                for (int trip = 0; trip < trips; ++trip) {
                    const int i = trip * kBlock + tid;
                    bool f1 = false, f2 = false;
                    if (i < n) {
                        double up, lo;
                        emd_envelopes(v, a.t, p, c.nM, c.nD, i, &up, &lo);
                        const double mu = (up + lo) / 2.0, amp = (up - lo) / 2.0;
                        const double sigma = fabs(mu / amp);
                        f1 = sigma > a.theta1;
                        f2 = !(sigma < a.theta2);
                    }
                    over += __popcll(__ballot(f1));
                    broke = broke || __ballot(f2) != 0ull;
                }
                if (lane == 0) {
                    votes[wave * 2 + 0] = over;
                    votes[wave * 2 + 1] = broke ? 1 : 0;
                }
                __syncthreads();
                int total = 0, any = 0;
#pragma unroll
                for (int k = 0; k < kWaves; ++k) {
                    total += votes[k * 2 + 0];
                    any |= votes[k * 2 + 1];
                }
                const int gap = c.nZ - (c.nM + c.nD);
                is_imf = (double)total / (double)n < a.alpha && !any && gap >= -1 && gap <= 1;
                if (is_imf) break;
                for (int i = tid; i < n; i += kBlock) {
                    double up, lo;
                    emd_envelopes(v, a.t, p, c.nM, c.nD, i, &up, &lo);
                    v.mode[i] = v.mode[i] - (up + lo) / 2.0;
                }
                sifts += 1;
                __syncthreads();
            }
            if (monotonic) break;
            if (!is_imf) flags |= 1;   // max_iter updates applied, still no IMF
            double *out = modes + (int64_t)n_modes * n;
            for (int i = tid; i < n; i += kBlock) {
                const double m = v.mode[i];
                out[i] = m;
                residue[i] = residue[i] - m;
            }
            if (tid == 0) a.sifts[(int64_t)row * a.max_modes + n_modes] = sifts;
            n_modes += 1;
        }
        if (!monotonic) {   // max_modes reached: is anything left in the residue?
            __syncthreads();
            for (int i = tid; i < n; i += kBlock) v.mode[i] = residue[i];
            __syncthreads();
            const ScanCounts c = emd_scan(v, n, words);
            if (!(c.nM < p || c.nD < p || c.nM + 2 * p < 4 || c.nD + 2 * p < 4)) flags |= 2;
        }
        if (tid == 0) {
            a.n_modes[row] = n_modes;
            a.flags[row] = flags;
            if (a.evals) a.evals[row] = evals;
        }
        __syncthreads();
    }
}

// ---- the ensemble stage of CEEMDAN --------------------------------------------------------------------------------------
// noisy[e] = residue + beta[e] * noise_modes[e][k] where realisation e has a mode k, the residue itself where not.
__global__ void ceemdan_noisy_kernel(const double *residue, const double *noise_modes, const int64_t *noise_n_modes,
                                     int noise_max_modes, int k, const double *beta, int64_t ensemble, int64_t n,
                                     double *noisy) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= ensemble * n) return;
    const int64_t e = id / n, j = id - e * n;
    double v = residue[j];
    if (noise_n_modes[e] > k) v = v + beta[e] * noise_modes[(e * noise_max_modes + k) * n + j];
    noisy[id] = v;
}

// mu = sum over e, ascending, of (noisy[e] - first mode[e]) / E; a realisation without a mode gives noisy - noisy = 0.
__global__ void ceemdan_fold_kernel(const double *noisy, const double *first, const int64_t *n_modes, int64_t ensemble,
                                    int64_t n, double *mu) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double sum = 0.0;
    for (int64_t e = 0; e < ensemble; ++e) {
        const double part = n_modes[e] > 0 ? noisy[e * n + j] - first[e * n + j] : 0.0;
        sum = sum + part / (double)ensemble;
    }
    mu[j] = sum;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct EmdDispatch {
    int64_t route, threads, rows, evals;   // route: 0 none yet, 1 LDS, 2 global workspace
};
thread_local EmdDispatch g_last = {};

bool emd_force_global() {
    const char *e = getenv("PDC_EMD_FORCE_GLOBAL");
    return e && e[0] && e[0] != '0';
}
bool emd_lds_route(int64_t n, int64_t p) { return n <= kLdsSamples && p <= kLdsPad && !emd_force_global(); }
int64_t emd_grid(int64_t rows, bool lds, int device) {
    const int64_t most = lds ? ((int64_t)1 << 30) : 2 * (int64_t)cu_count(device);
    return rows < most ? rows : most;
}
// Global route: one slab per workgroup; evals[rows] either way.
int64_t emd_work(int64_t n, int64_t rows, int64_t p, int64_t grid, bool lds) {
    return up256(rows * 8) + (lds ? 0 : grid * emd_bytes(n, p));
}

int emd_validate(const char *what, int64_t n, int64_t rows, int64_t max_iter, int64_t p, double theta1, double theta2,
                 double alpha, int64_t max_modes) {
    PDC_REQUIRE(n >= 1 && n <= kMaxSamples, "%s: 1 to 2^24 samples per row are served (got %lld)", what, (long long)n);
    PDC_REQUIRE(rows >= 1 && rows <= ((int64_t)1 << 40) / n, "%s: the number of rows is out of range (got %lld)", what,
                (long long)rows);
    PDC_REQUIRE(p >= 0 && p <= kMaxPad, "%s: pad_width must be 0 to 2^20 (got %lld)", what, (long long)p);
    PDC_REQUIRE(max_modes >= 1 && max_modes <= kMaxModes, "%s: max_modes must be 1 to %d (got %lld)", what, kMaxModes,
                (long long)max_modes);
    PDC_REQUIRE(max_iter >= 1 && max_iter <= kMaxIter, "%s: max_iter must be 1 to %lld (got %lld)", what,
                (long long)kMaxIter, (long long)max_iter);
    PDC_REQUIRE(std::isfinite(theta1) && std::isfinite(theta2) && std::isfinite(alpha),
                "%s: theta_1, theta_2 and alpha must be finite", what);
    return PDC_OK;
}

int emd_validate_host(const char *what, const double *t, const double *x, int64_t n, int64_t rows) {
    PDC_REQUIRE(t && x, "%s: NULL argument", what);
    for (int64_t i = 0; i < n; ++i) {
        PDC_REQUIRE(std::isfinite(t[i]), "%s: t[%lld] is not finite", what, (long long)i);
        PDC_REQUIRE(i == 0 || t[i] > t[i - 1], "%s: t must be strictly increasing (t[%lld])", what, (long long)i);
    }
    for (int64_t i = 0; i < rows * n; ++i)
        PDC_REQUIRE(std::isfinite(x[i]), "%s: x[%lld] is not finite", what, (long long)i);
    return PDC_OK;
}

int emd_launch(hipStream_t st, int device, EmdArgs a, void *work, bool lds, int64_t grid) {
    a.evals = a.counts ? nullptr : static_cast<int64_t *>(work);
    a.slab = static_cast<char *>(work) + up256((int64_t)a.rows * 8);
    a.slab_bytes = emd_bytes(a.n, a.p);
    g_last.route = lds ? 1 : 2;
    g_last.threads = kBlock;
    g_last.rows = a.rows;
    g_last.evals = -1;
    if (lds) {
        const int bytes = (int)emd_bytes(a.n, a.p);
        PDC_REQUIRE(bytes + 256 <= kLdsLimit, "emd: %d bytes of LDS asked for", bytes);
        PDC_TRY(allow_dynamic_lds((const void *)emd_kernel<true>, kLdsLimit - 256));
        hipLaunchKernelGGL(emd_kernel<true>, dim3((unsigned)grid), dim3(kBlock), bytes, st, a);
    } else {
        hipLaunchKernelGGL(emd_kernel<false>, dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    }
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

EmdArgs emd_args(const double *d_t, const double *d_x, int64_t n, int64_t rows, int64_t max_iter, int p, double theta1,
                 double theta2, double alpha, int max_modes, double *d_modes, double *d_residue, int64_t *d_n_modes,
                 int64_t *d_sifts, int64_t *d_flags) {
    EmdArgs a = {};
    a.t = d_t;
    a.x = d_x;
    a.n = (int)n;
    a.p = p;
    a.max_modes = max_modes;
    a.rows = (int)rows;
    a.max_iter = max_iter;
    a.theta1 = theta1;
    a.theta2 = theta2;
    a.alpha = alpha;
    a.modes = d_modes;
    a.residue = d_residue;
    a.n_modes = d_n_modes;
    a.sifts = d_sifts;
    a.flags = d_flags;
    return a;
}

}  // namespace
}  // namespace pdc

using namespace pdc;

extern "C" {

int64_t pdc_emd_lds_samples(void) { return kLdsSamples; }

int64_t pdc_emd_work_bytes(int64_t n, int64_t n_rows, int pad_width) {
    if (n < 1 || n > kMaxSamples || n_rows < 1 || n_rows > ((int64_t)1 << 40) / n || pad_width < 0 || pad_width > kMaxPad)
        return -1;
    const bool lds = emd_lds_route(n, pad_width);
    // (without a device the global route is sized for 256 compute units)
    const int64_t most = 2 * 256;
    return emd_work(n, n_rows, pad_width, lds ? n_rows : (n_rows < most ? n_rows : most), lds);
}

int pdc_emd_last_dispatch(int64_t *route, int64_t *threads, int64_t *rows, int64_t *sift_evaluations) {
    if (route) *route = g_last.route;
    if (threads) *threads = g_last.threads;
    if (rows) *rows = g_last.rows;
    if (sift_evaluations) *sift_evaluations = g_last.evals;
    return PDC_OK;
}

int pdc_emd_batch_dev(int device, void *stream, const double *d_t, const double *d_x, int64_t n, int64_t n_rows,
                      int64_t max_iter, int pad_width, double theta_1, double theta_2, double alpha, int max_modes,
                      double *d_modes, double *d_residue, int64_t *d_n_modes, int64_t *d_sifts, int64_t *d_flags) {
    PDC_TRY(emd_validate("emd", n, n_rows, max_iter, pad_width, theta_1, theta_2, alpha, max_modes));
    PDC_REQUIRE(d_t && d_x && d_modes && d_residue && d_n_modes && d_sifts && d_flags, "emd: NULL argument");
    PDC_REQUIRE(n_rows < ((int64_t)1 << 31), "emd: too many rows");
    PDC_TRY(use_device(device));
    const bool lds = emd_lds_route(n, pad_width);
    const int64_t grid = emd_grid(n_rows, lds, device);
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, emd_work(n, n_rows, pad_width, grid, lds), &work));
    return emd_launch(st, device,
                      emd_args(d_t, d_x, n, n_rows, max_iter, pad_width, theta_1, theta_2, alpha, max_modes, d_modes,
                               d_residue, d_n_modes, d_sifts, d_flags),
                      work, lds, grid);
}

int pdc_emd_batch(const double *t, const double *x, int64_t n, int64_t n_rows, int64_t max_iter, int pad_width,
                  double theta_1, double theta_2, double alpha, int max_modes, double *modes_out, double *residue_out,
                  int64_t *n_modes_out, int64_t *sifts_out, int64_t *flags_out, int device) {
    PDC_TRY(emd_validate("emd", n, n_rows, max_iter, pad_width, theta_1, theta_2, alpha, max_modes));
    PDC_REQUIRE(n_rows < ((int64_t)1 << 31), "emd: too many rows");
    PDC_TRY(emd_validate_host("emd", t, x, n, n_rows));
    PDC_REQUIRE(modes_out && residue_out && n_modes_out && sifts_out && flags_out, "emd: NULL output");
    HostCall hc(device);
    PDC_TRY(hc.status);
    const bool lds = emd_lds_route(n, pad_width);
    const int64_t grid = emd_grid(n_rows, lds, device);
    double *d_t = hc.in(SLOT_IN0, t, n * 8);
    double *d_x = hc.in(SLOT_IN1, x, n_rows * n * 8);
    double *d_modes = hc.out<double>(SLOT_OUT0, n_rows * max_modes * n * 8);
    double *d_res = hc.out<double>(SLOT_OUT1, n_rows * n * 8);
    Carve c;
    const int64_t at_nm = c.take(n_rows * 8), at_fl = c.take(n_rows * 8), at_sf = c.take(n_rows * max_modes * 8);
    char *d_small = hc.out<char>(SLOT_OUT2, c.at);
    void *d_work = hc.reserve(SLOT_WORK, emd_work(n, n_rows, pad_width, grid, lds));
    PDC_TRY(hc.status);
    PDC_HIP(hipMemsetAsync(d_small + at_sf, 0, (size_t)(n_rows * max_modes * 8), hc.stream()));
    PDC_TRY(emd_launch(hc.stream(), device,
                       emd_args(d_t, d_x, n, n_rows, max_iter, pad_width, theta_1, theta_2, alpha, max_modes, d_modes, d_res,
                                reinterpret_cast<int64_t *>(d_small + at_nm), reinterpret_cast<int64_t *>(d_small + at_sf),
                                reinterpret_cast<int64_t *>(d_small + at_fl)),
                       d_work, lds, grid));
    std::vector<int64_t> evals((size_t)n_rows);
    hc.back(residue_out, d_res, n_rows * n * 8);
    hc.back(n_modes_out, d_small + at_nm, n_rows * 8);
    hc.back(sifts_out, d_small + at_sf, n_rows * max_modes * 8);
    hc.back(flags_out, d_small + at_fl, n_rows * 8);
    hc.back(evals.data(), d_work, n_rows * 8);
    PDC_TRY(hc.status);
    PDC_HIP(hipStreamSynchronize(hc.stream()));
    // only the modes a row has come back: modes_out[b][k] for k >= n_modes_out[b] is left as it was
    for (int64_t b = 0; b < n_rows; ++b)
        hc.back(modes_out + b * max_modes * n, d_modes + b * max_modes * n, n_modes_out[b] * n * 8);
    const int status = hc.finish();
    int64_t total = 0;
    for (int64_t b = 0; b < n_rows; ++b) total += evals[(size_t)b];
    g_last.evals = status == PDC_OK ? total : -1;
    return status;
}

int pdc_emd_sift(const double *t, const double *x, int64_t n, int pad_width, double *upper_out, double *lower_out,
                 int32_t *idx_max_out, int32_t *idx_min_out, int64_t *counts_out, int device) {
    PDC_TRY(emd_validate("emd sift", n, 1, 1, pad_width, 0.0, 0.0, 0.0, 1));
    PDC_TRY(emd_validate_host("emd sift", t, x, n, 1));
    PDC_REQUIRE(upper_out && lower_out && idx_max_out && idx_min_out && counts_out, "emd sift: NULL output");
    HostCall hc(device);
    PDC_TRY(hc.status);
    const bool lds = emd_lds_route(n, pad_width);
    const int64_t half = n / 2 + 1;
    double *d_t = hc.in(SLOT_IN0, t, n * 8);
    double *d_x = hc.in(SLOT_IN1, x, n * 8);
    Carve c;
    const int64_t at_up = c.take(n * 8), at_lo = c.take(n * 8), at_im = c.take(half * 4), at_id = c.take(half * 4),
                  at_ct = c.take(4 * 8);
    char *d_out = hc.out<char>(SLOT_OUT0, c.at);
    void *d_work = hc.reserve(SLOT_WORK, emd_work(n, 1, pad_width, 1, lds));
    PDC_TRY(hc.status);
    PDC_HIP(hipMemsetAsync(d_out, 0, (size_t)c.at, hc.stream()));
    EmdArgs a = emd_args(d_t, d_x, n, 1, 1, pad_width, 0.0, 0.0, 0.0, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
    a.upper = reinterpret_cast<double *>(d_out + at_up);
    a.lower = reinterpret_cast<double *>(d_out + at_lo);
    a.idx_max = reinterpret_cast<int32_t *>(d_out + at_im);
    a.idx_min = reinterpret_cast<int32_t *>(d_out + at_id);
    a.counts = reinterpret_cast<int64_t *>(d_out + at_ct);
    PDC_TRY(emd_launch(hc.stream(), device, a, d_work, lds, 1));
    hc.back(upper_out, a.upper, n * 8);
    hc.back(lower_out, a.lower, n * 8);
    hc.back(idx_max_out, a.idx_max, half * 4);
    hc.back(idx_min_out, a.idx_min, half * 4);
    hc.back(counts_out, a.counts, 4 * 8);
    return hc.finish();
}

int pdc_ceemdan_stage_dev(int device, void *stream, const double *d_t, const double *d_residue, int64_t n,
                          const double *d_noise_modes, const int64_t *d_noise_n_modes, int64_t ensemble,
                          int noise_max_modes, int k, const double *d_beta, int64_t max_iter, int pad_width,
                          double theta_1, double theta_2, double alpha, double *d_mu, int64_t *d_n_modes,
                          int64_t *d_sifts, int64_t *d_flags) {
    PDC_TRY(emd_validate("ceemdan stage", n, ensemble, max_iter, pad_width, theta_1, theta_2, alpha, 1));
    PDC_REQUIRE(ensemble < ((int64_t)1 << 31), "ceemdan stage: the ensemble is too large");
    PDC_REQUIRE(noise_max_modes >= 1 && noise_max_modes <= kMaxModes && k >= 0,
                "ceemdan stage: noise_max_modes must be 1 to %d and k >= 0", kMaxModes);
    PDC_REQUIRE(d_t && d_residue && d_noise_modes && d_noise_n_modes && d_beta && d_mu && d_n_modes && d_sifts && d_flags,
                "ceemdan stage: NULL argument");
    PDC_TRY(use_device(device));
    const bool lds = emd_lds_route(n, pad_width);
    const int64_t grid = emd_grid(ensemble, lds, device);
    hipStream_t st = (hipStream_t)stream;
    // noisy rows | their first modes | their residues | the decomposition's own workspace
    Carve c;
    const int64_t plane = ensemble * n * 8;
    const int64_t at_noisy = c.take(plane), at_first = c.take(plane), at_res = c.take(plane),
                  at_work = c.take(emd_work(n, ensemble, pad_width, grid, lds));
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, c.at, &work));
    char *base = static_cast<char *>(work);
    double *noisy = reinterpret_cast<double *>(base + at_noisy), *first = reinterpret_cast<double *>(base + at_first);
    const int64_t cells = ensemble * n;
    hipLaunchKernelGGL(ceemdan_noisy_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, d_residue,
                       d_noise_modes, d_noise_n_modes, noise_max_modes, k, d_beta, ensemble, n, noisy);
    PDC_HIP(hipGetLastError());
    PDC_TRY(emd_launch(st, device,
                       emd_args(d_t, noisy, n, ensemble, max_iter, pad_width, theta_1, theta_2, alpha, 1, first,
                                reinterpret_cast<double *>(base + at_res), d_n_modes, d_sifts, d_flags),
                       base + at_work, lds, grid));
    hipLaunchKernelGGL(ceemdan_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, noisy, first, d_n_modes,
                       ensemble, n, d_mu);
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

}  // extern "C"
