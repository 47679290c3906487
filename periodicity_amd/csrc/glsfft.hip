// Generalized Lomb-Scargle by the reference's OWN algorithm on the device (SURVEY.md §8 f1,
// "Tier F"): Press-Rybicki extirpolation + inverse FFT, exactly as the reference's
// src/periodicity/spectral.py:11-40 (`_trig_sum`) does it on the CPU, followed by
// the same epilogue (spectral.py:113-132).  O(N + nfft log nfft) instead of O(N nf); it inherits
// the reference's approximation error (median ~1e-3 relative vs the exact sums) and therefore
// reproduces `power_ref` itself, where the direct-sum kernel (gls.hip) reproduces the exact sums.
//
// Pipeline (all on one stream; nothing but power[nf], or the raw sums, leaves the device), for one curve or a batch
// (blockIdx.y = curve, or curve x grid); per curve 2 or 3 complex grids: (w y @ df), (w @ 2 df), (w @ df) with fit_mean:
//   prologue               weights, centring, YY, {tmin, tmax, sorted}                               (:99-108, 120)
//                          glsfft_prep_{a,c}: one curve, grid-wide, fixed-order partials
//                          glsfft_prep_batch_kernel: one workgroup per curve
//   extirpolation          `Extirp`: weights pre-rotated to fmin about tmin (:19-20), grid position (:21), whole hits
//                          deposited (:22-24), the rest over four neighbours with cubic Lagrange weights (:25-33)
//                          glsfft_deposit_kernel: sorted stamps on a grid that does not wrap - every thread owns cells and
//                            adds their samples in order, no atomics, no memset; otherwise it only zeroes the grid
//                          glsfft_spread_kernel: one thread per sample, fp64 global atomics - the grids the deposit
//                            kernel left empty (stamps out of order, or a grid that wraps), else it returns at once
//   inverse FFT            Stockham autosort, out of place, ping-pong between the grids and one scratch buffer; every
//                          pass streams the array once (HBM-bound: 32 B per point per pass); twiddles from the
//                          cycle-domain sincos (no tables, no recurrences)                                     (:34)
//                          fft_pass_lds_kernel<RB>: radix 16 x RB through LDS in one trip (N >= 4096)
//                          fft_pass_kernel<R>: plain radix-16/8/4/2 for what is left
//                          the first pass reads live cells only, the last stores [0, nf) only
//   glsfft_epilogue_kernel undo the tmin shift (:35-37), scale by nfft (:38-39), power (:113-132);
//                          glsfft_raw_sums_kernel stops at S and C (pdc_trig_sums_fft); row_nanmax_kernel for batches
// How the path got here, with the experiments that were withdrawn: docs/history.md.
#include "pdc_internal.h"
#include "gls_epilogue.h"
#include "gls_sums.h"

#include <cstdlib>
#include <vector>

using namespace pdc;

namespace {

constexpr int kBlock = 256;

struct cplx {
    double re, im;
};
__device__ __forceinline__ cplx operator+(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx operator-(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) {
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

// ---- in-register DFT of R = 2^m points, e^{+2 pi i jk/R} (inverse direction), natural order -------
template <int R, int K>
__device__ __forceinline__ cplx twiddle_const() {
    // exp(+2 pi i K / R) for R <= 16, K < R/2
    constexpr int q = K * (16 / R);  // sixteenths of a turn, 0..7
    constexpr double c[8] = {1.0, 0.92387953251128675613, 0.70710678118654752440,
                             0.38268343236508977173, 0.0, -0.38268343236508977173,
                             -0.70710678118654752440, -0.92387953251128675613};
    constexpr double s[8] = {0.0, 0.38268343236508977173, 0.70710678118654752440,
                             0.92387953251128675613, 1.0, 0.92387953251128675613,
                             0.70710678118654752440, 0.38268343236508977173};
    return {c[q], s[q]};
}

template <int R>
struct Dft {
    template <int K>
    static __device__ __forceinline__ void combine(cplx *x, const cplx *e, const cplx *o) {
        if constexpr (K < R / 2) {
            cplx t;
            if constexpr (K == 0) {
                t = o[0];
            } else if constexpr (4 * K == R) {
                t = {-o[K].im, o[K].re};  // times +i
            } else {
                t = cmul(twiddle_const<R, K>(), o[K]);
            }
            x[K] = e[K] + t;
            x[K + R / 2] = e[K] - t;
            combine<K + 1>(x, e, o);
        }
    }
    static __device__ __forceinline__ void run(cplx *x) {
        cplx e[R / 2], o[R / 2];
#pragma unroll
        for (int i = 0; i < R / 2; ++i) {
            e[i] = x[2 * i];
            o[i] = x[2 * i + 1];
        }
        Dft<R / 2>::run(e);
        Dft<R / 2>::run(o);
        combine<0>(x, e, o);
    }
};
template <>
struct Dft<1> {
    static __device__ __forceinline__ void run(cplx *) {}
};

// The extirpolated grids are empty beyond the last sample's position (80 % of the cells at the default
// five samples per peak): the deposit kernel does not write those cells and the FIRST pass does not read
// them.  ord = {tmin, tmax, sorted} of the curve (see glsfft_deposit_kernel); nullptr: every cell is live.
struct LiveArgs {
    const double *ord;
    int ord_stride, ngrid, g_first;
    double df;
};

__device__ __forceinline__ bool deposit_in_order(const double *ord, double nfftd, double dfg) {
    const double span = ord[1] - ord[0];   // (NaN or -inf when no time stamp is a number: the atomic kernel then)
    return ord[2] != 0.0 && span >= 0.0 && (span * nfftd) * dfg < nfftd;
}

// cells [0, live) of transform `y` of the launch may be non-zero
__device__ __forceinline__ int64_t live_cells(const LiveArgs &l, int64_t y, int64_t nfft) {
    if (!l.ord) return nfft;
    const int64_t curve = y / l.ngrid;
    const int g = l.g_first + (int)(y - curve * l.ngrid);
    const double *ord = l.ord + curve * l.ord_stride;
    const double nfftd = (double)nfft, dfg = g == 1 ? 2.0 * l.df : l.df;
    if (!deposit_in_order(ord, nfftd, dfg)) return nfft;
    const int64_t live = (int64_t)(((ord[1] - ord[0]) * nfftd) * dfg) + 4;   // last position + its neighbours
    return live < nfft ? live : nfft;
}

// One Stockham pass: N points, sub-transforms of length Ns become length Ns*R.
template <int R>
__global__ __launch_bounds__(kBlock) void fft_pass_kernel(const cplx *__restrict__ in,
                                                          cplx *__restrict__ out, int64_t N,
                                                          int64_t Ns, int64_t keep, LiveArgs lv) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t T = N / R;
    if (j >= T) return;
    const int64_t live = live_cells(lv, blockIdx.y, N);
    in += (int64_t)blockIdx.y * N;   // batch of independent transforms, one per blockIdx.y
    out += (int64_t)blockIdx.y * N;
    const int64_t k = j & (Ns - 1);
    cplx v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = j + r * T < live ? in[j + r * T] : cplx{0.0, 0.0};
    const double inv = 1.0 / (double)(Ns * R);  // power of two: exact
#pragma unroll
    for (int r = 1; r < R; ++r) {
        double s, c;
        sincos_cycles((double)(r * k) * inv, s, c);  // e^{+2 pi i r k / (Ns R)}
        v[r] = cmul(v[r], cplx{c, s});
    }
    Dft<R>::run(v);
    const int64_t j0 = (j - k) * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (j0 + r * Ns < keep) out[j0 + r * Ns] = v[r];  // last pass: only the first `keep` outputs
}


// One Stockham pass of radix R = 16 x RB (RB = 16, 8, 4, 2) through LDS: one HBM trip does a radix-16
// stage and a radix-RB stage.  A workgroup of 256 threads owns JT = 256/RB consecutive butterflies j
// (each an R-point DFT over the inputs in[j + r*T], r = r1 + RB*r2, r1 < RB, r2 < 16):
//   stage A  thread (jj, r1): outer twiddles, 16-point DFT over r2, inner twiddle W_R^(r1*s2) -> LDS
//   stage B  (jj, s2) pairs, 16/RB per thread: RB-point DFT over r1 -> Y[s2 + 16 s1]
//            -> out[(j-k)*R + k + s*Ns]
// Global accesses are runs of >= 16 consecutive complex numbers (256 B).  Requires N >= 4096.
template <int RB>
__global__ __launch_bounds__(256) void fft_pass_lds_kernel(const cplx *__restrict__ in,
                                                            cplx *__restrict__ out, int64_t N,
                                                            int64_t Ns, int64_t keep, LiveArgs lv) {
    constexpr int R = 16 * RB;
    constexpr int JT = 256 / RB;          // butterflies per workgroup
    // Padded LDS row per butterfly: ONE complex number (16 B) of padding, not a whole number of LDS bank rows (32 banks
    // x 4 B), which would be no skew at all.  With R + 1 the 16-byte slot of (jj, r1, s2) is (jj + s2) mod 8: eight
    // lanes per slot, the minimum for 64 x 16 B.
    constexpr int ROW = R + 1;
    __shared__ cplx tile[JT * ROW];       // [jj][r1][s2]
    __shared__ cplx wR[R];
    const int tid = threadIdx.x;
    const int64_t live = live_cells(lv, blockIdx.y, N);
    in += (int64_t)blockIdx.y * N;
    out += (int64_t)blockIdx.y * N;
    if (tid < R) {
        double s, c;
        sincos_cycles((double)tid * (1.0 / (double)R), s, c);
        wR[tid] = cplx{c, s};
    }
    const int64_t T = N / R;
    const int64_t j_base = (int64_t)blockIdx.x * JT;
    // ---- stage A -------------------------------------------------------------------------------
    {
        const int jj = tid % JT, r1 = tid / JT;
        const int64_t j = j_base + jj;
        const int64_t k = j & (Ns - 1);
        cplx v[16];
#pragma unroll
        for (int r2 = 0; r2 < 16; ++r2) {
            const int64_t at = j + (int64_t)(r1 + RB * r2) * T;
            v[r2] = at < live ? in[at] : cplx{0.0, 0.0};
        }
        if (Ns > 1) {
            // outer twiddle e^{2 pi i r k / (R Ns)}, r = r1 + RB r2: tw(r1) * tw(RB)^r2
            const double inv = 1.0 / (double)(Ns * R);
            double s, c;
            sincos_cycles((double)((int64_t)r1 * k) * inv, s, c);
            cplx tw = cplx{c, s};
            sincos_cycles((double)((int64_t)RB * k) * inv, s, c);
            const cplx step = cplx{c, s};
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) {
                v[r2] = cmul(v[r2], tw);
                tw = cmul(tw, step);
            }
        }
        Dft<16>::run(v);
        __syncthreads();  // wR ready
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2)
            tile[jj * ROW + r1 * 16 + s2] = cmul(v[s2], wR[(r1 * s2) % R]);
    }
    __syncthreads();
    // ---- stage B -------------------------------------------------------------------------------
#pragma unroll
    for (int it = 0; it < 16 / RB; ++it) {
        const int pair = tid + it * 256;  // (jj, s2) pairs, JT * 16 of them
        // lanes run over jj when consecutive j write consecutive addresses (Ns >= 16), over s2 when
        // the R outputs of one j are contiguous (first pass, Ns == 1)
        const int jj = Ns > 1 ? pair % JT : pair / 16;
        const int s2 = Ns > 1 ? pair / JT : pair % 16;
        const int64_t j = j_base + jj;
        const int64_t k = j & (Ns - 1);
        cplx v[RB];
#pragma unroll
        for (int r1 = 0; r1 < RB; ++r1) v[r1] = tile[jj * ROW + r1 * 16 + s2];
        Dft<RB>::run(v);
        const int64_t j0 = (j - k) * R + k;
#pragma unroll
        for (int s1 = 0; s1 < RB; ++s1) {
            const int64_t o = j0 + (int64_t)(s2 + 16 * s1) * Ns;
            if (o < keep) out[o] = v[s1];  // last pass: only the first `keep` outputs are ever read
        }
    }
}

// ---- prologue: spectral.py:99-108, 120 -- two grid-wide kernels, deterministic partials ------------
// A: per-workgroup partial sums of err^-2 and err^-2 * y and the partial minimum of t.
// C: every workgroup re-reduces A's partials (<= kMaxPart, fixed order -> identical in all of them),
//    writes w and w*y and its partial of YY = sum w y^2.  Consumers reduce the YY partials the same way.
constexpr int kMaxPart = 512;

struct FftPrepArgs {
    const double *t, *y, *dy;
    int64_t n;
    int fit_mean, nparts;
    double *wy, *w;
    double *part;   // [5][kMaxPart]: sum err^-2 | sum err^-2 y | min t | -max t | out-of-order pairs
    double *ypart;  // [kMaxPart]: partial YY
    double *scal;   // {YY (filled by the epilogue's reduction), Werr, tmin, tmax, sorted}
};

// block-wide minimum for BLOCK-thread blocks, the same in every thread; `red` holds BLOCK / 64 numbers and may be in use
// up to the call (as with block_sum)
template <int BLOCK>
__device__ __forceinline__ double block_min(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_down(v, o, 64);
        v = u < v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < BLOCK / 64; ++w) r = red[w] < r ? red[w] : r;
    return r;
}

__global__ __launch_bounds__(kBlock) void glsfft_prep_a_kernel(FftPrepArgs a) {
    __shared__ double red[kBlock / 64];
    double sw = 0.0, swy = 0.0, tmin = __builtin_inf(), ntmax = __builtin_inf(), disorder = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
        const double e = a.dy ? a.dy[i] : 1.0;
        const double wr = 1.0 / (e * e);
        sw += wr;
        swy += wr * a.y[i];
        const double ti = a.t[i];
        tmin = ti < tmin ? ti : tmin;
        ntmax = -ti < ntmax ? -ti : ntmax;
        if (i > 0 && !(ti >= a.t[i - 1])) disorder = 1.0;   // (a NaN counts as disorder)
    }
    sw = block_sum<kBlock>(sw, red);
    swy = block_sum<kBlock>(swy, red);
    tmin = block_min<kBlock>(tmin, red);
    ntmax = block_min<kBlock>(ntmax, red);
    disorder = block_sum<kBlock>(disorder, red);
    if (threadIdx.x == 0) {
        a.part[blockIdx.x] = sw;
        a.part[kMaxPart + blockIdx.x] = swy;
        a.part[2 * kMaxPart + blockIdx.x] = tmin;
        a.part[3 * kMaxPart + blockIdx.x] = ntmax;
        a.part[4 * kMaxPart + blockIdx.x] = disorder;
    }
}

// fixed-order reduction of `count` partials by one workgroup (identical result in every workgroup)
__device__ __forceinline__ double reduce_partials(const double *p, int count, double *red) {
    double v = 0.0;
    for (int i = threadIdx.x; i < count; i += kBlock) v += p[i];
    return block_sum<kBlock>(v, red);
}

__global__ __launch_bounds__(kBlock) void glsfft_prep_c_kernel(FftPrepArgs a) {
    __shared__ double red[kBlock / 64];
    const double W = reduce_partials(a.part, a.nparts, red);
    const double ybar = a.fit_mean ? reduce_partials(a.part + kMaxPart, a.nparts, red) / W : 0.0;
    double tmin = __builtin_inf();
    for (int i = threadIdx.x; i < a.nparts; i += kBlock) {
        const double u = a.part[2 * kMaxPart + i];
        tmin = u < tmin ? u : tmin;
    }
    tmin = block_min<kBlock>(tmin, red);
    double ntmax = __builtin_inf();
    for (int i = threadIdx.x; i < a.nparts; i += kBlock) {
        const double u = a.part[3 * kMaxPart + i];
        ntmax = u < ntmax ? u : ntmax;
    }
    ntmax = block_min<kBlock>(ntmax, red);
    const double disorder = reduce_partials(a.part + 4 * kMaxPart, a.nparts, red);
    double yy = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
        const double w = inv_var(a.dy, i) / W;
        const double yc = a.y[i] - ybar;
        a.w[i] = w;
        a.wy[i] = w * yc;
        yy += w * yc * yc;
    }
    yy = block_sum<kBlock>(yy, red);
    if (threadIdx.x == 0) {
        a.ypart[blockIdx.x] = yy;
        if (blockIdx.x == 0) {
            a.scal[1] = W;
            a.scal[2] = tmin;
            a.scal[3] = -ntmax;                        // latest time stamp
            a.scal[4] = disorder == 0.0 ? 1.0 : 0.0;   // time stamps in non-decreasing order
        }
    }
}

// ---- prologue of a batch: B light curves on one grid (bootstrap replicates share t), one workgroup per curve ----
struct FftBatchPrepArgs {
    const double *t, *y, *dy;
    const int64_t *offsets;  // [B + 1]
    int shared_t, fit_mean;
    double *w, *wy;   // [n_total]
    double *scal;     // [B][8] = {YY, Werr, tmin, tmax, sorted, -, -, -}
    // bootstrap replicates by index (spectral.py:146-148): y, dy = ONE curve, sample i of replicate b is picks[b n + i]
    const int32_t *picks;
};

__global__ __launch_bounds__(1024) void glsfft_prep_batch_kernel(FftBatchPrepArgs a) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    const int64_t off = a.offsets[blockIdx.x], n = a.offsets[blockIdx.x + 1] - off;
    const double *t = a.shared_t ? a.t : a.t + off;
    const int32_t *pk = a.picks ? a.picks + off : nullptr;
    const double *y = pk ? a.y : a.y + off;
    const double *dy = a.dy ? (pk ? a.dy : a.dy + off) : nullptr;
    auto at = [pk](int64_t i) -> int64_t { return pk ? (int64_t)pk[i] : i; };
    double acc = 0.0, tmin = __builtin_inf(), ntmax = __builtin_inf(), disorder = 0.0;
    for (int64_t i = tid; i < n; i += 1024) {
        const double e = dy ? dy[at(i)] : 1.0;
        acc += 1.0 / (e * e);
        const double ti = t[i];
        tmin = ti < tmin ? ti : tmin;
        ntmax = -ti < ntmax ? -ti : ntmax;
        if (i > 0 && !(ti >= t[i - 1])) disorder = 1.0;   // (a NaN counts as disorder)
    }
    const double W = block_sum<1024>(acc, red);
    disorder = block_sum<1024>(disorder, red);
    tmin = block_min<1024>(tmin, red);
    ntmax = block_min<1024>(ntmax, red);
    double ybar = 0.0;
    if (a.fit_mean) {
        acc = 0.0;
        for (int64_t i = tid; i < n; i += 1024) {
            const double e = dy ? dy[at(i)] : 1.0;
            acc += (1.0 / (e * e)) / W * y[at(i)];
        }
        ybar = block_sum<1024>(acc, red);
    }
    double yy = 0.0;
    for (int64_t i = tid; i < n; i += 1024) {
        const double e = dy ? dy[at(i)] : 1.0;
        const double w = (1.0 / (e * e)) / W;
        const double yc = y[at(i)] - ybar;
        a.w[off + i] = w;
        a.wy[off + i] = w * yc;
        yy += w * yc * yc;
    }
    yy = block_sum<1024>(yy, red);
    if (tid == 0) {
        double *s = a.scal + (int64_t)blockIdx.x * 8;
        s[0] = yy;
        s[1] = W;
        s[2] = tmin;
        s[3] = -ntmax;
        s[4] = disorder == 0.0 ? 1.0 : 0.0;
    }
}

// ---- extirpolation: spectral.py:18-33 ---------------------------------------------------------------
// One sample on one grid: where it lands and how a weight is shared out, every rule once and in the reference's order
// of operations.  The atomic route (spread_one) and the ordered one (glsfft_deposit_kernel) are built from these, so
// they agree to the order of their additions.  The two walks over the deposits stay two: as one visitor called by
// both, glsfft_deposit_kernel took 128 registers instead of 124 and 402 us instead of 398 for 200 curves.
struct Extirp {
    // w * np.exp(2j * np.pi * fmin * (t - tmin)): the phase is fl(fl(2 pi fmin) * dt) radians
    static __device__ __forceinline__ void prerotation(double fmin, double dt, double &sn, double &cs) {
        sincos((6.283185307179586 * fmin) * dt, &sn, &cs);
    }
    // (t - tmin) * nfft * df, which "% nfft" leaves as it is on a grid that does not wrap
    static __device__ __forceinline__ double position(double dt, double nfftd, double df) { return (dt * nfftd) * df; }
    // tnorm = ((t - tmin) * nfft * df) % nfft
    static __device__ __forceinline__ double tnorm(double dt, double nfftd, double df) {
        double tn = fmod(position(dt, nfftd, df), nfftd);
        if (tn != 0.0 && tn < 0.0) tn += nfftd;
        return tn;
    }
    // tnorm % 1 == 0: one deposit of the weight itself at cell tn
    static __device__ __forceinline__ bool whole(double tn) { return tn - __builtin_floor(tn) == 0.0; }
    // else four neighbours from here on
    static __device__ __forceinline__ int64_t first_neighbour(double tn, int64_t nfft) {
        const int64_t ilo = (int64_t)(tn - 2.0);  // astype(int): truncation toward zero
        return ilo < 0 ? 0 : (ilo > nfft - 4 ? nfft - 4 : ilo);
    }
    // weight h leaves (h * numerator) / divisor(j) at neighbour ilo + 3 - j, j = 0 .. 3 in the reference's order
    static __device__ __forceinline__ double numerator(double tn, int64_t ilo) {
        const double x = tn - (double)ilo;
        return ((x * (x - 1.0)) * (x - 2.0)) * (x - 3.0);
    }
    static __device__ __forceinline__ double divisor(int j, double tn, int64_t ind) {
        const double den[4] = {6.0, -2.0, 2.0, -6.0};  // the reference's running denominator
        return den[j] * (tn - (double)ind);
    }
};

// The curves of a launch and their grids, for both extirpolation kernels.
struct ExtirpArgs {
    const double *t, *h0, *h1;   // h0: weights of grid 0 (w y); h1: weights of grids 1 (@ 2 df) and 2 (@ df)
    const int64_t *offsets;      // per-curve sample ranges; nullptr: one curve of n samples
    int64_t n;
    int shared_t, ngrid;         // ngrid = grids per curve in `grids` (3 with fit_mean, else 2; raw sums: 1)
    int slot_first, nslots;      // deposit slots of this launch: slot 0 = grid 0 (and grid 2, which shares its
                                 // positions and phases, when ngrid == 3); slot 1 = grid 1
    int64_t nfft;
    double df, fmin;
    double *grids;               // [curve][ngrid][nfft] complex: every live cell is written
    // (filled by fft_pipeline from the epilogue's scalars)
    const double *ord;           // ord[curve * ord_stride + {0, 1, 2}] = {tmin, tmax, sorted}
    int ord_stride;
};

// ---- atomics: one thread per sample, for the grids that glsfft_deposit_kernel has only zeroed ----------------------
__device__ __forceinline__ void grid_add(double *grid, int64_t idx, double re, double im) {
    unsafeAtomicAdd(grid + 2 * idx, re);
    unsafeAtomicAdd(grid + 2 * idx + 1, im);
}

__device__ __forceinline__ void spread_one(double *grid, int64_t nfft, double dt, double h, double df, double fmin,
                                           const double *ord) {
    const double nfftd = (double)nfft;
    if (deposit_in_order(ord, nfftd, df)) return;   // glsfft_deposit_kernel has done this grid
    double sn, cs;
    Extirp::prerotation(fmin, dt, sn, cs);
    const double hre = h * cs, him = h * sn;
    const double tn = Extirp::tnorm(dt, nfftd, df);
    if (Extirp::whole(tn)) {
        grid_add(grid, (int64_t)tn, hre, him);
        return;
    }
    const int64_t ilo = Extirp::first_neighbour(tn, nfft);
    const double prod = Extirp::numerator(tn, ilo);
    const double nre = hre * prod, nim = him * prod;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t ind = ilo + (3 - j);
        const double d = Extirp::divisor(j, tn, ind);
        grid_add(grid, ind, nre / d, nim / d);
    }
}

__global__ __launch_bounds__(kBlock) void glsfft_spread_kernel(ExtirpArgs a) {
    const int64_t curve = blockIdx.y;
    const int64_t off = a.offsets ? a.offsets[curve] : 0;
    const int64_t n = a.offsets ? a.offsets[curve + 1] - off : a.n;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double *ord = a.ord + curve * a.ord_stride;
    const double dt = a.t[(a.shared_t ? 0 : off) + i] - ord[0];
    double *grids = a.grids + 2 * ((curve * a.ngrid) * a.nfft);
    spread_one(grids, a.nfft, dt, a.h0[off + i], a.df, a.fmin, ord);
    if (a.ngrid > 1) spread_one(grids + 2 * a.nfft, a.nfft, dt, a.h1[off + i], 2.0 * a.df, 2.0 * a.fmin, ord);   // (:110)
    if (a.ngrid > 2) spread_one(grids + 4 * a.nfft, a.nfft, dt, a.h1[off + i], a.df, a.fmin, ord);
}

// ---- the same deposits without atomics, in a fixed order ---------------------------------------------
// With time stamps in non-decreasing order and a grid that does not wrap ((tmax - tmin) nfft df < nfft -
// always so for the default n >= 1 samples per peak), grid positions rise with the sample index, so the
// samples that touch a cell are consecutive.  A thread owns groups of four consecutive cells: a search
// finds the first sample that can reach them, the deposits are added in sample order and stored once -
// bitwise reproducible (the atomic kernel above adds in arrival order), and the memset goes away: every
// cell up to the last sample's reach is written (the empty ones with zero), the rest is read by nobody.
// Otherwise this kernel only zeroes the grid and the atomic kernel does the work (`deposit_in_order` is
// false for it exactly then).

constexpr int kDepCells = 4;                     // cells per thread
#ifndef PDC_DEP_ITERS
#define PDC_DEP_ITERS 4
#endif
constexpr int kDepIters = PDC_DEP_ITERS;         // groups of cells per thread: the workgroup's search is shared
constexpr int kDepSpan = kDepCells * kBlock * kDepIters;   // cells per workgroup
constexpr int kDepStage = 768;                   // samples of a workgroup's range kept in LDS: position, pre-rotation, weights

__global__ __launch_bounds__(kBlock) void glsfft_deposit_kernel(ExtirpArgs a) {
    __shared__ double s_pos[kDepStage];
    // the samples themselves too, with their pre-rotation exp(2 pi i fmin (t - tmin)) evaluated ONCE, by the thread that
    // stages them (else three dependent global loads and a sincos for every (sample, group of cells) visit)
    __shared__ double s_cs[kDepStage], s_sn[kDepStage], s_h[kDepStage], s_h2[kDepStage];
    __shared__ unsigned long long s_ballot[2][kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t curve = blockIdx.y / a.nslots;
    const int g = a.slot_first + (int)(blockIdx.y - curve * a.nslots);
    const bool twin = g == 0 && a.ngrid == 3;
    const int64_t G0 = (int64_t)blockIdx.x * kDepSpan;
    // (cells from `live` on are never read: the first FFT pass takes them as zero)
    const int64_t live = live_cells(LiveArgs{a.ord, a.ord_stride, 1, g, a.df}, curve, a.nfft);
    if (G0 >= live) return;   // (workgroup-uniform)
    const int64_t off = a.offsets ? a.offsets[curve] : 0;
    const int64_t n = a.offsets ? a.offsets[curve + 1] - off : a.n;
    const double *t = a.t + (a.shared_t ? 0 : off);
    const double *h = (g == 0 ? a.h0 : a.h1) + off, *h2 = a.h1 + off;
    const double *ord = a.ord + curve * a.ord_stride;
    const double dfg = g == 1 ? 2.0 * a.df : a.df, fming = g == 1 ? 2.0 * a.fmin : a.fmin;
    const double nfftd = (double)a.nfft, tmin = ord[0];
    // tnorm of sample i: used only when the grid does not wrap, where "% nfft" (a libm fmod per probe) changes nothing
    auto position = [&](int64_t i) -> double { return Extirp::position(t[i] - tmin, nfftd, dfg); };
    const bool ordered = n > 0 && deposit_in_order(ord, nfftd, dfg);   // (workgroup-uniform)
    int64_t w_first = 0, w_last = 0;
    bool staged = false;
    if (ordered) {
        // The samples that can reach this workgroup's cells, [w_first, w_last): first sample at or beyond
        // G0 - 4 and first at or beyond G0 + span + 4, by a 256-ary search made by the whole workgroup
        // (three rounds for 1e5 samples instead of 17 dependent loads per thread).
        const double bound[2] = {(double)(G0 - 4), (double)(G0 + kDepSpan + 4)};
        int64_t lo[2] = {0, 0}, hi[2] = {n, n};   // the answer lies in [lo, hi]
        for (;;) {
            const int64_t w0 = hi[0] - lo[0], w1 = hi[1] - lo[1];
            if (w0 <= 0 && w1 <= 0) break;        // (workgroup-uniform)
            bool pred[2];
            int64_t step[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int64_t w = hi[q] - lo[q];
                step[q] = (w + kBlock - 1) / kBlock;
                const int64_t at = lo[q] + (int64_t)tid * step[q];
                pred[q] = w > 0 && at < hi[q] && position(at) >= bound[q];
            }
            __syncthreads();
            const unsigned long long b0 = __ballot(pred[0]), b1 = __ballot(pred[1]);
            if (lane == 0) {
                s_ballot[0][wave] = b0;
                s_ballot[1][wave] = b1;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (hi[q] - lo[q] <= 0) continue;
                int first = kBlock;               // first probe at or beyond the bound
                for (int w = kBlock / 64 - 1; w >= 0; --w)
                    if (s_ballot[q][w]) first = w * 64 + __builtin_ctzll(s_ballot[q][w]);
                const int64_t probes = (hi[q] - lo[q] + step[q] - 1) / step[q];   // probes inside [lo, hi)
                const int64_t new_hi = first < probes ? lo[q] + (int64_t)first * step[q] : hi[q];
                const int64_t new_lo = first > 0 ? lo[q] + (int64_t)((first < probes ? first : probes) - 1) * step[q] + 1 : lo[q];
                lo[q] = new_lo < new_hi ? new_lo : new_hi;
                hi[q] = new_hi;
            }
        }
        w_first = lo[0];
        w_last = lo[1];
        staged = w_last - w_first <= kDepStage;   // (workgroup-uniform)
        if (staged)
            for (int64_t i = w_first + tid; i < w_last; i += kBlock) {
                s_pos[i - w_first] = position(i);
                double sn0, cs0;
                Extirp::prerotation(fming, t[i] - tmin, sn0, cs0);
                s_cs[i - w_first] = cs0;
                s_sn[i - w_first] = sn0;
                s_h[i - w_first] = h[i];
                s_h2[i - w_first] = twin ? h2[i] : 0.0;
            }
        __syncthreads();
    }
    auto pos_at = [&](int64_t i) -> double { return staged ? s_pos[i - w_first] : position(i); };
    for (int it = 0; it < kDepIters; ++it) {
        const int64_t g0 = G0 + ((int64_t)it * kBlock + tid) * kDepCells;
        if (g0 >= live) break;
        double acc_re[kDepCells], acc_im[kDepCells], twin_re[kDepCells], twin_im[kDepCells];
#pragma unroll
        for (int c = 0; c < kDepCells; ++c) acc_re[c] = acc_im[c] = twin_re[c] = twin_im[c] = 0.0;
        if (ordered) {
            const double lo_t = (double)(g0 - 4), hi_t = (double)(g0 + kDepCells + 4);
            int64_t first = w_first, last = w_last;   // first sample of the workgroup's range at or beyond lo_t
            while (first < last) {
                const int64_t mid = (first + last) >> 1;
                if (pos_at(mid) >= lo_t) last = mid; else first = mid + 1;
            }
            for (int64_t i = first; i < w_last; ++i) {
                const double tn = pos_at(i);
                if (!(tn < hi_t)) break;
                int64_t ilo = 0;
                const bool whole = Extirp::whole(tn);
                if (!whole) {
                    ilo = Extirp::first_neighbour(tn, a.nfft);
                    if (ilo + 3 < g0 || ilo >= g0 + kDepCells) continue;
                } else if ((int64_t)tn < g0 || (int64_t)tn >= g0 + kDepCells) {
                    continue;
                }
                const double hi_ = staged ? s_h[i - w_first] : h[i];
                const double h2i = !twin ? 0.0 : (staged ? s_h2[i - w_first] : h2[i]);
                double sn, cs;
                if (staged) {
                    sn = s_sn[i - w_first];
                    cs = s_cs[i - w_first];
                } else {
                    Extirp::prerotation(fming, t[i] - tmin, sn, cs);
                }
                const double hre = hi_ * cs, him = hi_ * sn;
                const double kre = twin ? h2i * cs : 0.0, kim = twin ? h2i * sn : 0.0;
                if (whole) {   // one deposit
                    const int64_t ind = (int64_t)tn;
#pragma unroll
                    for (int c = 0; c < kDepCells; ++c)
                        if (ind == g0 + c) {
                            acc_re[c] += hre;
                            acc_im[c] += him;
                            twin_re[c] += kre;
                            twin_im[c] += kim;
                        }
                    continue;
                }
                const double prod = Extirp::numerator(tn, ilo);
                const double nre = hre * prod, nim = him * prod, mre = kre * prod, mim = kim * prod;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t ind = ilo + (3 - j);
                    if (ind < g0 || ind >= g0 + kDepCells) continue;
                    const double d = Extirp::divisor(j, tn, ind);
                    const double vre = nre / d, vim = nim / d;
                    const double ure = twin ? mre / d : 0.0, uim = twin ? mim / d : 0.0;
#pragma unroll
                    for (int c = 0; c < kDepCells; ++c)
                        if (ind == g0 + c) {
                            acc_re[c] += vre;
                            acc_im[c] += vim;
                            twin_re[c] += ure;
                            twin_im[c] += uim;
                        }
                }
            }
        }
        double *out = a.grids + 2 * ((curve * a.ngrid + g) * a.nfft + g0);
        double *out2 = a.grids + 2 * ((curve * a.ngrid + 2) * a.nfft + g0);
#pragma unroll
        for (int c = 0; c < kDepCells; ++c)
            if (g0 + c < a.nfft) {
                out[2 * c] = acc_re[c];
                out[2 * c + 1] = acc_im[c];
                if (twin) {
                    out2[2 * c] = twin_re[c];
                    out2[2 * c + 1] = twin_im[c];
                }
            }
    }
}

// ---- epilogue: spectral.py:34-39 then :113-132 ----------------------------------------------------------
struct FftEpiArgs {
    const double *ypart;   // partial YY sums of a single curve (nparts of them); nullptr: YY = scal[0]
    int nparts, psd;
    int64_t nf;
    double *power;         // [curve][nf]; glsfft_raw_sums_kernel: S
    double *raw_c;         // glsfft_raw_sums_kernel: C
    const double *scal;    // scal[curve * scal_stride + {0 .. 4}] = {YY, Werr, tmin, tmax, sorted}
    int scal_stride;
    // (filled by fft_pipeline)
    int ngrid;
    const cplx *result;    // [curve][ngrid][nfft]: transforms of (w y @ df), (w @ 2 df), (w @ df) with fit_mean
    int64_t nfft;
    double df, fmin;
};

// fftgrid[:nf] of pocketfft's ifft, which divides by nfft (the reference multiplies it back: do both so that the
// roundings match), *= exp(2j pi tmin f); C = nfft*re, S = nfft*im
__device__ __forceinline__ void finish_sum(cplx z, double tmin, double f, double nfftd, double &S,
                                           double &C) {
    const double scale = 1.0 / nfftd;
    z.re *= scale;
    z.im *= scale;
    if (tmin != 0.0) {
        const double ang = (6.283185307179586 * tmin) * f;
        double sn, cs;
        sincos(ang, &sn, &cs);
        z = cmul(z, cplx{cs, sn});
    }
    C = nfftd * z.re;
    S = nfftd * z.im;
}

__global__ __launch_bounds__(kBlock) void glsfft_epilogue_kernel(FftEpiArgs a) {
    __shared__ double red[kBlock / 64];
    const int64_t b = blockIdx.y;
    const double *sc = a.scal + b * a.scal_stride;
    const double YY = a.ypart ? reduce_partials(a.ypart, a.nparts, red) : sc[0];   // (workgroup-uniform)
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.nf) return;
    const double nfftd = (double)a.nfft, tmin = sc[2];
    const cplx *g = a.result + (b * a.ngrid) * a.nfft;
    const double f = a.fmin + a.df * (double)j;
    double Sh, Ch, S2, C2, S = 0.0, C = 0.0;
    finish_sum(g[j], tmin, f, nfftd, Sh, Ch);
    finish_sum(g[a.nfft + j], tmin, 2.0 * a.fmin + (2.0 * a.df) * (double)j, nfftd, S2, C2);
    double p;
    if (a.ngrid == 3) {
        finish_sum(g[2 * a.nfft + j], tmin, f, nfftd, S, C);
        p = gls_power_from_sums<true>(Sh, Ch, S, C, S2, C2, YY, sc[1], a.psd);
    } else {
        p = gls_power_from_sums<false>(Sh, Ch, S, C, S2, C2, YY, sc[1], a.psd);
    }
    a.power[b * a.nf + j] = p;
}

// pdc_trig_sums_fft: one curve, one grid, S and C as they are
__global__ __launch_bounds__(kBlock) void glsfft_raw_sums_kernel(FftEpiArgs a) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.nf) return;
    double S, C;
    finish_sum(a.result[j], a.scal[2], a.fmin + a.df * (double)j, (double)a.nfft, S, C);
    a.power[j] = S;
    a.raw_c[j] = C;
}

// NaN-aware maximum and its first index per row (Signal.amax / argmax, core.py:202-215).  Wave w takes the w-th
// quarter of the row, its lanes stride through it: ascending ranges per lane and per wave, as ArgMax asks.
__global__ __launch_bounds__(kBlock) void row_nanmax_kernel(const double *power, int64_t nf,
                                                            double *amax, int64_t *argmax) {
    __shared__ double rv[kBlock / 64];
    __shared__ long long ri[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (scalar: so is its range)
    const double *x = power + (int64_t)blockIdx.x * nf;
    const int64_t quarter = (nf + kBlock / 64 - 1) / (kBlock / 64);
    const int64_t beg = wave * quarter, end = beg + quarter < nf ? beg + quarter : nf;
    ArgMax m;
    // (four loads in flight: one at a time, a wave on its own quarter took 20 us for 200 rows of 12000 against the 17 of
    // a workgroup striding over the row together)
    for (int64_t i = beg + lane; i < end; i += 4 * 64) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + 64 * u < end ? x[i + 64 * u] : __builtin_nan("");
#pragma unroll
        for (int u = 0; u < 4; ++u) m.take(v[u], i + 64 * u);
    }
    if (m.block_fold<kBlock / 64>(rv, ri, lane, wave)) {
        if (amax) amax[blockIdx.x] = m.j >= 0 ? m.v : __builtin_nan("");
        if (argmax) argmax[blockIdx.x] = m.j;
    }
}

// ---- host side -----------------------------------------------------------------------------------------
int64_t fft_length(int64_t nf) {
    // 1 << int(nf * 5 - 1).bit_length()                                         (spectral.py:18)
    int64_t v = nf * 5 - 1, bits = 0;
    while (v > 0) {
        ++bits;
        v >>= 1;
    }
    return (int64_t)1 << bits;
}

template <int R>
void launch_pass(hipStream_t st, const cplx *in, cplx *out, int64_t N, int64_t Ns, int batch,
                 int64_t keep, const LiveArgs &lv) {
    const int64_t T = N / R;
    hipLaunchKernelGGL(fft_pass_kernel<R>, dim3((unsigned)((T + kBlock - 1) / kBlock), (unsigned)batch),
                       dim3(kBlock), 0, st, in, out, N, Ns, keep, lv);
}

// Unnormalised inverse FFT of `batch` contiguous arrays of N = 2^bits points in `a`, using `b` (same
// size) as the other half of the ping-pong; returns the buffer that holds the results.  Only the first
// `keep_out` outputs of every transform are needed by the caller (spectral.py:34 keeps [:nf]): the
// final pass skips the stores beyond them.
cplx *inverse_fft(hipStream_t st, cplx *a, cplx *b, int64_t N, int batch = 1, int64_t keep_out = -1,
                  LiveArgs input_live = LiveArgs{nullptr, 0, 1, 0, 0.0}) {
    int bits = 0;
    while (((int64_t)1 << bits) < N) ++bits;
    int64_t Ns = 1;
    cplx *src = a, *dst = b;
    static const bool no_lds = [] { const char *e = getenv("PDC_FFT_NO256"); return e && e[0] == '1'; }();
    const LiveArgs all_live{nullptr, 0, 1, 0, 0.0};
    while (bits > 0) {
        const LiveArgs &lv = Ns == 1 ? input_live : all_live;   // only the first pass reads the deposits
        int r = bits >= 4 ? 4 : bits;
        if (bits == 5) r = 3;  // 5 = 3 + 2 rather than 4 + 1
        // LDS-blocked passes (radix 16 x RB in one trip through HBM): 8 bits at a time, then the
        // remainder in one more LDS pass if it is 5..7 bits, else in a plain radix-2/4/8/16 pass
        int lds_bits = 0;
        if (!no_lds && bits >= 5 && N >= 4096)  // a workgroup covers R * JT = 4096 points
            lds_bits = bits >= 8 ? 8 : bits;
        const int done = lds_bits ? lds_bits : r;   // bits of this pass
        const int64_t keep = (bits == done && keep_out >= 0) ? keep_out : N;  // final pass only
        if (lds_bits) {
            const int64_t R = (int64_t)1 << lds_bits;
            const int jt = 256 / (int)(R / 16);
            const dim3 grid((unsigned)((N / R) / jt), (unsigned)batch);
            switch (lds_bits) {
                case 8: hipLaunchKernelGGL(fft_pass_lds_kernel<16>, grid, dim3(256), 0, st, src, dst, N, Ns, keep, lv); break;
                case 7: hipLaunchKernelGGL(fft_pass_lds_kernel<8>, grid, dim3(256), 0, st, src, dst, N, Ns, keep, lv); break;
                case 6: hipLaunchKernelGGL(fft_pass_lds_kernel<4>, grid, dim3(256), 0, st, src, dst, N, Ns, keep, lv); break;
                default: hipLaunchKernelGGL(fft_pass_lds_kernel<2>, grid, dim3(256), 0, st, src, dst, N, Ns, keep, lv); break;
            }
        } else {
            switch (r) {
                case 4: launch_pass<16>(st, src, dst, N, Ns, batch, keep, lv); break;
                case 3: launch_pass<8>(st, src, dst, N, Ns, batch, keep, lv); break;
                case 2: launch_pass<4>(st, src, dst, N, Ns, batch, keep, lv); break;
                default: launch_pass<2>(st, src, dst, N, Ns, batch, keep, lv); break;
            }
        }
        Ns <<= done;
        bits -= done;
        cplx *tmp = src;
        src = dst;
        dst = tmp;
    }
    return src;
}

// The `n_curves` curves of `x`, the longest of n_max samples: deposits -> atomics -> inverse FFT -> epilogue (-> row
// maxima).  `scratch`: ping-pong partner of x.grids; `e`: the caller's part of the epilogue's arguments.
// grid_by_grid (one curve): the passes of one grid after the other, see pdc_gls_scan_fft_dev.
int fft_pipeline(hipStream_t st, ExtirpArgs x, int64_t n_curves, int64_t n_max, cplx *scratch, bool grid_by_grid,
                 FftEpiArgs e, double *amax = nullptr, int64_t *argmax = nullptr) {
    x.ord = e.scal + 2;
    x.ord_stride = e.scal_stride;
    // ALL grids' deposits in one launch up front: a deposit launch is a chain of dependent searches, ~50 us whatever it
    // writes, and only the live fifth of a grid is written
    hipLaunchKernelGGL(glsfft_deposit_kernel, dim3((unsigned)((x.nfft + kDepSpan - 1) / kDepSpan), (unsigned)(n_curves * x.nslots)),
                       dim3(kBlock), 0, st, x);
    if (n_max > 0)
        hipLaunchKernelGGL(glsfft_spread_kernel, dim3((unsigned)((n_max + kBlock - 1) / kBlock), (unsigned)n_curves),
                           dim3(kBlock), 0, st, x);
    PDC_HIP(hipGetLastError());
    cplx *grids = reinterpret_cast<cplx *>(x.grids);
    if (grid_by_grid) {   // (every grid's transform ends in the same half of its ping-pong: the layout of the results holds)
        for (int g = 0; g < x.ngrid; ++g)
            e.result = inverse_fft(st, grids + g * x.nfft, scratch + g * x.nfft, x.nfft, 1, e.nf, LiveArgs{x.ord, 0, 1, g, x.df}) - g * x.nfft;
    } else {
        e.result = inverse_fft(st, grids, scratch, x.nfft, (int)(n_curves * x.ngrid), e.nf, LiveArgs{x.ord, x.ord_stride, x.ngrid, 0, x.df});
    }
    PDC_HIP(hipGetLastError());
    e.ngrid = x.ngrid;
    e.nfft = x.nfft;
    e.df = x.df;
    e.fmin = x.fmin;
    const dim3 bins((unsigned)((e.nf + kBlock - 1) / kBlock), (unsigned)n_curves);
    if (e.raw_c)
        hipLaunchKernelGGL(glsfft_raw_sums_kernel, bins, dim3(kBlock), 0, st, e);
    else
        hipLaunchKernelGGL(glsfft_epilogue_kernel, bins, dim3(kBlock), 0, st, e);
    if (amax || argmax) hipLaunchKernelGGL(row_nanmax_kernel, dim3((unsigned)n_curves), dim3(kBlock), 0, st, e.power, e.nf, amax, argmax);
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

// Workspace: the weights of n samples, `scal_bytes` of scalars (and partials), n_grids grids and their ping-pong partner
// (both contiguous: batched FFT stride = nfft), power_rows rows of nf powers.
struct FftLayout {
    int64_t wy, w, scal, grids, scratch, power, total;
};

FftLayout fft_layout(int64_t n, int64_t scal_bytes, int64_t n_grids, int64_t nfft, int64_t power_rows = 0, int64_t nf = 0) {
    FftLayout L;
    int64_t at = 0;
    auto sub = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 255) & ~(int64_t)255; return o; };
    L.wy = sub(n * 8);
    L.w = sub(n * 8);
    L.scal = sub(scal_bytes);
    L.grids = sub(n_grids * nfft * 16);
    L.scratch = sub(n_grids * nfft * 16);
    L.power = sub(power_rows * nf * 8);
    L.total = at;
    return L;
}

// one curve: scal[8] | part[5][kMaxPart] | ypart[kMaxPart], and three grids whether fit_mean or not
FftLayout fft_layout_single(int64_t n, int64_t nfft) { return fft_layout(n, (6 * kMaxPart + 8) * 8, 3, nfft); }

}  // namespace

extern "C" {

int64_t pdc_gls_fft_work_bytes(int64_t n, int64_t nf) {
    if (n < 0 || nf < 0) return -1;
    return fft_layout_single(n, fft_length(nf > 0 ? nf : 1)).total;
}

int pdc_gls_scan_fft_dev(int device, void *stream, const double *d_t, const double *d_y,
                         const double *d_dy, int64_t n, double fmin, double df, int64_t nf,
                         int fit_mean, int psd, double *d_power, void *work, int64_t work_bytes) {
    PDC_REQUIRE(d_t && d_y && (d_power || nf == 0), "gls_fft: NULL argument");
    PDC_REQUIRE(n >= 0 && nf >= 0 && nf < ((int64_t)1 << 40), "gls_fft: bad size");
    if (nf == 0) return PDC_OK;
    const int64_t nfft = fft_length(nf);
    const FftLayout L = fft_layout_single(n, nfft);
    PDC_REQUIRE(work && work_bytes >= L.total, "gls_fft: workspace too small (%lld < %lld bytes)",
                (long long)work_bytes, (long long)L.total);
    PDC_TRY(use_device(device));
    hipStream_t st = (hipStream_t)stream;
    char *base = static_cast<char *>(work);
    double *wy = reinterpret_cast<double *>(base + L.wy);
    double *w = reinterpret_cast<double *>(base + L.w);
    double *scal = reinterpret_cast<double *>(base + L.scal);

    int nparts = (int)((n + 4 * kBlock - 1) / (4 * kBlock));
    nparts = nparts < 1 ? 1 : (nparts > kMaxPart ? kMaxPart : nparts);
    FftPrepArgs p{d_t, d_y, d_dy, n, fit_mean, nparts, wy, w, scal + 8, scal + 8 + 5 * kMaxPart, scal};
    hipLaunchKernelGGL(glsfft_prep_a_kernel, dim3(nparts), dim3(kBlock), 0, st, p);
    hipLaunchKernelGGL(glsfft_prep_c_kernel, dim3(nparts), dim3(kBlock), 0, st, p);
    PDC_HIP(hipGetLastError());

    const int ngrid = fit_mean ? 3 : 2;
    // One grid's ping-pong (32 B per point) may fit in the 256 MiB Infinity Cache while all of them do
    // not: then the PASSES grid by grid, so that each grid's ping-pong stays cache-warm (measured at
    // nfft = 2^23: 0.66 vs 0.69 ms); otherwise batched FFT passes (gridDim.y = ngrid; 6.4 vs 6.7 ms at
    // nfft = 2^26).  The deposits are one launch either way (fft_pipeline).
    const int64_t mall = (int64_t)256 << 20;
    const bool grid_by_grid = nfft * 32 <= mall && (int64_t)ngrid * nfft * 32 > mall;
    return fft_pipeline(st, ExtirpArgs{d_t, wy, w, nullptr, n, 0, ngrid, 0, 2, nfft, df, fmin, reinterpret_cast<double *>(base + L.grids)},
                        1, n, reinterpret_cast<cplx *>(base + L.scratch), grid_by_grid,
                        FftEpiArgs{p.ypart, nparts, psd, nf, d_power, nullptr, scal, 0});
}

int pdc_gls_scan_fft(const double *t, const double *y, const double *dy, int64_t n, double fmin,
                     double df, int64_t nf, int fit_mean, int psd, double *power_out, int device) {
    PDC_REQUIRE(t && y && (power_out || nf == 0), "gls_fft: NULL argument");
    PDC_REQUIRE(n >= 0 && nf >= 0, "gls_fft: negative size");
    HostCall hc(device);
    const int64_t wb = pdc_gls_fft_work_bytes(n, nf);
    double *d_t = hc.in(SLOT_IN0, t, n * 8), *d_y = hc.in(SLOT_IN1, y, n * 8), *d_dy = hc.in(SLOT_IN2, dy, n * 8);
    double *d_pow = hc.out<double>(SLOT_OUT0, nf * 8);
    void *d_work = hc.reserve(SLOT_WORK, wb);
    PDC_TRY(hc.status);
    PDC_TRY(pdc_gls_scan_fft_dev(device, hc.stream(), d_t, d_y, d_dy, n, fmin, df, nf, fit_mean, psd, d_pow, d_work, wb));
    hc.back(power_out, d_pow, nf * 8);
    return hc.finish();
}


}  // extern "C"

namespace {
// `picks` != NULL: the bootstrap form - y and dy hold ONE curve of offsets[1] samples, replicate b reads
// sample picks[b n + i]; only the indices cross PCIe
int fft_batch_host(const double *t, const double *y, const double *dy, const int64_t *offsets,
                   int64_t n_curves, int shared_t, double fmin, double df, int64_t nf,
                   int fit_mean, int psd, double *power_out, double *amax_out,
                   int64_t *argmax_out, int device, const int32_t *picks) {
    PDC_REQUIRE(t && y && offsets, "gls_fft_batch: t, y and offsets must not be NULL");
    PDC_REQUIRE(n_curves >= 1 && nf >= 0, "gls_fft_batch: bad size");
    PDC_REQUIRE(power_out || amax_out || argmax_out, "gls_fft_batch: no output requested");
    // (first here, last in check(): a call wrong in both ways keeps the text it has always got)
    PDC_REQUIRE(offsets[0] == 0, "gls_fft_batch: offsets[0] must be 0");
    GlsBatchIn in;
    PDC_TRY(in.check("gls_fft_batch", offsets, n_curves, shared_t));
    if (nf == 0) return PDC_OK;
    HostCall hc(device);
    const int64_t n_total = in.n_total, n_max = in.n_max;
    const int64_t nfft = fft_length(nf);
    const int ngrid = fit_mean ? 3 : 2;
    // curves per pass: grids + ping-pong scratch + power within ~8 GiB, and gridDim.y <= 65535
    const int64_t per_curve = 2 * ngrid * nfft * 16 + nf * 8;
    int64_t chunk = ((int64_t)8 << 30) / per_curve;
    chunk = chunk < 1 ? 1 : chunk;
    chunk = chunk > n_curves ? n_curves : chunk;
    chunk = chunk > 65535 / ngrid ? 65535 / ngrid : chunk;
    const FftLayout L = fft_layout(n_total, n_curves * 64, chunk * ngrid, nfft, chunk, nf);
    in.upload(hc, t, y, dy, offsets, n_curves, picks != nullptr);   // (bootstrap: one curve of values / errors on the device)
    const int32_t *d_picks = hc.in(SLOT_OUT0, picks, n_total * 4);
    double *d_amax = amax_out ? hc.out<double>(SLOT_OUT1, n_curves * 8) : nullptr;
    int64_t *d_arg = argmax_out ? hc.out<int64_t>(SLOT_OUT2, n_curves * 8) : nullptr;
    char *base = hc.out<char>(SLOT_WORK, L.total);
    PDC_TRY(hc.status);
    hipStream_t st = hc.stream();
    double *w = reinterpret_cast<double *>(base + L.w), *wy = reinterpret_cast<double *>(base + L.wy);
    double *scal = reinterpret_cast<double *>(base + L.scal), *power = reinterpret_cast<double *>(base + L.power);
    hipLaunchKernelGGL(glsfft_prep_batch_kernel, dim3((unsigned)n_curves), dim3(1024), 0, st,
                       FftBatchPrepArgs{in.d_t, in.d_y, in.d_dy, in.d_off, shared_t, fit_mean, w, wy, scal, d_picks});
    PDC_HIP(hipGetLastError());
    for (int64_t c0 = 0; c0 < n_curves; c0 += chunk) {
        const int64_t bc = n_curves - c0 < chunk ? n_curves - c0 : chunk;
        PDC_TRY(fft_pipeline(st, ExtirpArgs{in.d_t, wy, w, in.d_off + c0, 0, shared_t, ngrid, 0, 2, nfft, df, fmin,
                                            reinterpret_cast<double *>(base + L.grids)},
                             bc, n_max, reinterpret_cast<cplx *>(base + L.scratch), false,
                             FftEpiArgs{nullptr, 0, psd, nf, power, nullptr, scal + c0 * 8, 8},
                             d_amax ? d_amax + c0 : nullptr, d_arg ? d_arg + c0 : nullptr));
        hc.back(power_out ? power_out + c0 * nf : nullptr, power, bc * nf * 8);
    }
    hc.back(amax_out, d_amax, n_curves * 8);
    hc.back(argmax_out, d_arg, n_curves * 8);
    return hc.finish();
}
}  // namespace

int pdc::gls_bootstrap_fft(const double *t, const double *y, const double *dy, int64_t n, const int32_t *picks,
                           int64_t n_boot, double fmin, double df, int64_t nf, int fit_mean, int psd,
                           double *amax_out, int64_t *argmax_out, int device) {
    std::vector<int64_t> offsets((size_t)n_boot + 1);
    for (int64_t b = 0; b <= n_boot; ++b) offsets[(size_t)b] = b * n;
    return fft_batch_host(t, y, dy, offsets.data(), n_boot, 1, fmin, df, nf, fit_mean, psd, nullptr, amax_out,
                          argmax_out, device, picks);
}

extern "C" {

int pdc_gls_scan_fft_batch(const double *t, const double *y, const double *dy, const int64_t *offsets,
                           int64_t n_curves, int shared_t, double fmin, double df, int64_t nf,
                           int fit_mean, int psd, double *power_out, double *amax_out,
                           int64_t *argmax_out, int device) {
    return fft_batch_host(t, y, dy, offsets, n_curves, shared_t, fmin, df, nf, fit_mean, psd, power_out, amax_out,
                          argmax_out, device, nullptr);
}

int pdc_trig_sums_fft(const double *t, const double *h, int64_t n, double df, int64_t nf,
                      double fmin, double *S_out, double *C_out, int device) {
    PDC_REQUIRE(t && h && S_out && C_out, "trig_sums_fft: NULL argument");
    PDC_REQUIRE(n >= 1 && nf >= 1, "trig_sums_fft: need at least one sample and one frequency");
    HostCall hc(device);
    const int64_t nfft = fft_length(nf);
    double tmin = t[0], tmax = t[0];
    bool sorted = t[0] == t[0];
    for (int64_t i = 1; i < n; ++i) {
        tmin = t[i] < tmin ? t[i] : tmin;
        tmax = t[i] > tmax ? t[i] : tmax;
        sorted = sorted && t[i] >= t[i - 1];
    }
    const double scal_host[8] = {0.0, 0.0, tmin, tmax, sorted ? 1.0 : 0.0, 0.0, 0.0, 0.0};
    double *d_t = hc.in(SLOT_IN0, t, n * 8), *d_h = hc.in(SLOT_IN1, h, n * 8);
    double *d_s = hc.out<double>(SLOT_OUT0, nf * 8), *d_c = hc.out<double>(SLOT_OUT1, nf * 8);
    const FftLayout L = fft_layout(0, sizeof(scal_host), 1, nfft);   // one curve, one grid, the caller's weights
    char *base = hc.out<char>(SLOT_WORK, L.total);
    PDC_TRY(hc.status);
    double *scal = reinterpret_cast<double *>(base + L.scal);
    hc.put(scal, scal_host, sizeof(scal_host));
    PDC_TRY(fft_pipeline(hc.stream(), ExtirpArgs{d_t, d_h, d_h, nullptr, n, 0, 1, 0, 1, nfft, df, fmin, reinterpret_cast<double *>(base + L.grids)},
                         1, n, reinterpret_cast<cplx *>(base + L.scratch), false,
                         FftEpiArgs{nullptr, 0, 0, nf, d_s, d_c, scal, 0}));
    hc.back(S_out, d_s, nf * 8);
    hc.back(C_out, d_c, nf * 8);
    return hc.finish();
}

}  // extern "C"
