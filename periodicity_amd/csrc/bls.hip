// Box least squares (Kovacs, Zucker & Mazeh 2002, A&A 391, 369): the search for a box-shaped dip - a transit, a detached
// eclipse - as the best two-level model of the folded curve, on gfx950.
//
// The reference has no such class: PARITY UNPINNED BY THE REFERENCE.  The weights and the centring are those of GLS
// (w = err^-2 / sum err^-2, y' = y - sum w y, YY = sum w y'^2), the phase is that of the other phase scans
// ((t / P) % 1, no time origin), and the bins are numpy's: [k / n_bins, (k + 1) / n_bins) with the double k / n_bins as
// the edge, phi == 1.0 in the last one.  Per trial period, over the boxes (start bin i, length L bins, wrapping past
// phase 1) with sums r = sum w, s = sum w y', c = count:
//     power = max SR / YY,  SR = s^2 / (r (1 - r)),   depth = -s / (r (1 - r)) of the maximising box,
// over the boxes with c >= min_points, N_b - c >= min_points, 0 < r < 1 (dips_only: s < 0); equal SR: the smaller L,
// then the smaller i.
//
// Deterministic by construction.  The prologue turns every sample into two 64-bit integers,
//     qw = llrint(w 2^60),   qs = llrint(w (y' / A) 2^60),   A = max |y'|,
// and the histograms, their prefix sums and the window sums are integer arithmetic: exact, whatever the order in which
// the atomic adds arrive and however the samples are split over workgroups.  |qs| <= qw + 1 and sum qw <= 2^60 + N / 2,
// so the prefix of the histogram extended by len_max <= n_bins - 1 wrap-around bins stays below 2^62.  A window sum is
// off by at most N 2^-61 on a scale where the total weight is 1.  Only SR and the depth are floating point.
//
// Decomposition
//   bls_prep_kernel     one workgroup: sum err^-2, weighted mean, A, YY, max |t|, the bad-input flag, and one 24-byte
//                       record {t, qw, qs} per sample.
//   bls_bin_kernel      grid (n_periods, slices): one workgroup bins one slice of the samples for one trial period into
//                       ONE histogram in LDS shared by its threads (lane = sample, three LDS atomic adds per sample).
//                       slices == 1: the workgroup goes on to search its own histogram.  slices > 1: it adds the
//                       histogram to a zeroed global one, and
//   bls_search_kernel   (one workgroup per period) reads that one back and searches it.
//   bls_search          the search both routes share: prefix sums of the extended histogram, the windows dealt to the
//                       threads, admissibility on the integers, a max-reduction that carries the (L, i) key.
#include "pdc_internal.h"
#include "gls_sums.h"

#include <climits>
#include <cmath>

using namespace pdc;

namespace {

constexpr int kBlock = 256;
constexpr int kPrepBlock = 1024;
constexpr int kMaxBins = 2048;
constexpr int kMaxSlices = 1024;
constexpr double kScale = 1152921504606846976.0;   // 2^60

struct BlsRec {
    double t;
    long long qw, qs;
};

struct BlsPrepArgs {
    const double *t, *y, *dy;
    int64_t n;
    BlsRec *rec;    // [n]
    double *scal;   // {YY, A, max |t|, bad}
};

struct BlsArgs {
    const BlsRec *rec;
    const double *scal;
    int64_t n, z_len;   // z_len: samples per slice
    const double *periods;
    int n_bins, len_min, len_max, min_points, dips_only;
    unsigned long long *gr, *gs;   // [n_periods][n_bins]       (slices > 1)
    unsigned *gc;                  // [n_periods][n_bins + 1]
    double *power, *depth;         // depth, start_bin, box_bins may be NULL
    int32_t *start_bin, *box_bins;
};

template <int BLOCK>
__device__ __forceinline__ double block_max(double v, double *lds_waves) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_down(v, o, 64);
        v = u > v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds_waves[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = lds_waves[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) r = lds_waves[w] > r ? lds_waves[w] : r;
    return r;
}

// ---- prologue: weights and centring as GLS takes them, then the fixed-point records -----------------------------------
__global__ __launch_bounds__(kPrepBlock) void bls_prep_kernel(BlsPrepArgs a) {
    __shared__ double red[kPrepBlock / 64];
    const int tid = threadIdx.x;
    double acc = 0.0, nbad = 0.0, tmax = 0.0;
    for (int64_t i = tid; i < a.n; i += kPrepBlock) {
        const double e = a.dy ? a.dy[i] : 1.0, at = __builtin_fabs(a.t[i]);
        const double iv = 1.0 / (e * e);
        acc += iv;
        const bool ok = at < HUGE_VAL && __builtin_fabs(a.y[i]) < HUGE_VAL && __builtin_fabs(e) < HUGE_VAL && e != 0.0 && iv < HUGE_VAL;
        nbad += ok ? 0.0 : 1.0;
        tmax = at > tmax ? at : tmax;
    }
    const double W = block_sum<kPrepBlock>(acc, red);
    nbad = block_sum<kPrepBlock>(nbad, red);
    tmax = block_max<kPrepBlock>(tmax, red);
    if (nbad != 0.0 || !(W > 0.0) || !(W < HUGE_VAL)) {   // (also n == 0) every output is NaN / -1: no record is read
        if (tid == 0) {
            a.scal[0] = __builtin_nan("");
            a.scal[1] = a.scal[2] = 0.0;
            a.scal[3] = 1.0;
        }
        return;
    }
    acc = 0.0;
    for (int64_t i = tid; i < a.n; i += kPrepBlock) {
        acc += inv_var(a.dy, i) / W * a.y[i];
    }
    const double ybar = block_sum<kPrepBlock>(acc, red);
    double amax = 0.0;
    for (int64_t i = tid; i < a.n; i += kPrepBlock) {
        const double d = __builtin_fabs(a.y[i] - ybar);
        amax = d > amax ? d : amax;
    }
    const double A = block_max<kPrepBlock>(amax, red);
    double yy = 0.0;
    for (int64_t i = tid; i < a.n; i += kPrepBlock) {
        const double w = inv_var(a.dy, i) / W;
        const double yc = a.y[i] - ybar;
        yy += (w * yc) * yc;
        BlsRec r;
        r.t = a.t[i];
        r.qw = __builtin_llrint(w * kScale);
        r.qs = A > 0.0 ? __builtin_llrint(w * (yc / A) * kScale) : 0;
        a.rec[i] = r;
    }
    yy = block_sum<kPrepBlock>(yy, red);
    if (tid == 0) {
        a.scal[0] = yy;
        a.scal[1] = A;
        a.scal[2] = tmax;
        a.scal[3] = (yy > 0.0 && yy < HUGE_VAL && A > 0.0 && A < HUGE_VAL) ? 0.0 : 1.0;   // a constant y has no periodogram
    }
}

__device__ __forceinline__ void bls_write(const BlsArgs &a, int64_t p, double power, double depth, int start, int len) {
    a.power[p] = power;
    if (a.depth) a.depth[p] = depth;
    if (a.start_bin) a.start_bin[p] = start;
    if (a.box_bins) a.box_bins[p] = len;
}

// LDS of a workgroup: the histogram hr | hs [n_bins], hc [n_bins + 1] (the extra counter: samples whose phase is NaN),
// and - where the workgroup searches - the prefix sums pr | ps | pc [n_bins + len_max + 1].
struct BlsLds {
    long long *hr, *hs, *pr, *ps;
    unsigned *hc, *pc;
};
__device__ __forceinline__ BlsLds bls_lds(unsigned char *raw, int nb, int len_max, bool search) {
    const int m1 = search ? nb + len_max + 1 : 0;
    BlsLds l;
    l.hr = reinterpret_cast<long long *>(raw);
    l.hs = l.hr + nb;
    l.pr = l.hs + nb;
    l.ps = l.pr + m1;
    l.hc = reinterpret_cast<unsigned *>(l.ps + m1);
    l.pc = l.hc + nb + 1;
    return l;
}
size_t bls_lds_bytes(int nb, int len_max, bool search) {
    const size_t m1 = search ? (size_t)nb + len_max + 1 : 0;
    return (size_t)nb * 16 + m1 * 16 + ((size_t)nb + 1) * 4 + m1 * 4;
}
constexpr int kMaxLds = kMaxBins * 16 + 4096 * 16 + (kMaxBins + 1) * 4 + 4096 * 4;   // 122 884 B of the CU's 160 KiB

// ---- the search: run by the NT threads of a workgroup on the histogram of trial period p in LDS ---------------------
template <int NT>
__device__ void bls_search(const BlsArgs &a, const int64_t p, const BlsLds &l) {
    __shared__ long long w_r[NT / 64], w_s[NT / 64];
    __shared__ unsigned w_c[NT / 64];
    __shared__ double b_v[NT / 64];
    __shared__ int b_k[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nb = a.n_bins;
    if (l.hc[nb] != 0u) {   // a NaN phase (period 0 or NaN): this period only
        if (tid == 0) bls_write(a, p, __builtin_nan(""), __builtin_nan(""), -1, -1);
        return;
    }
    // prefix sums of the histogram extended by len_max wrap-around bins: thread `tid` owns a run of `chunk` entries
    const int M = nb + a.len_max, chunk = (M + NT - 1) / NT;
    const int b = tid * chunk < M ? tid * chunk : M, e = b + chunk < M ? b + chunk : M;
    long long ar = 0, as = 0;
    unsigned ac = 0u;
    for (int k = b; k < e; ++k) {
        const int j = k < nb ? k : k - nb;
        ar += l.hr[j];
        as += l.hs[j];
        ac += l.hc[j];
    }
    long long ir = ar, is = as;
    unsigned ic = ac;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long ur = __shfl_up(ir, o, 64), us = __shfl_up(is, o, 64);
        const unsigned uc = __shfl_up(ic, o, 64);
        if (lane >= o) {
            ir += ur;
            is += us;
            ic += uc;
        }
    }
    if (lane == 63) {
        w_r[wv] = ir;
        w_s[wv] = is;
        w_c[wv] = ic;
    }
    __syncthreads();
    long long run_r = ir - ar, run_s = is - as;
    unsigned run_c = ic - ac;
    for (int w = 0; w < wv; ++w) {
        run_r += w_r[w];
        run_s += w_s[w];
        run_c += w_c[w];
    }
    if (tid == 0) {
        l.pr[0] = 0;
        l.ps[0] = 0;
        l.pc[0] = 0u;
    }
    for (int k = b; k < e; ++k) {
        const int j = k < nb ? k : k - nb;
        run_r += l.hr[j];
        run_s += l.hs[j];
        run_c += l.hc[j];
        l.pr[k + 1] = run_r;
        l.ps[k + 1] = run_s;
        l.pc[k + 1] = run_c;
    }
    __syncthreads();

    // the windows: thread `tid` takes the start bins tid, tid + NT, ... at every length
    const long long r_total = l.pr[nb], n_total = (long long)l.pc[nb], min_points = a.min_points;
    double best = -1.0;
    int key = INT_MAX;   // L * 4096 + i of `best`: among equal SR the smaller L, then the smaller i
    for (int i = tid; i < nb; i += NT) {
        const long long r0 = l.pr[i], s0 = l.ps[i];
        const unsigned c0 = l.pc[i];
        for (int L = a.len_min; L <= a.len_max; ++L) {
            const long long R = l.pr[i + L] - r0, S = l.ps[i + L] - s0, c = (long long)(unsigned)(l.pc[i + L] - c0);
            const long long Rc = r_total - R;   // 1 - r, from the integers
            if (c >= min_points && n_total - c >= min_points && R > 0 && Rc > 0 && (!a.dips_only || S < 0)) {
                const double sd = (double)S;
                const double v = sd * sd / ((double)R * (double)Rc);
                const int k = L * 4096 + i;
                if (v > best || (v == best && k < key)) {
                    best = v;
                    key = k;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(best, o, 64);
        const int ok = __shfl_down(key, o, 64);
        if (ov > best || (ov == best && ok < key)) {
            best = ov;
            key = ok;
        }
    }
    if (lane == 0) {
        b_v[wv] = best;
        b_k[wv] = key;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < NT / 64; ++w)
        if (b_v[w] > best || (b_v[w] == best && b_k[w] < key)) {
            best = b_v[w];
            key = b_k[w];
        }
    if (key == INT_MAX) {   // no admissible box
        bls_write(a, p, __builtin_nan(""), __builtin_nan(""), -1, -1);
        return;
    }
    const int L = key >> 12, i = key & 4095;
    const double YY = a.scal[0], A = a.scal[1];
    const long long R = l.pr[i + L] - l.pr[i], S = l.ps[i + L] - l.ps[i];
    const double sd = (double)S, den = (double)R * (double)(r_total - R);
    // s = A S 2^-60, r = R 2^-60, 1 - r = Rc 2^-60
    bls_write(a, p, (sd * sd / den) * (A * A) / YY, -A * (sd / den * kScale), i, L);
}

// ---- binning --------------------------------------------------------------------------------------------------------
// FUSED: slices == 1, the workgroup bins every sample of its trial period and searches.
template <bool FUSED>
__global__ __launch_bounds__(kBlock) void bls_bin_kernel(BlsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, nb = a.n_bins;
    const int64_t p = blockIdx.x;
    const BlsLds l = bls_lds(lds_raw, nb, a.len_max, FUSED);
    if (a.scal[3] != 0.0) {   // bad input: every output is NaN / -1 (bls_search_kernel writes them on the other route)
        if (FUSED && tid == 0) bls_write(a, p, __builtin_nan(""), __builtin_nan(""), -1, -1);
        return;
    }
    for (int k = tid; k < nb; k += kBlock) {
        l.hr[k] = 0;
        l.hs[k] = 0;
    }
    for (int k = tid; k <= nb; k += kBlock) l.hc[k] = 0u;
    __syncthreads();

    const double period = a.periods[p];
    const double rp = 1.0 / period, dm0 = (double)nb;
    // the fast path of pdm_chunks.inc: u = frac(t * rp) * n_bins against the exact ((t / period) % 1) and the edges
    // k / n_bins, in units of u: quotient error <= 1.5 ulp(q) <= 3.4e-16 |q|, product / edge roundings 2.3e-16 n_bins;
    // doubled for safety.  A bin is accepted only when u is provably that far from every integer.
    const double eps = dm0 * (8.9e-16 * a.scal[2] * __builtin_fabs(rp) + 8.9e-16);
    const double thr = 0.5 - eps;
    const int64_t s_begin = FUSED ? 0 : (int64_t)blockIdx.y * a.z_len;
    const int64_t s_end = FUSED ? a.n : (s_begin + a.z_len < a.n ? s_begin + a.z_len : a.n);
    for (int64_t g = s_begin + tid; g < s_end; g += kBlock) {
        const BlsRec r = a.rec[g];
        const double u = __builtin_amdgcn_fract(r.t * rp) * dm0;
        int k = (int)u;
        if (!(__builtin_fabs(__builtin_amdgcn_fract(u) - 0.5) < thr)) {
            // exact path: numpy's float remainder of the IEEE quotient, explicit edges
            const double qe = r.t / period;
            const double phi = qe - __builtin_floor(qe);
            if (phi != phi) {   // poisons the period
                atomicAdd(&l.hc[nb], 1u);
                continue;
            }
            k = (int)(phi * dm0);
            k = k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);
            while (k > 0 && phi < (double)k / dm0) --k;
            while (k < nb - 1 && phi >= (double)(k + 1) / dm0) ++k;   // phi == 1.0 stays in the last bin
        }
        k = k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);   // (never taken: the index of an LDS atomic is kept in bounds anyway)
        atomicAdd(reinterpret_cast<unsigned long long *>(&l.hr[k]), (unsigned long long)r.qw);
        atomicAdd(reinterpret_cast<unsigned long long *>(&l.hs[k]), (unsigned long long)r.qs);
        atomicAdd(&l.hc[k], 1u);
    }
    __syncthreads();
    if (FUSED) {
        bls_search<kBlock>(a, p, l);
        return;
    }
    // integer adds commute: the global histogram does not depend on the order in which the slices arrive
    for (int k = tid; k < nb; k += kBlock) {
        const unsigned long long vr = (unsigned long long)l.hr[k], vs = (unsigned long long)l.hs[k];
        if (vr) atomicAdd(&a.gr[p * nb + k], vr);
        if (vs) atomicAdd(&a.gs[p * nb + k], vs);
    }
    for (int k = tid; k <= nb; k += kBlock) {
        const unsigned vc = l.hc[k];
        if (vc) atomicAdd(&a.gc[p * (nb + 1) + k], vc);
    }
}

__global__ __launch_bounds__(kBlock) void bls_search_kernel(BlsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, nb = a.n_bins;
    const int64_t p = blockIdx.x;
    const BlsLds l = bls_lds(lds_raw, nb, a.len_max, true);
    if (a.scal[3] != 0.0) {
        if (tid == 0) bls_write(a, p, __builtin_nan(""), __builtin_nan(""), -1, -1);
        return;
    }
    for (int k = tid; k < nb; k += kBlock) {
        l.hr[k] = (long long)a.gr[p * nb + k];
        l.hs[k] = (long long)a.gs[p * nb + k];
    }
    for (int k = tid; k <= nb; k += kBlock) l.hc[k] = a.gc[p * (nb + 1) + k];
    __syncthreads();
    bls_search<kBlock>(a, p, l);
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct BlsParams {
    int n_bins, len_min, len_max, min_points, dips_only, slices;
};

int bls_validate(const char *what, int64_t n, int64_t n_periods, const BlsParams &q) {
    PDC_REQUIRE(n >= 0 && n_periods >= 0, "%s: negative size", what);
    PDC_REQUIRE(n < ((int64_t)1 << 31) && n_periods < ((int64_t)1 << 31), "%s: at most 2^31 - 1 samples and trial periods", what);
    PDC_REQUIRE(q.n_bins >= 2 && q.n_bins <= kMaxBins, "%s: n_bins must be 2 .. %d (got %d)", what, kMaxBins, q.n_bins);
    PDC_REQUIRE(q.len_min >= 1 && q.len_min <= q.len_max && q.len_max <= q.n_bins - 1,
                "%s: box lengths need 1 <= len_min <= len_max <= n_bins - 1 (got %d .. %d of %d bins)", what, q.len_min,
                q.len_max, q.n_bins);
    PDC_REQUIRE(q.min_points >= 1, "%s: min_points must be at least 1 (got %d)", what, q.min_points);
    PDC_REQUIRE(q.slices >= 0 && q.slices <= kMaxSlices, "%s: slices must be 0 (chosen from the shape) .. %d (got %d)", what,
                kMaxSlices, q.slices);
    return PDC_OK;
}

int64_t bls_rec_bytes(int64_t n) { return up256((n > 0 ? n : 1) * (int64_t)sizeof(BlsRec)) + 256; }
int64_t bls_hist_bytes(int64_t n_periods, int n_bins) {
    return 2 * up256(n_periods * n_bins * 8) + up256(n_periods * (n_bins + 1) * 4);
}

// slices = 0.  One workgroup per trial period leaves a chip of 256 CUs short of work when the periods are few and the
// samples many: the samples are split until the grid has kTargetGroups workgroups, as long as a slice keeps
// kMinSlice samples (the constants: DESIGN.md 4.2b, profiles/r13_bls_timing.txt).
constexpr int64_t kTargetGroups = 2048;
constexpr int64_t kMinSlice = 4096;
int bls_auto_slices(int64_t n, int64_t n_periods) {
    int64_t s = (kTargetGroups + n_periods - 1) / n_periods;
    if (s > n / kMinSlice) s = n / kMinSlice;
    return (int)(s < 1 ? 1 : (s > kMaxSlices ? kMaxSlices : s));
}

// The route of one call: `slices` as asked for (0: from the shape; a split that does not fit `budget` falls back to one
// slice when it was chosen here, and is an error when the caller forced it), and the workspace it needs.
int bls_route(const char *what, int64_t n, int64_t n_periods, const BlsParams &q, int64_t budget, int *slices, int64_t *bytes) {
    int s = q.slices ? q.slices : bls_auto_slices(n, n_periods);
    if (n > 0 && s > n) s = (int)n;
    if (n == 0) s = 1;
    if (s > 1) {
        const int64_t total = bls_rec_bytes(n) + bls_hist_bytes(n_periods, q.n_bins);
        WorkScale ws(budget, [&] { return total; });
        if (!ws.fits() && !q.slices) s = 1;
        else PDC_REQUIRE_FITS(ws, what);
    }
    *slices = s;
    *bytes = bls_rec_bytes(n) + (s > 1 ? bls_hist_bytes(n_periods, q.n_bins) : 0);
    return PDC_OK;
}

int bls_enqueue(hipStream_t st, const double *d_t, const double *d_y, const double *d_dy, int64_t n, const double *d_periods,
                int64_t n_periods, const BlsParams &q, int slices, double *d_power, double *d_depth, int32_t *d_start,
                int32_t *d_box, void *work) {
    char *base = static_cast<char *>(work);
    BlsPrepArgs pa;
    pa.t = d_t;
    pa.y = d_y;
    pa.dy = d_dy;
    pa.n = n;
    pa.rec = reinterpret_cast<BlsRec *>(base);
    pa.scal = reinterpret_cast<double *>(base + bls_rec_bytes(n) - 256);
    hipLaunchKernelGGL(bls_prep_kernel, dim3(1), dim3(kPrepBlock), 0, st, pa);
    PDC_HIP(hipGetLastError());
    BlsArgs a;
    a.rec = pa.rec;
    a.scal = pa.scal;
    a.n = n;
    a.z_len = (n + slices - 1) / slices;
    a.periods = d_periods;
    a.n_bins = q.n_bins;
    a.len_min = q.len_min;
    a.len_max = q.len_max;
    a.min_points = q.min_points;
    a.dips_only = q.dips_only;
    a.gr = a.gs = nullptr;
    a.gc = nullptr;
    a.power = d_power;
    a.depth = d_depth;
    a.start_bin = d_start;
    a.box_bins = d_box;
    const size_t lds_search = bls_lds_bytes(q.n_bins, q.len_max, true);
    if (slices == 1) {
        PDC_TRY(allow_dynamic_lds((const void *)bls_bin_kernel<true>, kMaxLds));
        hipLaunchKernelGGL(bls_bin_kernel<true>, dim3((unsigned)n_periods), dim3(kBlock), lds_search, st, a);
        PDC_HIP(hipGetLastError());
        return PDC_OK;
    }
    // The global histogram is zeroed on the stream in EVERY call: the workspace is reused between calls (see the note on
    // reused workspaces at stream_scratch in pdc_internal.h), and the adds below start from what they find.
    char *hist = base + bls_rec_bytes(n);
    const int64_t plane = up256(n_periods * q.n_bins * 8);
    PDC_HIP(hipMemsetAsync(hist, 0, bls_hist_bytes(n_periods, q.n_bins), st));
    a.gr = reinterpret_cast<unsigned long long *>(hist);
    a.gs = reinterpret_cast<unsigned long long *>(hist + plane);
    a.gc = reinterpret_cast<unsigned *>(hist + 2 * plane);
    hipLaunchKernelGGL(bls_bin_kernel<false>, dim3((unsigned)n_periods, (unsigned)slices), dim3(kBlock),
                       bls_lds_bytes(q.n_bins, q.len_max, false), st, a);
    PDC_HIP(hipGetLastError());
    PDC_TRY(allow_dynamic_lds((const void *)bls_search_kernel, kMaxLds));
    hipLaunchKernelGGL(bls_search_kernel, dim3((unsigned)n_periods), dim3(kBlock), lds_search, st, a);
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

}  // namespace

extern "C" {

int pdc_bls_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                     const double *d_periods, int64_t n_periods, int n_bins, int len_min, int len_max, int min_points,
                     int dips_only, int slices, double *d_power, double *d_depth, int32_t *d_start_bin, int32_t *d_box_bins) {
    const BlsParams q = {n_bins, len_min, len_max, min_points, dips_only ? 1 : 0, slices};
    PDC_TRY(bls_validate("bls", n, n_periods, q));
    PDC_REQUIRE((d_t && d_y) || n == 0, "bls: NULL argument");
    PDC_REQUIRE((d_periods && d_power) || n_periods == 0, "bls: NULL argument");
    if (n_periods == 0) return PDC_OK;
    PDC_TRY(use_device(device));
    int s = 1;
    int64_t bytes = 0;
    PDC_TRY(bls_route("bls", n, n_periods, q, work_budget(), &s, &bytes));
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    PDC_TRY(stream_scratch(device, st, bytes, &work));
    ScratchPin pin;
    pin.device = device;
    pin.stream = st;
    pin.held = true;
    return bls_enqueue(st, d_t, d_y, d_dy, n, d_periods, n_periods, q, s, d_power, d_depth, d_start_bin, d_box_bins, work);
}

int pdc_bls_scan(const double *t, const double *y, const double *dy, int64_t n, const double *periods, int64_t n_periods,
                 int n_bins, int len_min, int len_max, int min_points, int dips_only, int slices, double *power,
                 double *depth, int32_t *start_bin, int32_t *box_bins, int device) {
    const BlsParams q = {n_bins, len_min, len_max, min_points, dips_only ? 1 : 0, slices};
    PDC_TRY(bls_validate("bls", n, n_periods, q));
    PDC_REQUIRE((t && y) || n == 0, "bls: NULL argument");
    PDC_REQUIRE((periods && power) || n_periods == 0, "bls: NULL argument");
    if (n_periods == 0) return PDC_OK;
    PDC_TRY(use_device(device));
    DeviceLock lock(device);
    int s = 1;
    int64_t bytes = 0;
    PDC_TRY(bls_route("bls", n, n_periods, q, host_work_budget(device), &s, &bytes));
    const int64_t nn = n > 0 ? n : 1, ints = up256(n_periods * 4);
    void *d_t, *d_y, *d_dy = nullptr, *d_per, *d_power, *d_depth, *d_int, *d_work;
    PDC_TRY(cached(device, SLOT_IN0, nn * 8, &d_t));
    PDC_TRY(cached(device, SLOT_IN1, nn * 8, &d_y));
    if (dy) PDC_TRY(cached(device, SLOT_IN2, nn * 8, &d_dy));
    PDC_TRY(cached(device, SLOT_IN3, n_periods * 8, &d_per));
    PDC_TRY(cached(device, SLOT_OUT0, n_periods * 8, &d_power));
    PDC_TRY(cached(device, SLOT_OUT1, n_periods * 8, &d_depth));
    PDC_TRY(cached(device, SLOT_OUT2, 2 * ints, &d_int));
    PDC_TRY(cached(device, SLOT_WORK, bytes, &d_work));
    int32_t *d_start = static_cast<int32_t *>(d_int), *d_box = reinterpret_cast<int32_t *>(static_cast<char *>(d_int) + ints);
    hipStream_t st = nullptr;
    PDC_TRY(host_stream(device, &st));
    if (n > 0) {
        PDC_HIP(hipMemcpyAsync(d_t, t, n * 8, hipMemcpyHostToDevice, st));
        PDC_HIP(hipMemcpyAsync(d_y, y, n * 8, hipMemcpyHostToDevice, st));
        if (dy) PDC_HIP(hipMemcpyAsync(d_dy, dy, n * 8, hipMemcpyHostToDevice, st));
    }
    PDC_HIP(hipMemcpyAsync(d_per, periods, n_periods * 8, hipMemcpyHostToDevice, st));
    PDC_TRY(bls_enqueue(st, (double *)d_t, (double *)d_y, (double *)d_dy, n, (double *)d_per, n_periods, q, s,
                        (double *)d_power, (double *)d_depth, d_start, d_box, d_work));
    PDC_HIP(hipMemcpyAsync(power, d_power, n_periods * 8, hipMemcpyDeviceToHost, st));
    if (depth) PDC_HIP(hipMemcpyAsync(depth, d_depth, n_periods * 8, hipMemcpyDeviceToHost, st));
    if (start_bin) PDC_HIP(hipMemcpyAsync(start_bin, d_start, n_periods * 4, hipMemcpyDeviceToHost, st));
    if (box_bins) PDC_HIP(hipMemcpyAsync(box_bins, d_box, n_periods * 4, hipMemcpyDeviceToHost, st));
    PDC_HIP(hipStreamSynchronize(st));
    return PDC_OK;
}

}  // extern "C"
