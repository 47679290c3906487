// Morlet wavelet power spectrum of an evenly sampled curve (timefrequency.WPS) on gfx950: PyWavelets' published `cwt`
// algorithm - the integrated wavelet tabulated on 1024 points, resampled per scale into a filter h of L entries,
// convolve, diff, centred cut - evaluated as an exact gather-sum.  Definitions: periodicity_hip.h.
//
// PyWavelets is not a dependency and the reference only calls it: PARITY UNPINNED BY THE REFERENCE.
//
// Identity.  With h[-1] = h[L] = 0 and x zero outside [0, N):
//     coef[n] = -sqrt(s) sum_{k = 0 .. L} (h[k] - h[k-1]) x[n + floor(L / 2) - k].
// h is a step function of the table, h[k] = int_psi[j[L-1-k]], j[m] = trunc(m / (s step)), so the difference is not zero
// at no more than 1025 positions whatever the scale: in filter position m = L - k, at m = 0, at m = L and wherever
// j[m] != j[m-1].  These are the TAPS of a scale: (m, -sqrt(s) (int_psi[j[m-1]] - int_psi[j[m]])), entries outside the
// filter 0.  No prefix sums, no cancellation, no FFT.
//
// Decomposition
//   wps_taps_kernel   one workgroup of 1024 threads per scale, thread q: the first position whose table entry is >= q,
//                     found from ceil(q s step) and corrected with the SAME division numpy makes, so the change points
//                     are numpy's bit for bit; kept when the entry is attained; a ballot prefix packs the taps in
//                     ascending position.  (wps_first() also runs on the host: pdc_wps_taps, for tests without a GPU.)
//   wps_scan_kernel   blockIdx = (tile of kTile consecutive time indices, chunk of scales).  Per scale the taps are cut
//                     into groups that reach at most kExtra positions; the workgroup stages the kTile + reach samples
//                     the group needs into LDS (zeros outside the curve; a group whose window misses the curve adds
//                     exact zeros and is skipped), then every lane accumulates re and im of its kOut outputs, one LDS
//                     read and two fma per (tap, output), weights and offsets from scalar loads.  Taps in ascending
//                     position whatever the grouping: one summation order per cell.  Epilogue |c|^2 / s, the planes
//                     where taken, the cone-of-influence mask, the row partial of the (scale, tile) by a fixed tree and
//                     the column partials of the chunk in registers.
//   wps_fold_kernel   rows: the tiles in ascending order; columns: the chunks in ascending order; means and masked
//                     means (NaN where nothing is eligible) with their counts.
// No atomics: the same bits from call to call.
#include "pdc_internal.h"

#include <cmath>

using namespace pdc;

namespace {

constexpr int kBlock = 256;
constexpr int kOut = 4;                   // outputs per lane (the LDS read rate sets the pace, not kOut)
constexpr int kTile = kBlock * kOut;      // time indices per workgroup
constexpr int kExtra = 1024;              // filter positions one staged window reaches beyond the tile
constexpr int kWindow = kTile + kExtra;   // doubles of LDS
constexpr int kTable = 1024;              // entries of the wavelet table
constexpr int kPitch = 1032;              // tap slots per scale (at most kTable + 1 are used)
constexpr int kTapBlock = 1024;
constexpr int kChunk = 8;                 // scales per chunk, unless PDC_WORK_BUDGET_GB asks for fewer column partials
constexpr double kMaxScale = 16777216.0;  // 2^24: positions stay below 2^31

struct WpsScale {
    double s;
    int64_t L;
    int64_t ntaps;
};

// ---- the resampling rule, host and device ------------------------------------------------------------------------------
// The unit is compiled with -ffp-contract=off: every operation below rounds once, as numpy's.
// j[m] of `(np.arange(...) / (s * step)).astype(int)`
__host__ __device__ inline int64_t wps_entry(int64_t m, double d) { return (int64_t)((double)m / d); }

// d = s * step and M = len(np.arange(s * span + 1)); false where the scale cannot be served
__host__ __device__ inline bool wps_shape(double s, double step, double span, double *d, int64_t *M) {
    if (!(s >= 1.0 / 64.0 && s <= kMaxScale)) return false;
    *d = s * step;
    *M = (int64_t)ceil(s * span + 1.0);
    return *d > 0.0 && *M >= 1 && *M < ((int64_t)1 << 31) && (double)*M / *d < 1e9;
}

// the first position m in [0, M] with j[m] >= q (M: none)
__host__ __device__ inline int64_t wps_first(int q, double d, int64_t M) {
    int64_t m = (int64_t)ceil((double)q * d);
    m = m < 0 ? 0 : (m > M ? M : m);
    while (m > 0 && wps_entry(m - 1, d) >= q) --m;
    while (m < M && wps_entry(m, d) < q) ++m;
    return m;
}

// L = len(j[j < 1024])
__host__ __device__ inline int64_t wps_length(double d, int64_t M) { return wps_first(kTable, d, M); }

// ---- taps --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTapBlock) void wps_taps_kernel(const double *scales, const double2 *table, double step,
                                                              double span, WpsScale *rec, int32_t *off, double2 *w) {
    __shared__ int wave_count[kTapBlock / 64];
    const int64_t i = blockIdx.x;
    const int q = threadIdx.x, lane = q & 63, wave = q >> 6;
    const double s = scales[i];
    double d = 1.0;
    int64_t M = 0;
    const bool ok = wps_shape(s, step, span, &d, &M);
    const int64_t L = ok ? wps_length(d, M) : 0;
    const double nsqrt = -__builtin_sqrt(s);
    const int64_t m = ok ? wps_first(q, d, M) : 0;
    const bool tap = ok && m < L && wps_entry(m, d) == q;
    double2 wt = make_double2(0.0, 0.0);
    if (tap) {
        const double2 after = table[q];
        double2 before = make_double2(0.0, 0.0);
        if (m > 0) before = table[wps_entry(m - 1, d)];
        wt = make_double2(nsqrt * (before.x - after.x), nsqrt * (before.y - after.y));
    }
    const unsigned long long votes = __ballot(tap);
    if (lane == 0) wave_count[wave] = __popcll(votes);
    __syncthreads();
    int at = __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
    for (int v = 0; v < kTapBlock / 64; ++v) {
        if (v < wave) at += wave_count[v];
        total += wave_count[v];
    }
    off += i * kPitch;
    w += i * kPitch;
    if (tap) {
        off[at] = (int32_t)m;
        w[at] = wt;
    }
    if (q == 0) {
        int64_t ntaps = 0;
        if (ok && L >= 1) {   // the filter's far edge: position L, the last entry against nothing
            const double2 before = table[wps_entry(L - 1, d)];
            off[total] = (int32_t)L;
            w[total] = make_double2(nsqrt * before.x, nsqrt * before.y);
            ntaps = total + 1;
        }
        rec[i].s = s;
        rec[i].L = L;
        rec[i].ntaps = ntaps;
    }
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
struct WpsRowPart {   // one (scale, tile)
    double sum, masked;
    int64_t count;
};

struct WpsArgs {
    const double *t, *periods;
    const WpsScale *rec;
    int64_t n, n_scales, tiles, chunks, chunk;
    double corr, t_min, t_max;
    double *spectrum;       // [n_scales][n] | NULL
    double2 *coefs;         // [n_scales][n] | NULL
    WpsRowPart *part_row;   // [n_scales][tiles]
    double *part_col;       // [chunks][2][n]: sum, masked sum
    double *gwps, *masked_gwps, *sav, *masked_sav;   // outputs | NULL
    int64_t *gwps_count, *sav_count;
};

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// min(t - t_min, t_max - t) as np.minimum of the two differences (finite times)
__device__ __forceinline__ double coi_edge(const WpsArgs &a, int64_t n) {
    const double tn = a.t[n];
    return __builtin_fmin(tn - a.t_min, a.t_max - tn);
}

// A lane's kOut samples of one tap, kBlock doubles apart, as four ds_read_b64 (256 B/clk/CU, the rate that keeps pace
// with two fma per read).  Written out because the compiler merges the four into two ds_read2st64_b64, which run at
// half that rate.  The values count as defined only behind lds_wait4, which every use goes through.
static_assert(kOut == 4 && kBlock * 8 == 2048, "lds_read4 spells the strides out");
__device__ __forceinline__ void lds_read4(double (&v)[kOut], unsigned addr) {
    asm volatile("ds_read_b64 %0, %4\n\tds_read_b64 %1, %4 offset:2048\n\tds_read_b64 %2, %4 offset:4096\n\t"
                 "ds_read_b64 %3, %4 offset:6144"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
                 : "v"(addr)
                 : "memory");
}
__device__ __forceinline__ void lds_wait4(double (&v)[kOut]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
}
__device__ __forceinline__ void tap_fma(double (&re)[kOut], double (&im)[kOut], const double2 wt, const double (&v)[kOut]) {
#pragma unroll
    for (int r = 0; r < kOut; ++r) {
        re[r] = __builtin_fma(wt.x, v[r], re[r]);
        im[r] = __builtin_fma(wt.y, v[r], im[r]);
    }
}

// offs, wts and x are read through scalar or read-only loads: restrict tells the compiler that the kernel's stores (the
// planes, the partials) do not touch them.
__global__ __launch_bounds__(kBlock) void wps_scan_kernel(WpsArgs a, const int32_t *__restrict__ offs,
                                                           const double2 *__restrict__ wts,
                                                           const double *__restrict__ x) {
    __shared__ double win[kWindow];
    __shared__ double red_sum[kBlock / 64], red_masked[kBlock / 64];
    __shared__ long long red_count[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    typedef __attribute__((address_space(3))) double *LdsPointer;
    const unsigned lds_lane = (unsigned)(uintptr_t)(LdsPointer)win + (unsigned)tid * 8u;   // this lane's win[tid]
    const int64_t tile = blockIdx.x;
    const int64_t n0 = tile * kTile;
    const int64_t i0 = (int64_t)blockIdx.y * a.chunk;
    const int64_t i1 = i0 + a.chunk < a.n_scales ? i0 + a.chunk : a.n_scales;

    double edge[kOut], col[kOut], mcol[kOut];
#pragma unroll
    for (int r = 0; r < kOut; ++r) {
        const int64_t n = n0 + r * kBlock + tid;
        edge[r] = n < a.n ? coi_edge(a, n) : 0.0;
        col[r] = mcol[r] = 0.0;
    }

    for (int64_t i = i0; i < i1; ++i) {
        const double s = a.rec[i].s;
        const int64_t L = a.rec[i].L;
        const int ntaps = (int)a.rec[i].ntaps;
        const int32_t *off = offs + i * kPitch;
        const double2 *w = wts + i * kPitch;
        const int64_t base = n0 - (L + 1) / 2;   // the sample that position 0 pairs with output n0
        double re[kOut], im[kOut];
#pragma unroll
        for (int r = 0; r < kOut; ++r) re[r] = im[r] = 0.0;

        for (int ta = 0; ta < ntaps;) {
            const int m_a = off[ta];
            int lo = ta + 1, len = ntaps - lo;   // tb: the first tap past the window's reach
            while (len > 0) {
                const int half = len >> 1;
                if (off[lo + half] - m_a <= kExtra) {
                    lo += half + 1;
                    len -= half + 1;
                } else {
                    len = half;
                }
            }
            const int tb = lo;
            const int reach = off[tb - 1] - m_a;   // <= kExtra
            const int64_t g0 = base + m_a;         // the sample in win[0]
            if (g0 + kTile + reach > 0 && g0 < a.n) {
                __syncthreads();   // the last group's reads are done
                for (int p = tid; p < kTile + reach; p += kBlock) {
                    const int64_t g = g0 + p;
                    win[p] = g >= 0 && g < a.n ? x[g] : 0.0;
                }
                __syncthreads();
                // Four taps a trip, the next tap's reads in flight behind this tap's fma.  A trip past the group's end
                // repeats its last tap with weight 0: fma(0, v, acc) is acc.
                for (int tp = ta; tp < tb; tp += 4) {
                    unsigned at[4];
                    double2 wt[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int q = tp + u < tb ? tp + u : tb - 1;
                        at[u] = lds_lane + (unsigned)(off[q] - m_a) * 8u;
                        wt[u] = tp + u < tb ? w[q] : make_double2(0.0, 0.0);
                    }
                    double va[kOut], vb[kOut];
                    lds_read4(va, at[0]);
                    lds_wait4(va);
                    lds_read4(vb, at[1]);
                    tap_fma(re, im, wt[0], va);
                    lds_wait4(vb);
                    lds_read4(va, at[2]);
                    tap_fma(re, im, wt[1], vb);
                    lds_wait4(va);
                    lds_read4(vb, at[3]);
                    tap_fma(re, im, wt[2], va);
                    lds_wait4(vb);
                    tap_fma(re, im, wt[3], vb);
                }
            }
            ta = tb;
        }

        // Epilogue: |c|^2 / s, the mask as numpy evaluates it, the row partial of this (scale, tile).
        const double reach_coi = a.corr * a.periods[i];
        double sum = 0.0, masked = 0.0;
        long long count = 0;
#pragma unroll
        for (int r = 0; r < kOut; ++r) {
            const int64_t n = n0 + r * kBlock + tid;
            if (n < a.n) {
                const double p = (re[r] * re[r] + im[r] * im[r]) / s;
                if (a.spectrum) a.spectrum[i * a.n + n] = p;
                if (a.coefs) a.coefs[i * a.n + n] = make_double2(re[r], im[r]);
                sum += p;
                col[r] += p;
                if (reach_coi < edge[r]) {
                    masked += p;
                    mcol[r] += p;
                    ++count;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_down(sum, o, 64);
            masked += __shfl_down(masked, o, 64);
            count += __shfl_down(count, o, 64);
        }
        __syncthreads();   // the last scale's partial has been read
        if (lane == 0) {
            red_sum[wave] = sum;
            red_masked[wave] = masked;
            red_count[wave] = count;
        }
        __syncthreads();
        if (tid == 0) {
            WpsRowPart part = {0.0, 0.0, 0};
            for (int v = 0; v < kBlock / 64; ++v) {
                part.sum += red_sum[v];
                part.masked += red_masked[v];
                part.count += red_count[v];
            }
            a.part_row[i * a.tiles + tile] = part;
        }
    }

    double *pc = a.part_col + (int64_t)blockIdx.y * 2 * a.n;
#pragma unroll
    for (int r = 0; r < kOut; ++r) {
        const int64_t n = n0 + r * kBlock + tid;
        if (n < a.n) {
            pc[n] = col[r];
            pc[a.n + n] = mcol[r];
        }
    }
}

// ---- marginals ---------------------------------------------------------------------------------------------------------
// Threads [0, n_scales): a row each, its tiles in ascending order; threads [n_scales, n_scales + n): a column each, its
// chunks in ascending order, and the column's count from the mask itself.
__global__ __launch_bounds__(kBlock) void wps_fold_kernel(WpsArgs a) {
    const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (id < a.n_scales) {
        double sum = 0.0, masked = 0.0;
        int64_t count = 0;
        for (int64_t tile = 0; tile < a.tiles; ++tile) {
            const WpsRowPart part = a.part_row[id * a.tiles + tile];
            sum += part.sum;
            masked += part.masked;
            count += part.count;
        }
        if (a.gwps) a.gwps[id] = sum / (double)a.n;
        if (a.masked_gwps) a.masked_gwps[id] = count > 0 ? masked / (double)count : quiet_nan();
        if (a.gwps_count) a.gwps_count[id] = count;
        return;
    }
    const int64_t n = id - a.n_scales;
    if (n >= a.n) return;
    double sum = 0.0, masked = 0.0;
    for (int64_t c = 0; c < a.chunks; ++c) {
        sum += a.part_col[c * 2 * a.n + n];
        masked += a.part_col[(c * 2 + 1) * a.n + n];
    }
    const double edge = coi_edge(a, n);
    int64_t count = 0;
    for (int64_t i = 0; i < a.n_scales; ++i) count += a.corr * a.periods[i] < edge ? 1 : 0;
    if (a.sav) a.sav[n] = sum / (double)a.n_scales;
    if (a.masked_sav) a.masked_sav[n] = count > 0 ? masked / (double)count : quiet_nan();
    if (a.sav_count) a.sav_count[n] = count;
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct WpsDispatch {
    int64_t tiles, chunks, chunk, dense, sparse;
};
thread_local WpsDispatch g_last = {};

// scale records | tap positions | tap weights | row partials | column partials
struct WpsPlan {
    int64_t tiles, chunk, chunks, at_rec, at_off, at_w, at_row, at_col, total;
};

bool wps_sizes_ok(int64_t n, int64_t n_scales) {
    if (n < 1 || n_scales < 1 || n > ((int64_t)1 << 40) || n_scales > ((int64_t)1 << 24)) return false;
    return n_scales <= (((int64_t)1 << 56) / n);
}

// The column partials are the part that grows with both sizes: under PDC_WORK_BUDGET_GB a chunk takes twice the scales
// until they fit (fewer, longer workgroups; the columns' summation order follows the chunks).  At most 65535 chunks, the
// grid's second dimension.
WpsPlan wps_plan(int64_t n, int64_t n_scales) {
    WpsPlan p;
    p.tiles = (n + kTile - 1) / kTile;
    Carve c;
    p.at_rec = c.take(n_scales * (int64_t)sizeof(WpsScale));
    p.at_off = c.take(n_scales * kPitch * 4);
    p.at_w = c.take(n_scales * kPitch * 16);
    p.at_row = c.take(n_scales * p.tiles * (int64_t)sizeof(WpsRowPart));
    const int64_t budget = work_budget();
    p.chunk = kChunk;
    for (;;) {
        p.chunks = (n_scales + p.chunk - 1) / p.chunk;
        const bool fits = budget <= 0 || c.at + up256(p.chunks * 2 * n * 8) <= budget;
        if ((fits && p.chunks <= 65535) || p.chunk >= n_scales) break;
        p.chunk *= 2;
    }
    p.at_col = c.take(p.chunks * 2 * n * 8);
    p.total = c.at;
    return p;
}

int wps_validate(int64_t n, int64_t n_scales, double step, double span, bool any_output) {
    PDC_REQUIRE(n >= 1, "wps: at least one sample is needed (got %lld)", (long long)n);
    PDC_REQUIRE(n_scales >= 1, "wps: at least one scale is needed (got %lld)", (long long)n_scales);
    PDC_REQUIRE(std::isfinite(step) && step > 0.0, "wps: the table's step must be finite and positive");
    PDC_REQUIRE(std::isfinite(span) && span > 0.0, "wps: the table's span must be finite and positive");
    PDC_REQUIRE(wps_sizes_ok(n, n_scales), "wps: plane too large");
    PDC_REQUIRE(any_output, "wps: every output is NULL");
    return PDC_OK;
}

// `work`: wps_plan(...).total bytes.  Everything is a device pointer; any output may be NULL.
int wps_enqueue(hipStream_t st, const double *d_x, const double *d_t, int64_t n, const double *d_periods,
                const double *d_scales, int64_t n_scales, const double *d_table, double step, double span, double corr,
                double t_min, double t_max, const WpsPlan &plan, double *d_spectrum, double *d_coefs, double *d_gwps,
                double *d_sav, double *d_masked_gwps, int64_t *d_gwps_count, double *d_masked_sav,
                int64_t *d_sav_count, void *work) {
    char *base = static_cast<char *>(work);
    WpsScale *rec = reinterpret_cast<WpsScale *>(base + plan.at_rec);
    int32_t *off = reinterpret_cast<int32_t *>(base + plan.at_off);
    double2 *w = reinterpret_cast<double2 *>(base + plan.at_w);
    hipLaunchKernelGGL(wps_taps_kernel, dim3((unsigned)n_scales), dim3(kTapBlock), 0, st, d_scales,
                       reinterpret_cast<const double2 *>(d_table), step, span, rec, off, w);
    PDC_HIP(hipGetLastError());
    WpsArgs a;
    a.t = d_t;
    a.periods = d_periods;
    a.rec = rec;
    a.n = n;
    a.n_scales = n_scales;
    a.tiles = plan.tiles;
    a.chunks = plan.chunks;
    a.chunk = plan.chunk;
    a.corr = corr;
    a.t_min = t_min;
    a.t_max = t_max;
    a.spectrum = d_spectrum;
    a.coefs = reinterpret_cast<double2 *>(d_coefs);
    a.part_row = reinterpret_cast<WpsRowPart *>(base + plan.at_row);
    a.part_col = reinterpret_cast<double *>(base + plan.at_col);
    a.gwps = d_gwps;
    a.masked_gwps = d_masked_gwps;
    a.sav = d_sav;
    a.masked_sav = d_masked_sav;
    a.gwps_count = d_gwps_count;
    a.sav_count = d_sav_count;
    g_last.tiles = plan.tiles;
    g_last.chunks = plan.chunks;
    g_last.chunk = plan.chunk;
    hipLaunchKernelGGL(wps_scan_kernel, dim3((unsigned)plan.tiles, (unsigned)plan.chunks), dim3(kBlock), 0, st, a, off, w,
                       d_x);
    PDC_HIP(hipGetLastError());
    const int64_t threads = n_scales + n;
    hipLaunchKernelGGL(wps_fold_kernel, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

}  // namespace

extern "C" {

int64_t pdc_wps_tile(void) { return kTile; }

int64_t pdc_wps_work_bytes(int64_t n, int64_t n_scales) {
    if (!wps_sizes_ok(n, n_scales)) return -1;
    return wps_plan(n, n_scales).total;
}

int pdc_wps_last_dispatch(int64_t *tiles, int64_t *chunks, int64_t *scales_per_chunk, int64_t *dense_scales,
                          int64_t *sparse_scales) {
    if (tiles) *tiles = g_last.tiles;
    if (chunks) *chunks = g_last.chunks;
    if (scales_per_chunk) *scales_per_chunk = g_last.chunk;
    if (dense_scales) *dense_scales = g_last.dense;
    if (sparse_scales) *sparse_scales = g_last.sparse;
    return PDC_OK;
}

int64_t pdc_wps_taps(double scale, double step, double span, int64_t *position_out, int32_t *before_out,
                     int32_t *after_out, int64_t *length_out) {
    double d;
    int64_t M;
    if (!(std::isfinite(step) && step > 0.0 && std::isfinite(span) && span > 0.0) || !wps_shape(scale, step, span, &d, &M)) {
        set_error("wps: scale %g cannot be served", scale);
        return PDC_ERR_INVALID;
    }
    const int64_t L = wps_length(d, M);
    if (length_out) *length_out = L;
    int64_t ntaps = 0;
    for (int q = 0; q < kTable && L >= 1; ++q) {
        const int64_t m = wps_first(q, d, M);
        if (!(m < L && wps_entry(m, d) == q)) continue;
        if (position_out) position_out[ntaps] = m;
        if (before_out) before_out[ntaps] = m > 0 ? (int32_t)wps_entry(m - 1, d) : -1;
        if (after_out) after_out[ntaps] = q;
        ++ntaps;
    }
    if (L >= 1) {
        if (position_out) position_out[ntaps] = L;
        if (before_out) before_out[ntaps] = (int32_t)wps_entry(L - 1, d);
        if (after_out) after_out[ntaps] = -1;
        ++ntaps;
    }
    return ntaps;
}

int pdc_wps_scan_dev(int device, void *stream, const double *d_x, const double *d_t, int64_t n, const double *d_periods,
                     const double *d_scales, int64_t n_scales, const double *d_table, double step, double span,
                     double corr, double t_min, double t_max, double *d_spectrum, double *d_coefs, double *d_gwps,
                     double *d_sav, double *d_masked_gwps, int64_t *d_gwps_count, double *d_masked_sav,
                     int64_t *d_sav_count) {
    PDC_TRY(wps_validate(n, n_scales, step, span,
                         d_spectrum || d_coefs || d_gwps || d_sav || d_masked_gwps || d_gwps_count || d_masked_sav ||
                             d_sav_count));
    PDC_REQUIRE(d_x && d_t && d_periods && d_scales && d_table, "wps: NULL argument");
    PDC_TRY(use_device(device));
    const WpsPlan plan = wps_plan(n, n_scales);
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, plan.total, &work));
    g_last.dense = g_last.sparse = -1;   // (the scales are on the device)
    return wps_enqueue(st, d_x, d_t, n, d_periods, d_scales, n_scales, d_table, step, span, corr, t_min, t_max, plan,
                       d_spectrum, d_coefs, d_gwps, d_sav, d_masked_gwps, d_gwps_count, d_masked_sav, d_sav_count, work);
}

int pdc_wps_scan(const double *x, const double *t, int64_t n, const double *periods, const double *scales,
                 int64_t n_scales, const double *table, double step, double span, double corr, double *spectrum_out,
                 double *coefs_out, double *gwps_out, double *sav_out, double *masked_gwps_out, int64_t *gwps_count_out,
                 double *masked_sav_out, int64_t *sav_count_out, int device) {
    PDC_TRY(wps_validate(n, n_scales, step, span,
                         spectrum_out || coefs_out || gwps_out || sav_out || masked_gwps_out || gwps_count_out ||
                             masked_sav_out || sav_count_out));
    PDC_REQUIRE(x && t && periods && scales && table, "wps: NULL argument");
    PDC_REQUIRE(std::isfinite(corr), "wps: the cone-of-influence factor must be finite");
    for (int q = 0; q < 2 * kTable; ++q) PDC_REQUIRE(std::isfinite(table[q]), "wps: the wavelet table is not finite");
    int64_t dense = 0, sparse = 0;
    for (int64_t i = 0; i < n_scales; ++i) {
        double d;
        int64_t M;
        PDC_REQUIRE(std::isfinite(periods[i]), "wps: periods[%lld] is not finite", (long long)i);
        PDC_REQUIRE(std::isfinite(scales[i]) && scales[i] <= kMaxScale && wps_shape(scales[i], step, span, &d, &M) &&
                        wps_length(d, M) >= 2,
                    "wps: scales[%lld] = %g cannot be served: the filter needs at least 2 entries and at most 2^24 "
                    "samples per period",
                    (long long)i, scales[i]);
        (wps_length(d, M) + 1 <= kTable + 1 ? dense : sparse) += 1;
    }
    double t_min = t[0], t_max = t[0];
    for (int64_t k = 0; k < n; ++k) {
        PDC_REQUIRE(std::isfinite(x[k]), "wps: x[%lld] is not finite", (long long)k);
        PDC_REQUIRE(std::isfinite(t[k]), "wps: t[%lld] is not finite", (long long)k);
        t_min = t[k] < t_min ? t[k] : t_min;
        t_max = t[k] > t_max ? t[k] : t_max;
    }
    HostCall hc(device);
    PDC_TRY(hc.status);
    const WpsPlan plan = wps_plan(n, n_scales);
    // x | t in one input slot, periods | scales in another, the table in a third
    Carve ci;
    const int64_t at_x = ci.take(n * 8), at_t = ci.take(n * 8);
    char *d_in = hc.out<char>(SLOT_IN0, ci.at);
    Carve cs;
    const int64_t at_p = cs.take(n_scales * 8), at_s = cs.take(n_scales * 8);
    char *d_sc = hc.out<char>(SLOT_IN1, cs.at);
    double *d_table = hc.in(SLOT_IN2, table, 2 * kTable * 8);
    const int64_t plane = n * n_scales * 8;
    double *d_spectrum = spectrum_out ? hc.out<double>(SLOT_OUT0, plane) : nullptr;
    double *d_coefs = coefs_out ? hc.out<double>(SLOT_OUT1, 2 * plane) : nullptr;
    Carve c;
    const int64_t at_g = c.take(n_scales * 8), at_mg = c.take(n_scales * 8), at_gc = c.take(n_scales * 8),
                  at_v = c.take(n * 8), at_mv = c.take(n * 8), at_vc = c.take(n * 8);
    char *d_small = hc.out<char>(SLOT_OUT2, c.at);
    void *d_work = hc.reserve(SLOT_WORK, plan.total);
    PDC_TRY(hc.status);
    hc.put(d_in + at_x, x, n * 8);
    hc.put(d_in + at_t, t, n * 8);
    hc.put(d_sc + at_p, periods, n_scales * 8);
    hc.put(d_sc + at_s, scales, n_scales * 8);
    PDC_TRY(hc.status);
    double *d_g = gwps_out ? reinterpret_cast<double *>(d_small + at_g) : nullptr;
    double *d_mg = masked_gwps_out ? reinterpret_cast<double *>(d_small + at_mg) : nullptr;
    int64_t *d_gc = gwps_count_out ? reinterpret_cast<int64_t *>(d_small + at_gc) : nullptr;
    double *d_v = sav_out ? reinterpret_cast<double *>(d_small + at_v) : nullptr;
    double *d_mv = masked_sav_out ? reinterpret_cast<double *>(d_small + at_mv) : nullptr;
    int64_t *d_vc = sav_count_out ? reinterpret_cast<int64_t *>(d_small + at_vc) : nullptr;
    g_last.dense = dense;
    g_last.sparse = sparse;
    PDC_TRY(wps_enqueue(hc.stream(), reinterpret_cast<double *>(d_in + at_x), reinterpret_cast<double *>(d_in + at_t), n,
                        reinterpret_cast<double *>(d_sc + at_p), reinterpret_cast<double *>(d_sc + at_s), n_scales,
                        d_table, step, span, corr, t_min, t_max, plan, d_spectrum, d_coefs, d_g, d_v, d_mg, d_gc, d_mv,
                        d_vc, d_work));
    hc.back(spectrum_out, d_spectrum, plane);
    hc.back(coefs_out, d_coefs, 2 * plane);
    hc.back(gwps_out, d_g, n_scales * 8);
    hc.back(masked_gwps_out, d_mg, n_scales * 8);
    hc.back(gwps_count_out, d_gc, n_scales * 8);
    hc.back(sav_out, d_v, n * 8);
    hc.back(masked_sav_out, d_mv, n * 8);
    hc.back(sav_count_out, d_vc, n * 8);
    return hc.finish();
}

}  // extern "C"
