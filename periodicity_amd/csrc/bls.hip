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
// The prologue's body, the record, the LDS layout, the clearing and binning loops, the search and the limits are in
// bls_common.h, shared with the batch over ragged period grids (bls_ragged.hip); this unit keeps the kernels, the
// routes and the entries of the single call.
#include "pdc_internal.h"
#include "gls_sums.h"

#include <climits>
#include <cmath>

using namespace pdc;

namespace {

#include "bls_common.h"

struct BlsPrepArgs {
    const double *t, *y, *dy;
    int64_t n;
    BlsRec *rec;    // [n]
    double *scal;   // {YY, A, max |t|, bad}
};

__global__ __launch_bounds__(kPrepBlock) void bls_prep_kernel(BlsPrepArgs a) {
    bls_prep_body(a.t, a.y, a.dy, a.n, a.rec, a.scal);
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
    bls_clear(l, nb);
    const int64_t s_begin = FUSED ? 0 : (int64_t)blockIdx.y * a.z_len;
    const int64_t s_end = FUSED ? a.n : (s_begin + a.z_len < a.n ? s_begin + a.z_len : a.n);
    bls_bin(a.rec, a.scal[2], a.periods[p], nb, s_begin, s_end, l);
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
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, bytes, &work));
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
    HostCall hc(device);
    PDC_TRY(hc.status);
    int s = 1;
    int64_t bytes = 0;
    PDC_TRY(bls_route("bls", n, n_periods, q, host_work_budget(device), &s, &bytes));
    // (an empty curve still gets its blocks, and nothing to copy: t, y may be NULL then)
    const int64_t nn = n > 0 ? n : 1, ints = up256(n_periods * 4);
    double *d_t = hc.out<double>(SLOT_IN0, nn * 8), *d_y = hc.out<double>(SLOT_IN1, nn * 8);
    double *d_dy = dy ? hc.out<double>(SLOT_IN2, nn * 8) : nullptr;
    if (n > 0) {
        hc.put(d_t, t, n * 8);
        hc.put(d_y, y, n * 8);
        hc.put(d_dy, dy, n * 8);
    }
    double *d_per = hc.in(SLOT_IN3, periods, n_periods * 8);
    double *d_power = hc.out<double>(SLOT_OUT0, n_periods * 8), *d_depth = hc.out<double>(SLOT_OUT1, n_periods * 8);
    char *d_int = hc.out<char>(SLOT_OUT2, 2 * ints);   // start_bin | box_bins
    void *d_work = hc.reserve(SLOT_WORK, bytes);
    PDC_TRY(hc.status);
    int32_t *d_start = reinterpret_cast<int32_t *>(d_int), *d_box = reinterpret_cast<int32_t *>(d_int + ints);
    PDC_TRY(bls_enqueue(hc.stream(), d_t, d_y, d_dy, n, d_per, n_periods, q, s, d_power, d_depth, d_start, d_box, d_work));
    hc.back(power, d_power, n_periods * 8);
    hc.back(depth, d_depth, n_periods * 8);
    hc.back(start_bin, d_start, n_periods * 4);
    hc.back(box_bins, d_box, n_periods * 4);
    return hc.finish();
}

}  // extern "C"
