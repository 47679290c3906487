// StringLength over a batch of light curves that each keep their OWN period grid ("ragged" grids):
// StringLength.batch.  Included at the end of stringlength.hip: it needs sl_period.h (duo_period, is_one_cycle,
// onecycle_sum, prep_sample: the functions the single call's kernels call), sl_p1.inc, the duo:: layout and the
// single call's host ladder (stringlength_scan_impl, launch_fast_for).
//
// Every curve's trial periods are 1 / np.linspace(count * s, s, count), s = dphi / baseline_b (phase.py:
// _string_periods): curve b owns samples [offsets[b], offsets[b+1]) and the periods 1 / linspace(start[b], stop[b],
// P_b), P_b = p_offsets[b+1] - p_offsets[b], whose lengths go to out[p_offsets[b] + j] (period order).
//
// A curve of 1 <= N <= duo::kCapD samples takes, in the single call, the one-cycle pre-pass, sl_prep_kernel, the duo
// kernel and sl_fast_kernel on the periods the duo kernel marked.  Here, for all such curves of a group at once:
//   sl_ragged_periods_kernel  one thread per (curve, period): 1.0 / (j * step + start), exactly 1.0 / stop at the
//                             last index - numpy's linspace rule (the unit is built with -ffp-contract=off), then an
//                             IEEE division, as 1 / np.linspace(...) computes the single call's periods.
//   sl_ragged_prep_kernel     one workgroup per curve: prep_sample, as sl_prep_kernel and sl_tame_kernel call it - the AoS
//                             (t, m) records, the |t| flag and the bad[0..1] words (OR reductions: any order gives the
//                             same words).
//   sl_ragged_mark_kernel     one thread per (curve, period): is_one_cycle, as sl_onecycle_mark_kernel calls it, with
//                             that curve's words.
//   sl_ragged_onecycle_kernel one 1024-thread workgroup per listed (curve, period): onecycle_sum<1024>, as
//                             sl_onecycle_kernel calls it (one reduction shape, so the same bits).
//   sl_duo_ragged_kernel      persistent; the ticket counts (curve, period) items in a dispatch-order prefix table,
//                             costliest curve first (ragged_order); a workgroup finds its curve by a scalar binary
//                             search and runs sl_duo_kernel's period - sl_p1.inc, then duo_period - on a DuoCurve of
//                             that curve's slices.  One launch per instance the single call would pick (<16, 256, 512>,
//                             <16>, <36>, <52>): P3c adds range lengths r = tid, tid + kB, ..., so the block size decides
//                             the summation order.  A marked period increments its curve's counter.
// Then the host reads the B counters and runs launch_fast_for<false> on the slices of every curve with marks; curves
// the duo kernel does not take (N > kCapD, N = 0, or knobs that move the single call off it) run
// stringlength_scan_impl on their slices, with the hints the host entry would compute.  Every value is therefore the
// single call's, bit for bit.  sl_ragged_pitch_kernel writes the optional pitched copy for the peak table: FSeries
// order (ascending frequency = the period index reversed on a descending frequency grid), negated (a string length
// is minimal at the period).
#include <algorithm>
#include <atomic>

namespace {

namespace slr {

constexpr int kMeta = 14;          // arrays of B + 1 in the metadata upload (slr_group_dev), in this order:
enum { M_OFF, M_POFF, M_ROUTE, M_ORDER, M_OPRE = M_ORDER + 4, M_START = M_OPRE + 4, M_STEP, M_STOP };   // order, opre: [4]
constexpr int kPrepBlock = 256;
constexpr int kRangeGrid = 1024;   // duo workgroups at most (4 x 256 CUs): the range scratch is laid out for them
constexpr int64_t kMarkGrid = 32;  // workgroups of the marked-period fallback (its scratch is laid out for them)
constexpr int kLong = 4, kNone = 5;   // routes beyond the four duo instances

struct Args {
    const double *t, *m;            // every curve's samples
    const int64_t *offsets, *poff;  // [B + 1]
    const int64_t *route;           // [B] 0..3 duo instance, kLong, kNone
    const double *start, *step, *stop;   // [B] the FREQUENCY linspace of every curve
    int64_t n_curves, p_total;
    double *periods;                // [p_total]
    fast::rec_t *rec;               // [n_total]
    unsigned *flags;                // [B] sl_prep_kernel's flag
    unsigned *bad;                  // [B][2] sl_tame_kernel's words
    unsigned char *skip, *todo;     // [p_total]
    unsigned *list, *count;         // one-cycle periods (global index) and their number
    unsigned *marked;               // [B] periods the duo kernel left to the one-workgroup kernel
    double *ell;                    // [p_total]
    double *pitched;                // [B][pitch] or nullptr
    int64_t pitch;
};

__device__ __forceinline__ int64_t curve_of(const int64_t *poff, int64_t n_curves, int64_t q) {
    int64_t lo = 0, hi = n_curves - 1;   // the last b with poff[b] <= q (empty curves share their start)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (poff[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void sl_ragged_periods_kernel(Args a) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.p_total) return;
    const int64_t b = curve_of(a.poff, a.n_curves, q);
    const int64_t j = q - a.poff[b], count = a.poff[b + 1] - a.poff[b];
    const double f = count > 1 && j == count - 1 ? a.stop[b] : __dadd_rn(__dmul_rn((double)j, a.step[b]), a.start[b]);
    a.periods[q] = 1.0 / f;
}

__global__ __launch_bounds__(kPrepBlock) void sl_ragged_prep_kernel(Args a) {
    const int64_t b = blockIdx.x;
    if (a.route[b] >= kLong) return;   // (workgroup-uniform)
    __shared__ unsigned words[2];
    if (threadIdx.x < 2) words[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t off = a.offsets[b], n = a.offsets[b + 1] - off;
    const double *t = a.t + off, *m = a.m + off;
    fast::PrepFlags f;
    for (int64_t i = threadIdx.x; i < n; i += kPrepBlock) fast::prep_sample(t, m, i, a.rec + off, f);
    if (f.wild) atomicOr(&words[0], 1u);
    if (f.unsorted) atomicOr(&words[1], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        a.flags[b] = words[0] ? 0u : 1u;
        a.bad[2 * b + 0] = words[0];
        a.bad[2 * b + 1] = words[1];
    }
}

__global__ __launch_bounds__(256) void sl_ragged_mark_kernel(Args a) {
    using namespace fast;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.p_total) return;
    const int64_t b = curve_of(a.poff, a.n_curves, q);
    bool one = false;
    if (a.route[b] < kLong) {
        const int64_t off = a.offsets[b], n = a.offsets[b + 1] - off;
        one = is_one_cycle(a.t + off, n, a.periods[q], a.bad[2 * b], a.bad[2 * b + 1]);
    }
    a.skip[q] = one ? 1 : 0;
    if (one) a.list[atomicAdd(a.count, 1u)] = (unsigned)q;
}

__global__ __launch_bounds__(kBlock) void sl_ragged_onecycle_kernel(Args a) {
    using namespace fast;
    __shared__ double red[kBlock / 64];
    const unsigned count = *a.count;
    for (unsigned k = blockIdx.x; k < count; k += gridDim.x) {   // (workgroup-uniform)
        const int64_t q = a.list[k];
        const int64_t b = curve_of(a.poff, a.n_curves, q);
        const int64_t off = a.offsets[b], n = a.offsets[b + 1] - off;
        const double period = a.periods[q];
        const bool safe = period_is_safe(period, a.bad[2 * b] == 0u);
        const double total = onecycle_sum<kBlock>(a.t + off, a.m + off, n, period, safe, red);
        if (threadIdx.x == 0) a.ell[q] = total;
        __syncthreads();
    }
}

// FSeries order and sign for pdc_peaks_topk_dev: ascending frequency is the period index reversed when the frequency
// grid descends (start > stop: the usual case), kept otherwise
__global__ __launch_bounds__(256) void sl_ragged_pitch_kernel(Args a) {
    const int64_t b = blockIdx.x;
    const int64_t po = a.poff[b], np = a.poff[b + 1] - po;
    const bool rev = a.start[b] > a.stop[b];
    for (int64_t j = threadIdx.x; j < np; j += 256) a.pitched[b * a.pitch + (rev ? np - 1 - j : j)] = -a.ell[po + j];
}

}  // namespace slr

namespace duo {

struct RaggedDuoArgs {
    const double *t, *m, *periods;
    const rec_t *rec;
    const int64_t *offsets, *poff;   // [B + 1]
    const int64_t *order, *opre;     // this instance's curves in dispatch order [mc], their period prefix [mc + 1]
    int64_t mc;
    const unsigned *flags;           // [B]
    unsigned *ticket;                // [0] next item (zeroed before the launch)
    unsigned *marked;                // [B]
    double *ell;
    unsigned char *todo;
    const unsigned char *skip;
    double *rsum;                    // [grid][nr_pad][4]
    int *rcnt;                       // [grid][nr_pad]
    double *rlen;                    // [grid][nr_pad]
    int64_t nr_pad;
};

// sl_duo_kernel over the (curve, period) items of every curve of one instance: the same duo_period, on the curve of
// the ticket
template <int KMAX, int BLK = duo::kB, int NBL = kNB>
__global__ __launch_bounds__(BLK, 4) void sl_duo_ragged_kernel(RaggedDuoArgs ra) {
    using L = View<BLK>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ unsigned wave_tot[BLK / 64];
    __shared__ double red[BLK / 64];
    __shared__ unsigned s_item, s_bad;
    const int tid0 = threadIdx.x, lane = tid0 & 63, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
    const L v = L::carve(lds_raw, wave);
    const RangeScratch rs = {ra.rsum + (int64_t)blockIdx.x * ra.nr_pad * 4, ra.rcnt + (int64_t)blockIdx.x * ra.nr_pad,
                             ra.rlen + (int64_t)blockIdx.x * ra.nr_pad};
    const unsigned n_items = (unsigned)ra.opre[ra.mc];

    for (;;) {
        __syncthreads();   // the previous item is done with LDS
        if (tid0 == 0) {
            s_item = atomicAdd(ra.ticket, 1u);
            s_bad = 0u;
        }
        __syncthreads();
        const unsigned item = (unsigned)__builtin_amdgcn_readfirstlane((int)s_item);
        if (item >= n_items) break;
        // dispatch position: the c with opre[c] <= item < opre[c + 1] (every listed curve has >= 1 period)
        int64_t lo = 0, hi = ra.mc - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (ra.opre[mid] <= (int64_t)item) lo = mid;
            else hi = mid - 1;
        }
        const int64_t curve = ra.order[lo];
        const int64_t p = (int64_t)item - ra.opre[lo];
        const int64_t off = ra.offsets[curve], po = ra.poff[curve];
        if (ra.skip[po + p]) continue;   // (workgroup-uniform)
        const DuoCurve c = {ra.t + off, ra.m + off, ra.rec + off, ra.periods + po, ra.ell + po, ra.todo + po,
                            (int)(ra.offsets[curve + 1] - off), ra.flags[curve] != 0u, ra.marked + curve};
        const int n = c.n;
        const double period = c.periods[p];
        const double y = 1.0 / period;
        const bool safe = period_is_safe(period, c.t_safe);
        int tid = tid0;   // (opaque copy, once per period: addresses built from it are not hoisted out of the ticket loop and spilled)
        asm volatile("" : "+v"(tid));
        unsigned pk[(KMAX + 1) / 2];
        {   // (P1 is text in the kernel body: sl_p1.inc says why)
            constexpr int P1_BLK = BLK, P1_NB = NBL;
            const double *const p1_t = c.t;
#include "sl_p1.inc"
        }
        duo_period<KMAX, BLK, NBL>(c, p, period, y, safe, tid, pk, v, rs, red, &s_bad, lane, wave);
    }
}

}  // namespace duo

// ---- host side ----------------------------------------------------------------------------------------------------
// The route the single call takes for a curve of n samples and P periods: 0..3 = duo instance <16, 256, 512>, <16>,
// <36>, <52> (sl_fast); kLong = anything else (stringlength_scan_impl on the curve's slices); kNone = no periods.
int slr_route(int64_t n, int64_t P) {
    if (P == 0) return slr::kNone;
    const Knobs &k = knobs();
    if (n < 1 || n > duo::kCapD || !k.slices || k.general_only || !k.duo || stream_takes(n) ||
        n > k.fast_slices * (int64_t)fast::FL<unsigned>::capacity)
        return slr::kLong;
    if (k.quad && n <= duo::kCapQ) return 0;
    const int64_t kd = (n + duo::kB - 1) / duo::kB;
    return kd <= 16 ? 1 : (kd <= 36 ? 2 : 3);
}

// Bytes of the area a curve's fallback needs: the marked periods' scratch (sl_layout at kMarkGrid periods) or the
// whole single-call workspace.  Call outside any WorkScale scope (the scan itself runs outside one).
int64_t slr_fallback_bytes(int route, int64_t n, int64_t P, int hints) {
    if (route == slr::kNone) return 0;
    if (route == slr::kLong) return sorted_scan_work_bytes(3, n, P, hints);
    return sl_layout(n, P < slr::kMarkGrid ? P : slr::kMarkGrid, false).total;
}

struct SlRaggedLayout {
    int64_t meta, rec, flags, bad, periods, skip, todo, list, count, ell, range, fallback, total;
};
// nr_pad: range slots of the longest duo curve (0: none); fallback: the largest slr_fallback_bytes of the group
SlRaggedLayout slr_layout(int64_t B, int64_t n_total, int64_t p_total, int64_t nr_pad, int64_t fallback) {
    SlRaggedLayout w;
    Carve c;
    w.meta = c.take(slr::kMeta * (B + 1) * 8);
    w.rec = c.take(n_total * 16);
    w.flags = c.take(B * 4);
    w.bad = c.take(B * 8);
    w.periods = c.take(p_total * 8);
    w.skip = c.take(p_total);
    w.todo = c.take(p_total);
    w.list = c.take(p_total * 4);
    w.count = c.take(256);   // count | ticket | (256 on) marked [B]
    c.take(B * 4);
    w.ell = c.take(p_total * 8);
    w.range = c.take((int64_t)slr::kRangeGrid * nr_pad * (32 + 4 + 8));
    w.fallback = c.take(fallback);
    w.total = c.at;
    return w;
}

template <int KMAX, int BLK = duo::kB, int NBL = fast::kNB>
int launch_duo_ragged(const duo::RaggedDuoArgs &a, int n_max, int64_t grid, hipStream_t st) {
    const size_t lds = duo::View<BLK>::bytes(n_max);
    PDC_TRY(allow_dynamic_lds((const void *)duo::sl_duo_ragged_kernel<KMAX, BLK, NBL>, duo::kLdsWg - duo::kStaticD));
    hipLaunchKernelGGL((duo::sl_duo_ragged_kernel<KMAX, BLK, NBL>), dim3((unsigned)grid), dim3(BLK), lds, st, a);
    return PDC_OK;
}

struct SlrStats {
    std::atomic<int64_t> marked{0}, long_curves{0};
};
SlrStats g_slr_stats;

// Every launch of one group.  Metadata (offsets, p_offsets rebased to the group, the frequency linspace, per-curve
// hints and fallback bytes) on the host; t, m, the outputs and the workspace on the device.  Waits for the stream once,
// after the duo scan, to read the per-curve counts of marked periods.
int slr_group_dev(int device, hipStream_t st, const double *d_t, const double *d_m, const int64_t *offsets,
                  int64_t B, const double *start, const double *step, const double *stop, const int64_t *poff,
                  const int *hints, double *d_out, double *d_pitched, int64_t pitch, void *work, int64_t work_bytes,
                  std::vector<int64_t> &host_meta, bool wait_meta) {
    const int64_t n_total = offsets[B], p_total = poff[B];
    std::vector<int> route((size_t)B);
    int64_t n_duo = 0, fb = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b], P = poff[b + 1] - poff[b];
        route[(size_t)b] = slr_route(n, P);
        if (route[(size_t)b] < slr::kLong) n_duo = std::max(n_duo, n);
        fb = std::max(fb, slr_fallback_bytes(route[(size_t)b], n, P, hints ? hints[b] : kHintLists));
    }
    const SlRaggedLayout w = slr_layout(B, n_total, p_total, n_duo > 0 ? range_slots(n_duo) : 0, fb);
    PDC_REQUIRE(work && work_bytes >= w.total, "stringlength_ragged: workspace too small (%lld < %lld bytes)",
                (long long)work_bytes, (long long)w.total);
    PDC_REQUIRE(n_total == 0 || (d_t && d_m), "stringlength_ragged: t and m must not be NULL");
    PDC_TRY(use_device(device));
    if (p_total == 0) return PDC_OK;
    char *base = static_cast<char *>(work);
    // metadata: one upload; every duo instance's dispatch order = ragged_order (costliest curve first)
    RaggedMeta meta(host_meta, slr::kMeta, B, base + w.meta);
    meta.fill_offsets(offsets, poff);
    meta.fill_linspace(slr::M_START, start, step, stop);
    std::copy(route.begin(), route.end(), meta.i64(slr::M_ROUTE));
    int64_t mc[4], items[4];
    int n_max[4] = {0, 0, 0, 0};
    std::vector<int64_t> rows((size_t)B + 1);
    for (int c = 0; c < 4; ++c) {   // each instance's curves, most samples first, and their period prefix
        rows[0] = 0;
        for (int64_t b = 0; b < B; ++b) {
            rows[(size_t)b + 1] = rows[(size_t)b] + (route[(size_t)b] == c ? poff[b + 1] - poff[b] : 0);
            if (route[(size_t)b] == c) n_max[c] = std::max(n_max[c], (int)(offsets[b + 1] - offsets[b]));
        }
        mc[c] = ragged_order(offsets, rows.data(), B, 1, meta.i64(slr::M_ORDER + c), meta.i64(slr::M_OPRE + c));
        items[c] = meta.i64(slr::M_OPRE + c)[mc[c]];
    }
    PDC_TRY(meta.upload(st, wait_meta));

    slr::Args a = {};
    a.t = d_t;
    a.m = d_m;
    a.offsets = meta.d_i64(slr::M_OFF);
    a.poff = meta.d_i64(slr::M_POFF);
    a.route = meta.d_i64(slr::M_ROUTE);
    a.start = meta.d_f64(slr::M_START);
    a.step = meta.d_f64(slr::M_STEP);
    a.stop = meta.d_f64(slr::M_STOP);
    a.n_curves = B;
    a.p_total = p_total;
    a.periods = ptr<double>(base, w.periods);
    a.rec = ptr<fast::rec_t>(base, w.rec);
    a.flags = ptr<unsigned>(base, w.flags);
    a.bad = ptr<unsigned>(base, w.bad);
    a.skip = ptr<unsigned char>(base, w.skip);
    a.todo = ptr<unsigned char>(base, w.todo);
    a.list = ptr<unsigned>(base, w.list);
    a.count = ptr<unsigned>(base, w.count);
    a.marked = ptr<unsigned>(base, w.count + 256);
    a.ell = d_out ? d_out : ptr<double>(base, w.ell);
    a.pitched = d_pitched;
    a.pitch = pitch;
    unsigned *ticket = a.count + 1;
    PDC_HIP(hipMemsetAsync(a.count, 0, (size_t)(256 + B * 4), st));
    const unsigned pgrid = (unsigned)((p_total + 255) / 256);
    hipLaunchKernelGGL(slr::sl_ragged_periods_kernel, dim3(pgrid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(slr::sl_ragged_prep_kernel, dim3((unsigned)B), dim3(slr::kPrepBlock), 0, st, a);
    hipLaunchKernelGGL(slr::sl_ragged_mark_kernel, dim3(pgrid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(slr::sl_ragged_onecycle_kernel, dim3(256), dim3(kBlock), 0, st, a);
    PDC_HIP(hipGetLastError());

    const bool any_duo = items[0] + items[1] + items[2] + items[3] > 0;
    if (any_duo) {
        duo::RaggedDuoArgs d;
        d.t = d_t;
        d.m = d_m;
        d.periods = a.periods;
        d.rec = a.rec;
        d.offsets = a.offsets;
        d.poff = a.poff;
        d.flags = a.flags;
        d.ticket = ticket;
        d.marked = a.marked;
        d.ell = a.ell;
        d.todo = a.todo;
        d.skip = a.skip;
        d.nr_pad = range_slots(n_duo);
        d.rsum = ptr<double>(base, w.range);
        d.rcnt = ptr<int>(base, w.range + (int64_t)slr::kRangeGrid * d.nr_pad * 32);
        d.rlen = ptr<double>(base, w.range + (int64_t)slr::kRangeGrid * d.nr_pad * 36);
        const int cus = cu_count(device);
        for (int c = 0; c < 4; ++c) {
            if (items[c] == 0) continue;
            d.order = meta.d_i64(slr::M_ORDER + c);
            d.opre = meta.d_i64(slr::M_OPRE + c);
            d.mc = mc[c];
            int64_t grid = (c == 0 ? 4 : 2) * (int64_t)cus;
            grid = std::min(grid, std::min(items[c], (int64_t)slr::kRangeGrid));
            PDC_HIP(hipMemsetAsync(ticket, 0, 4, st));
            if (c == 0) PDC_TRY((launch_duo_ragged<16, 256, 512>(d, n_max[c], grid, st)));
            else if (c == 1) PDC_TRY(launch_duo_ragged<16>(d, n_max[c], grid, st));
            else if (c == 2) PDC_TRY(launch_duo_ragged<36>(d, n_max[c], grid, st));
            else PDC_TRY(launch_duo_ragged<52>(d, n_max[c], grid, st));
            PDC_HIP(hipGetLastError());
        }
    }
    // fallbacks on each curve's slices: the marked periods (sl_fast's one-workgroup kernel), the long curves
    char *area = base + w.fallback;
    if (any_duo) {
        std::vector<unsigned> marks((size_t)B);
        PDC_HIP(hipMemcpyAsync(marks.data(), a.marked, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        PDC_HIP(hipStreamSynchronize(st));
        for (int64_t b = 0; b < B; ++b) {
            if (route[(size_t)b] >= slr::kLong || marks[(size_t)b] == 0) continue;
            const int64_t off = offsets[b], po = poff[b], n = offsets[b + 1] - off, P = poff[b + 1] - po;
            const SlLayout l = sl_layout(n, P < slr::kMarkGrid ? P : slr::kMarkGrid, false);
            fast::FastArgs f = fast_args(l, area, d_t + off, d_m + off, a.periods + po, n, P, a.ell + po);
            f.rec = a.rec + off;
            f.flags = a.flags + b;
            f.skip = a.skip + po;
            f.todo = a.todo + po;
            f.todo_count = a.marked + b;
            PDC_TRY(launch_fast_for<false>(f, l.grid, st, knobs().p17));
            PDC_HIP(hipGetLastError());
            g_slr_stats.marked += marks[(size_t)b];
        }
    }
    for (int64_t b = 0; b < B; ++b) {
        if (route[(size_t)b] != slr::kLong) continue;
        const int64_t off = offsets[b], po = poff[b], n = offsets[b + 1] - off, P = poff[b + 1] - po;
        PDC_TRY(stringlength_scan_impl(device, st, d_t + off, d_m + off, n, a.periods + po, P, a.ell + po, area,
                                       w.total - w.fallback, hints ? hints[b] : kHintLists));
        ++g_slr_stats.long_curves;
    }
    if (d_pitched) {
        hipLaunchKernelGGL(slr::sl_ragged_pitch_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
        PDC_HIP(hipGetLastError());
    }
    return PDC_OK;
}

// ---- host entries: ragged_run (ragged.hip) deals the curves to device slots and runs each slot's groups ----------
RaggedSlots g_slr_slots;

// Range maxima over the curves of a group in O(1) (make_groups asks for every prefix of a share)
struct RangeMax {
    std::vector<std::vector<int64_t>> lv;
    explicit RangeMax(const std::vector<int64_t> &v) : lv{v} {
        for (size_t h = 1; ((size_t)1 << h) <= v.size(); ++h) {
            const std::vector<int64_t> &p = lv.back();
            std::vector<int64_t> q(v.size() - ((size_t)1 << h) + 1);
            for (size_t i = 0; i < q.size(); ++i) q[i] = std::max(p[i], p[i + ((size_t)1 << (h - 1))]);
            lv.push_back(std::move(q));
        }
    }
    int64_t operator()(int64_t c0, int64_t c1) const {   // max over [c0, c1), c1 > c0
        size_t h = 0;
        while (((size_t)2 << h) <= (size_t)(c1 - c0)) ++h;
        return std::max(lv[h][(size_t)c0], lv[h][(size_t)c1 - ((size_t)1 << h)]);
    }
};

struct SlJob : RaggedBatch {
    const double *t, *m, *start, *step, *stop;
    double *out;
    std::vector<int> hints;            // per curve (long curves: host_hints, as pdc_stringlength_scan computes them)
    const RangeMax *fb_max = nullptr, *nr_max = nullptr;   // per-curve fallback bytes, range slots of the duo curves

    SlJob(const double *t_, const double *m_, const int64_t *offsets_, const double *start_, const double *step_,
          const double *stop_, const int64_t *p_offsets, double *out_)
        : t(t_), m(m_), start(start_), step(step_), stop(stop_), out(out_) {
        offsets = offsets_;
        rows = p_offsets;
        negate_heights = true;   // (a string length is minimal at the period)
    }

    struct Bytes {
        int64_t in_t, in_m, out, work, table, total;
    };
    Bytes bytes(int64_t c0, int64_t c1, int64_t p_max) const {
        const int64_t n = offsets[c1] - offsets[c0], np = rows[c1] - rows[c0], B = c1 - c0;
        Bytes g;
        Carve c;
        g.in_t = c.take(n * 8);
        g.in_m = c.take(n * 8);
        g.out = c.take(out ? np * 8 : 0);
        g.work = c.at;
        g.table = g.work + slr_layout(B, n, np, (*nr_max)(c0, c1), (*fb_max)(c0, c1)).total;
        g.total = g.table + ragged_table_bytes(B, p_max, k);
        return g;
    }
    int64_t group_bytes(int64_t c0, int64_t c1, int64_t p_max) const override { return bytes(c0, c1, p_max).total; }

    int run_group(RaggedSlot &s, int64_t c0, int64_t c1, int64_t p_max, double *pitched) const override {
        const RaggedGroup g(*this, s, c0, c1);
        const Bytes at = bytes(c0, c1, p_max);
        PDC_TRY(g.upload(at.in_t, t));
        PDC_TRY(g.upload(at.in_m, m));
        PDC_TRY(slr_group_dev(s.device, g.st, g.at<double>(at.in_t), g.at<double>(at.in_m), g.off.data(), g.B, start + c0,
                              step + c0, stop + c0, g.roff.data(), hints.data() + c0, g.at_if<double>(out, at.out),
                              pitched, p_max, g.buf + at.work, at.table - at.work, s.meta, false));
        return g.rows_back(out, at.out);
    }
};

int slr_validate(const char *what, const int64_t *offsets, int64_t n_curves, const double *start, const double *step,
                 const double *stop, const int64_t *p_offsets) {
    PDC_REQUIRE(offsets && start && step && stop && p_offsets, "%s: NULL argument", what);
    auto curve = [&](int64_t b) {
        PDC_REQUIRE(offsets[b + 1] - offsets[b] < ((int64_t)1 << 31), "%s: curve %lld has 2^31 samples or more", what,
                    (long long)b);
        return PDC_OK;
    };
    return ragged_validate(what, offsets, p_offsets, "p_offsets", n_curves, 1,
                           "periods: the grids are too large for one launch", curve);
}

// The host-side periods of curve b (as the device writes them): what host_hints reads for a long curve
int slr_hints(const double *t, int64_t n, double start, double step, double stop, int64_t P) {
    std::vector<double> periods((size_t)P);
    for (int64_t j = 0; j < P; ++j) {
        const double f = P > 1 && j == P - 1 ? stop : (double)j * step + start;
        periods[(size_t)j] = 1.0 / f;
    }
    return sorted_scan_hints(3, t, n, periods.data(), P);
}

int slr_host(SlJob &j, int64_t n_curves, const int *devices, int n_devices) {
    PDC_REQUIRE(j.offsets[n_curves] == 0 || (j.t && j.m), "stringlength_ragged: t and m must not be NULL");
    std::vector<int64_t> fb((size_t)n_curves), nr((size_t)n_curves);
    j.hints.assign((size_t)n_curves, kHintLists);
    for (int64_t b = 0; b < n_curves; ++b) {   // (outside any WorkScale scope: the sizes the scans will ask for)
        const int64_t n = j.offsets[b + 1] - j.offsets[b], P = j.rows_of(b);
        const int route = slr_route(n, P);
        if (route == slr::kLong)
            j.hints[(size_t)b] = slr_hints(j.t + j.offsets[b], n, j.start[b], j.step[b], j.stop[b], P);
        fb[(size_t)b] = slr_fallback_bytes(route, n, P, j.hints[(size_t)b]);
        nr[(size_t)b] = route < slr::kLong ? range_slots(n) : 0;
    }
    const RangeMax fb_max(fb), nr_max(nr);
    j.fb_max = &fb_max;
    j.nr_max = &nr_max;
    g_slr_stats.marked = 0;
    g_slr_stats.long_curves = 0;
    return ragged_run("stringlength_ragged", g_slr_slots, j, n_curves, devices, n_devices);
}

}  // namespace

// Frees the per-slot buffers and streams of the ragged StringLength host entries (pdc_release()).
int pdc::release_sl_ragged() { return g_slr_slots.release(); }

extern "C" {

int pdc_test_sl_ragged_stats(int64_t *groups, int64_t *marked, int64_t *long_curves) {
    PDC_REQUIRE(groups && marked && long_curves, "pdc_test_sl_ragged_stats: NULL argument");
    std::lock_guard<std::mutex> lk(g_slr_slots.mutex);
    *groups = g_slr_slots.groups;
    *marked = g_slr_stats.marked;
    *long_curves = g_slr_stats.long_curves;
    return PDC_OK;
}

int64_t pdc_stringlength_ragged_work_bytes(const int64_t *offsets, const int64_t *p_offsets, int64_t n_curves) {
    if (!offsets || !p_offsets || n_curves < 1) return -1;
    int64_t n_duo = 0, fb = 0;
    for (int64_t b = 0; b < n_curves; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b], P = p_offsets[b + 1] - p_offsets[b];
        if (n < 0 || P < 0) return -1;
        const int route = slr_route(n, P);
        if (route < slr::kLong) n_duo = std::max(n_duo, n);
        fb = std::max(fb, slr_fallback_bytes(route, n, P, kHintLists));
    }
    return slr_layout(n_curves, offsets[n_curves] - offsets[0], p_offsets[n_curves] - p_offsets[0],
                      n_duo > 0 ? range_slots(n_duo) : 0, fb).total;
}

int pdc_stringlength_scan_ragged_dev(int device, void *stream, const double *d_t, const double *d_m,
                                     const int64_t *offsets, int64_t n_curves, const double *start, const double *step,
                                     const double *stop, const int64_t *p_offsets, double *d_out, double *d_pitched,
                                     int64_t pitch, void *work, int64_t work_bytes) {
    PDC_TRY(slr_validate("stringlength_ragged_dev", offsets, n_curves, start, step, stop, p_offsets));
    PDC_REQUIRE(d_out || d_pitched, "stringlength_ragged_dev: no output requested");
    if (d_pitched) PDC_TRY(ragged_check_pitch("stringlength_ragged_dev", p_offsets, n_curves, pitch, "periods"));
    std::vector<int64_t> meta;
    return slr_group_dev(device, (hipStream_t)stream, d_t, d_m, offsets, n_curves, start, step, stop, p_offsets,
                         nullptr, d_out, d_pitched, pitch, work, work_bytes, meta, true);
}

int pdc_stringlength_scan_ragged(const double *t, const double *m, const int64_t *offsets, int64_t n_curves,
                                 const double *start, const double *step, const double *stop,
                                 const int64_t *p_offsets, double *out, const int *devices, int n_devices) {
    PDC_TRY(slr_validate("stringlength_ragged", offsets, n_curves, start, step, stop, p_offsets));
    PDC_REQUIRE(out, "stringlength_ragged: no output requested");
    SlJob j(t, m, offsets, start, step, stop, p_offsets, out);
    return slr_host(j, n_curves, devices, n_devices);
}

int pdc_stringlength_ragged_peaks(const double *t, const double *m, const int64_t *offsets, int64_t n_curves,
                                  const double *start, const double *step, const double *stop,
                                  const int64_t *p_offsets, int k, int by_prominence, int64_t *count_out,
                                  int64_t *idx_out, double *height_out, double *prominence_out, int64_t *half_lo_out,
                                  int64_t *half_hi_out, double *out, const int *devices, int n_devices) {
    PDC_TRY(slr_validate("stringlength_ragged_peaks", offsets, n_curves, start, step, stop, p_offsets));
    SlJob j(t, m, offsets, start, step, stop, p_offsets, out);
    PDC_TRY(j.want_table("stringlength_ragged_peaks", k, by_prominence, count_out, idx_out, height_out, prominence_out,
                         half_lo_out, half_hi_out, out != nullptr));
    return slr_host(j, n_curves, devices, n_devices);
}

}  // extern "C"
