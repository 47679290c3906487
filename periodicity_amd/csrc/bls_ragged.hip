// Box least squares over a batch of light curves that each keep their OWN period grid ("ragged" grids): BLS.batch.
//
// Curve b owns samples [offsets[b], offsets[b+1]) and the trial periods linspace(start[b], stop[b], P_b),
// P_b = p_offsets[b+1] - p_offsets[b]; its four result rows go to X[p_offsets[b] + j] in period order, as
// pdc_bls_scan returns them, and its best box (the first maximum of the power row) to five [B] arrays.
//
// Decomposition
//   bls_ragged_prep_kernel    one workgroup of kPrepBlock threads per curve: bls_prep_body (bls_common.h) on the curve's
//                             slice - the statements, the order and the block size of bls_prep_kernel, so the records
//                             and YY, A, max |t| are the single call's bits.
//   bls_ragged_bin_kernel     one workgroup of kBlock threads per (curve, trial period): the fused route of
//                             bls_bin_kernel<true>.  The flat workgroup index is mapped to (curve, period) by a scalar
//                             binary search in the period prefix of the dispatch order (costliest curve first:
//                             ragged_order with a tile of 1); the period is rebuilt with numpy's linspace rule, not
//                             uploaded.  Clearing, binning and search are bls_common.h's.
//   bls_ragged_finish_kernel  one workgroup per curve: the NaN-aware argmax of the power row (among equal maxima the
//                             smaller period index; -1 / NaN for an empty or all-NaN row), the five best values and,
//                             for a peak table, the pitched [B][pitch] copy of the row in FSeries order (the period
//                             index reversed when stop > start).  Launched when a best output or the copy is asked for.
//
// There is no sliced route: a batch has sum P_b workgroups, and the sums are integers, so one workgroup per period gives
// the bits of every `slices` of the single call.
//
// The host entries' device slots, groups, budget and peak table are the shared driver's (ragged.hip); this unit sizes
// and runs one group.
#include "pdc_internal.h"
#include "gls_sums.h"

#include <climits>
#include <cmath>
#include <vector>

using namespace pdc;

namespace {

#include "bls_common.h"

constexpr int kFinBlock = 256;

struct BlsRaggedArgs {
    const double *t, *y, *dy;                     // samples of every curve; dy may be nullptr
    const int64_t *offsets, *poff;                // [B + 1] samples, periods
    const int64_t *operiod, *order;               // [m + 1] period prefix in dispatch order, [m] curve at each position
    const double *start, *step, *stop;            // [B] the linspace description of each grid
    int64_t m;
    int n_bins, len_min, len_max, min_points, dips_only;
    BlsRec *rec;                                  // [n_total]
    double *scal;                                 // [B][4] YY, A, max |t|, bad
    double *power, *depth;                        // [P_total] rows (never nullptr: the caller's or the workspace's)
    int32_t *start_bin, *box_bins;
    int64_t *best_index;                          // [B], each may be nullptr
    double *best_power, *best_depth;
    int32_t *best_start, *best_box;
    double *pitched;                              // [B][pitch] or nullptr
    int64_t pitch;
};

// np.linspace(start, stop, count)[j]: y = j * step; y += start; y[-1] = stop (count > 1).  With count == 1 the host
// passes step = stop - start (numpy's `y * delta`).
__device__ __forceinline__ double linspace_at(int64_t j, int64_t count, double start, double step, double stop) {
    if (count > 1 && j == count - 1) return stop;
    return __dadd_rn(__dmul_rn((double)j, step), start);
}

__global__ __launch_bounds__(kPrepBlock) void bls_ragged_prep_kernel(BlsRaggedArgs ra) {
    const int64_t b = blockIdx.x;
    const int64_t off = ra.offsets[b], n = ra.offsets[b + 1] - off;
    bls_prep_body(ra.t + off, ra.y + off, ra.dy ? ra.dy + off : nullptr, n, ra.rec + off, ra.scal + 4 * b);
}

__global__ __launch_bounds__(kBlock) void bls_ragged_bin_kernel(BlsRaggedArgs ra) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int64_t g = blockIdx.x;
    // dispatch position: the q with operiod[q] <= g < operiod[q + 1] (every listed curve has >= 1 period)
    int64_t lo = 0, hi = ra.m - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (ra.operiod[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int64_t curve = ra.order[lo];
    const int64_t p = g - ra.operiod[lo];
    const int64_t off = ra.offsets[curve], po = ra.poff[curve];
    const int64_t np = ra.poff[curve + 1] - po;
    BlsArgs a;
    a.rec = ra.rec + off;
    a.scal = ra.scal + 4 * curve;
    a.n = a.z_len = ra.offsets[curve + 1] - off;
    a.periods = nullptr;
    a.n_bins = ra.n_bins;
    a.len_min = ra.len_min;
    a.len_max = ra.len_max;
    a.min_points = ra.min_points;
    a.dips_only = ra.dips_only;
    a.gr = a.gs = nullptr;
    a.gc = nullptr;
    a.power = ra.power + po;
    a.depth = ra.depth + po;
    a.start_bin = ra.start_bin + po;
    a.box_bins = ra.box_bins + po;
    const int tid = threadIdx.x, nb = a.n_bins;
    const BlsLds l = bls_lds(lds_raw, nb, a.len_max, true);
    if (a.scal[3] != 0.0) {   // bad input: every output of the curve is NaN / -1
        if (tid == 0) bls_write(a, p, __builtin_nan(""), __builtin_nan(""), -1, -1);
        return;
    }
    bls_clear(l, nb);
    bls_bin(a.rec, a.scal[2], linspace_at(p, np, ra.start[curve], ra.step[curve], ra.stop[curve]), nb, 0, a.n, l);
    bls_search<kBlock>(a, p, l);
}

__global__ __launch_bounds__(kFinBlock) void bls_ragged_finish_kernel(BlsRaggedArgs ra) {
    __shared__ double w_v[kFinBlock / 64];
    __shared__ long long w_i[kFinBlock / 64];
    const int64_t b = blockIdx.x;
    const int64_t po = ra.poff[b], np = ra.poff[b + 1] - po;
    const int tid = threadIdx.x;
    // FSeries order is ascending frequency 1 / p: the reversed period index on an ascending grid, the period index on
    // a descending (or constant) one - for grids whose periods have one sign, which the caller ensures
    const bool rev = ra.stop[b] > ra.start[b];
    const double *row = ra.power + po;
    double best = 0.0;
    long long at = LLONG_MAX;   // LLONG_MAX: nothing finite seen; else the first index of `best`
    for (int64_t j = tid; j < np; j += kFinBlock) {
        const double v = row[j];
        if (ra.pitched) ra.pitched[b * ra.pitch + (rev ? np - 1 - j : j)] = v;
        if (v == v && (at == LLONG_MAX || v > best)) {
            best = v;
            at = j;
        }
    }
    auto better = [](double ov, long long oi, double v, long long i) {
        return oi != LLONG_MAX && (i == LLONG_MAX || ov > v || (ov == v && oi < i));
    };
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(best, o, 64);
        const long long oi = __shfl_down(at, o, 64);
        if (better(ov, oi, best, at)) {
            best = ov;
            at = oi;
        }
    }
    if ((tid & 63) == 0) {
        w_v[tid >> 6] = best;
        w_i[tid >> 6] = at;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < kFinBlock / 64; ++w)
        if (better(w_v[w], w_i[w], best, at)) {
            best = w_v[w];
            at = w_i[w];
        }
    const bool none = at == LLONG_MAX;
    if (ra.best_index) ra.best_index[b] = none ? -1 : at;
    if (ra.best_power) ra.best_power[b] = none ? __builtin_nan("") : best;
    if (ra.best_depth) ra.best_depth[b] = none ? __builtin_nan("") : ra.depth[po + at];
    if (ra.best_start) ra.best_start[b] = none ? -1 : ra.start_bin[po + at];
    if (ra.best_box) ra.best_box[b] = none ? -1 : ra.box_bins[po + at];
}

// ---- host side ------------------------------------------------------------------------------------------------
// The caller's outputs of one launch sequence (device pointers, any may be NULL).
struct BlsOut {
    double *power, *depth;
    int32_t *start_bin, *box_bins;
    int64_t *best_index;
    double *best_power, *best_depth;
    int32_t *best_start, *best_box;
    bool any_best() const { return best_index || best_power || best_depth || best_start || best_box; }
    bool any() const { return power || depth || start_bin || box_bins || any_best(); }
};

// Workspace of one launch over B curves: scal [B][4] | the metadata tables | the records | the rows the caller did not
// pass (own_*: power, depth: 8 bytes a period; start_bin, box_bins: 4) ; with k > 0 also the peak-table tail
// (ragged_table_bytes).
struct BlsLayout {
    int64_t scal, meta, rec, power, depth, start_bin, box_bins, pitched, total;
};
constexpr int kMetaArrays = 7;   // offsets | poff | operiod | order (int64) | start | step | stop, B + 1 each
enum { M_OFF, M_POFF, M_OPERIOD, M_ORDER, M_START, M_STEP, M_STOP };

BlsLayout bls_layout(int64_t n_curves, int64_t n_total, int64_t p_total, int64_t p_max, int k, bool own_power,
                     bool own_depth, bool own_start, bool own_box) {
    BlsLayout w;
    Carve c;
    w.scal = c.take(n_curves * 32);
    w.meta = c.take(kMetaArrays * (n_curves + 1) * 8);
    w.rec = c.take((n_total > 0 ? n_total : 1) * (int64_t)sizeof(BlsRec));
    w.power = c.take(own_power ? p_total * 8 : 0);
    w.depth = c.take(own_depth ? p_total * 8 : 0);
    w.start_bin = c.take(own_start ? p_total * 4 : 0);
    w.box_bins = c.take(own_box ? p_total * 4 : 0);
    w.pitched = c.at;
    w.total = w.pitched + ragged_table_bytes(n_curves, p_max, k);
    return w;
}

// Checks the host-side description of a batch; the same text for every entry point.
int validate(const char *what, const int64_t *offsets, int64_t n_curves, const double *start, const double *step,
             const double *stop, const int64_t *poff, const BlsParams &q) {
    PDC_TRY(bls_validate(what, 0, 0, q));
    PDC_REQUIRE(offsets && start && step && stop && poff, "%s: NULL argument", what);
    auto curve = [&](int64_t b) { return bls_validate(what, offsets[b + 1] - offsets[b], poff[b + 1] - poff[b], q); };
    return ragged_validate(what, offsets, poff, "p_offsets", n_curves, 1, "periods: the grids are too large for one launch",
                           curve);
}

// Every launch of one group of curves.  Metadata come from the host (offsets, p_offsets rebased to the group), the
// sample arrays, the outputs and the workspace are on the device.
int bls_ragged_dev(int device, hipStream_t st, const double *d_t, const double *d_y, const double *d_dy,
                   const int64_t *offsets, int64_t n_curves, const double *start, const double *step, const double *stop,
                   const int64_t *poff, const BlsParams &q, const BlsOut &out, double *d_pitched, int64_t pitch, void *work,
                   int64_t work_bytes, std::vector<int64_t> &host_meta, bool wait_meta) {
    const int64_t n_total = offsets[n_curves], p_total = poff[n_curves];
    const BlsLayout w = bls_layout(n_curves, n_total, p_total, 0, 0, !out.power, !out.depth, !out.start_bin,
                                   !out.box_bins);   // (the pitched copy is the caller's)
    PDC_REQUIRE(work && work_bytes >= w.total, "bls_ragged: workspace too small (%lld < %lld bytes)", (long long)work_bytes,
                (long long)w.total);
    PDC_REQUIRE(n_total == 0 || (d_t && d_y), "bls_ragged: t and y must not be NULL");
    PDC_TRY(use_device(device));
    char *base = static_cast<char *>(work);
    // metadata: one upload; dispatch order = ragged_order (costliest curve first)
    RaggedMeta meta(host_meta, kMetaArrays, n_curves, base + w.meta);
    meta.fill_offsets(offsets, poff);
    meta.fill_linspace(M_START, start, step, stop);
    const int64_t m = ragged_order(offsets, poff, n_curves, 1, meta.i64(M_ORDER), meta.i64(M_OPERIOD));
    const int64_t groups = meta.i64(M_OPERIOD)[m];   // == p_total
    PDC_TRY(meta.upload(st, wait_meta));

    BlsRaggedArgs a = {};
    a.t = d_t;
    a.y = d_y;
    a.dy = d_dy;
    a.offsets = meta.d_i64(M_OFF);
    a.poff = meta.d_i64(M_POFF);
    a.operiod = meta.d_i64(M_OPERIOD);
    a.order = meta.d_i64(M_ORDER);
    a.start = meta.d_f64(M_START);
    a.step = meta.d_f64(M_STEP);
    a.stop = meta.d_f64(M_STOP);
    a.m = m;
    a.n_bins = q.n_bins;
    a.len_min = q.len_min;
    a.len_max = q.len_max;
    a.min_points = q.min_points;
    a.dips_only = q.dips_only;
    a.rec = reinterpret_cast<BlsRec *>(base + w.rec);
    a.scal = reinterpret_cast<double *>(base + w.scal);
    a.power = out.power ? out.power : reinterpret_cast<double *>(base + w.power);
    a.depth = out.depth ? out.depth : reinterpret_cast<double *>(base + w.depth);
    a.start_bin = out.start_bin ? out.start_bin : reinterpret_cast<int32_t *>(base + w.start_bin);
    a.box_bins = out.box_bins ? out.box_bins : reinterpret_cast<int32_t *>(base + w.box_bins);
    a.best_index = out.best_index;
    a.best_power = out.best_power;
    a.best_depth = out.best_depth;
    a.best_start = out.best_start;
    a.best_box = out.best_box;
    a.pitched = d_pitched;
    a.pitch = pitch;
    hipLaunchKernelGGL(bls_ragged_prep_kernel, dim3((unsigned)n_curves), dim3(kPrepBlock), 0, st, a);
    PDC_HIP(hipGetLastError());
    if (groups > 0) {
        PDC_TRY(allow_dynamic_lds((const void *)bls_ragged_bin_kernel, kMaxLds));
        hipLaunchKernelGGL(bls_ragged_bin_kernel, dim3((unsigned)groups), dim3(kBlock),
                           bls_lds_bytes(q.n_bins, q.len_max, true), st, a);
        PDC_HIP(hipGetLastError());
    }
    if (out.any_best() || d_pitched) {
        hipLaunchKernelGGL(bls_ragged_finish_kernel, dim3((unsigned)n_curves), dim3(kFinBlock), 0, st, a);
        PDC_HIP(hipGetLastError());
    }
    return PDC_OK;
}

// ---- host entries: ragged_run (ragged.hip) deals the curves to device slots and runs each slot's groups ----------
RaggedSlots g_slots;

// What one host call computes and where its results go (caller's host arrays, any may be NULL); rows = p_offsets.
struct BlsJob : RaggedBatch {
    BlsParams q;
    const double *t, *y, *dy;
    const double *start, *step, *stop;
    BlsOut out;

    BlsJob(const double *t_, const double *y_, const double *dy_, const int64_t *offsets_, const double *start_,
           const double *step_, const double *stop_, const int64_t *p_offsets, const BlsParams &q_, const BlsOut &out_)
        : q(q_), t(t_), y(y_), dy(dy_), start(start_), step(step_), stop(stop_), out(out_) {
        offsets = offsets_;
        rows = p_offsets;
    }

    // The slot buffer of the group [c0, c1) whose longest grid has p_max periods: inputs | rows | best | workspace.
    struct Bytes {
        int64_t in_t, in_y, in_dy, power, depth, start_bin, box_bins, best_index, best_power, best_depth, best_start,
                best_box, work, total;
    };
    Bytes bytes(int64_t c0, int64_t c1, int64_t p_max) const {
        const int64_t n = offsets[c1] - offsets[c0], np = rows[c1] - rows[c0], B = c1 - c0;
        Bytes g;
        Carve c;
        g.in_t = c.take(n * 8);
        g.in_y = c.take(n * 8);
        g.in_dy = c.take(dy ? n * 8 : 0);
        g.power = c.take(np * 8);
        g.depth = c.take(np * 8);
        g.start_bin = c.take(np * 4);
        g.box_bins = c.take(np * 4);
        g.best_index = c.take(B * 8);
        g.best_power = c.take(B * 8);
        g.best_depth = c.take(B * 8);
        g.best_start = c.take(B * 4);
        g.best_box = c.take(B * 4);
        g.work = c.at;
        g.total = g.work + bls_layout(B, n, np, p_max, k, false, false, false, false).total;
        return g;
    }
    int64_t group_bytes(int64_t c0, int64_t c1, int64_t p_max) const override { return bytes(c0, c1, p_max).total; }

    int run_group(RaggedSlot &s, int64_t c0, int64_t c1, int64_t p_max, double *pitched) const override {
        const RaggedGroup g(*this, s, c0, c1);
        const Bytes at = bytes(c0, c1, p_max);
        PDC_TRY(g.upload(at.in_t, t));
        PDC_TRY(g.upload(at.in_y, y));
        PDC_TRY(g.upload(at.in_dy, dy));
        const BlsOut d = {g.at<double>(at.power),
                          g.at<double>(at.depth),
                          g.at<int32_t>(at.start_bin),
                          g.at<int32_t>(at.box_bins),
                          g.at_if<int64_t>(out.best_index, at.best_index),
                          g.at_if<double>(out.best_power, at.best_power),
                          g.at_if<double>(out.best_depth, at.best_depth),
                          g.at_if<int32_t>(out.best_start, at.best_start),
                          g.at_if<int32_t>(out.best_box, at.best_box)};
        PDC_TRY(bls_ragged_dev(s.device, g.st, g.at<double>(at.in_t), g.at<double>(at.in_y), g.at_if<double>(dy, at.in_dy),
                               g.off.data(), g.B, start + c0, step + c0, stop + c0, g.roff.data(), q, d, pitched, p_max,
                               g.buf + at.work, at.total - at.work, s.meta, false));
        PDC_TRY(g.rows_back(out.power, at.power));
        PDC_TRY(g.rows_back(out.depth, at.depth));
        PDC_TRY(g.rows_back(out.start_bin, at.start_bin));
        PDC_TRY(g.rows_back(out.box_bins, at.box_bins));
        PDC_TRY(g.curves_back(out.best_index, at.best_index));
        PDC_TRY(g.curves_back(out.best_power, at.best_power));
        PDC_TRY(g.curves_back(out.best_depth, at.best_depth));
        PDC_TRY(g.curves_back(out.best_start, at.best_start));
        return g.curves_back(out.best_box, at.best_box);
    }
};

int bls_host(const char *what, const BlsJob &j, int64_t n_curves, const int *devices, int n_devices) {
    PDC_REQUIRE(j.offsets[n_curves] == 0 || (j.t && j.y), "%s: t and y must not be NULL", what);
    return ragged_run(what, g_slots, j, n_curves, devices, n_devices);
}

}  // namespace

// Frees the per-slot buffers and streams of the ragged BLS host entries (pdc_release()).
int pdc::release_bls_ragged() { return g_slots.release(); }

extern "C" {

int pdc_test_bls_ragged_groups(int64_t *groups) {
    PDC_REQUIRE(groups, "pdc_test_bls_ragged_groups: NULL argument");
    std::lock_guard<std::mutex> lk(g_slots.mutex);
    *groups = g_slots.groups;
    return PDC_OK;
}

int64_t pdc_bls_ragged_work_bytes(int64_t n_curves, int64_t n_total, int64_t p_total, int64_t p_max, int k) {
    if (n_curves < 1 || n_total < 0 || p_total < 0 || p_max < 0 || k < 0) return -1;
    return bls_layout(n_curves, n_total, p_total, p_max, k, true, true, true, true).total;
}

int pdc_bls_scan_ragged_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy,
                            const int64_t *offsets, int64_t n_curves, const double *start, const double *step,
                            const double *stop, const int64_t *p_offsets, int n_bins, int len_min, int len_max,
                            int min_points, int dips_only, double *d_power, double *d_depth, int32_t *d_start_bin,
                            int32_t *d_box_bins, int64_t *d_best_index, double *d_best_power, double *d_best_depth,
                            int32_t *d_best_start, int32_t *d_best_box, double *d_pitched, int64_t pitch, void *work,
                            int64_t work_bytes) {
    const BlsParams q = {n_bins, len_min, len_max, min_points, dips_only ? 1 : 0, 0};
    PDC_TRY(validate("bls_ragged_dev", offsets, n_curves, start, step, stop, p_offsets, q));
    const BlsOut out = {d_power, d_depth, d_start_bin, d_box_bins, d_best_index, d_best_power, d_best_depth, d_best_start,
                        d_best_box};
    PDC_REQUIRE(out.any() || d_pitched, "bls_ragged_dev: no output requested");
    if (d_pitched) PDC_TRY(ragged_check_pitch("bls_ragged_dev", p_offsets, n_curves, pitch, "periods"));
    std::vector<int64_t> meta;
    return bls_ragged_dev(device, (hipStream_t)stream, d_t, d_y, d_dy, offsets, n_curves, start, step, stop, p_offsets, q,
                          out, d_pitched, pitch, work, work_bytes, meta, true);
}

int pdc_bls_scan_ragged(const double *t, const double *y, const double *dy, const int64_t *offsets, int64_t n_curves,
                        const double *start, const double *step, const double *stop, const int64_t *p_offsets, int n_bins,
                        int len_min, int len_max, int min_points, int dips_only, double *power, double *depth,
                        int32_t *start_bin, int32_t *box_bins, int64_t *best_index, double *best_power, double *best_depth,
                        int32_t *best_start, int32_t *best_box, const int *devices, int n_devices) {
    const BlsParams q = {n_bins, len_min, len_max, min_points, dips_only ? 1 : 0, 0};
    PDC_TRY(validate("bls_ragged", offsets, n_curves, start, step, stop, p_offsets, q));
    const BlsOut out = {power, depth, start_bin, box_bins, best_index, best_power, best_depth, best_start, best_box};
    PDC_REQUIRE(out.any(), "bls_ragged: no output requested");
    const BlsJob j(t, y, dy, offsets, start, step, stop, p_offsets, q, out);
    return bls_host("bls_ragged", j, n_curves, devices, n_devices);
}

int pdc_bls_ragged_peaks(const double *t, const double *y, const double *dy, const int64_t *offsets, int64_t n_curves,
                         const double *start, const double *step, const double *stop, const int64_t *p_offsets, int n_bins,
                         int len_min, int len_max, int min_points, int dips_only, int k, int by_prominence,
                         int64_t *count_out, int64_t *idx_out, double *height_out, double *prominence_out,
                         int64_t *half_lo_out, int64_t *half_hi_out, double *power, double *depth, int32_t *start_bin,
                         int32_t *box_bins, int64_t *best_index, double *best_power, double *best_depth,
                         int32_t *best_start, int32_t *best_box, const int *devices, int n_devices) {
    const BlsParams q = {n_bins, len_min, len_max, min_points, dips_only ? 1 : 0, 0};
    PDC_TRY(validate("bls_ragged_peaks", offsets, n_curves, start, step, stop, p_offsets, q));
    const BlsOut out = {power, depth, start_bin, box_bins, best_index, best_power, best_depth, best_start, best_box};
    BlsJob j(t, y, dy, offsets, start, step, stop, p_offsets, q, out);
    PDC_TRY(j.want_table("bls_ragged_peaks", k, by_prominence, count_out, idx_out, height_out, prominence_out, half_lo_out,
                         half_hi_out, out.any()));
    return bls_host("bls_ragged_peaks", j, n_curves, devices, n_devices);
}

}  // extern "C"
