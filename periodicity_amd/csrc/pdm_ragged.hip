// PDM, AoV and conditional entropy over a batch of light curves that each keep their OWN period grid ("ragged"
// grids): PDM.batch, AOV.batch, ConditionalEntropy.batch.
//
// The phase-folding classes build every curve's grid from that curve's data - np.linspace(p_min, p_max, count)
// with p_min = 2 median_dt, p_max = oversample baseline and, for n_periods=None, a count of their own
// (phase.py:167-180) - so two curves almost never share one.  Here curve b owns samples [offsets[b], offsets[b+1])
// and the trial periods linspace(start[b], stop[b], P_b), P_b = p_offsets[b+1] - p_offsets[b], written to
// out[p_offsets[b] + j] (period order, as the single call's `_scan` returns them).
//
// Decomposition
//   pdm_ragged_prep_kernel    one workgroup of BLOCK threads per curve: mean of x, max |t| and sum (x - mean)^2 by
//                             block_reduce<BLOCK> over i = tid, tid + BLOCK, ...  - the order and the BLOCK of the
//                             unsplit pdm_scan_kernel, whose every workgroup computes the same three values for
//                             itself; so the scan below starts from the single call's bits.
//   pdm_ragged_scan_kernel    one workgroup per (curve, tile of 64 trial periods), found by a scalar binary search
//                             in a dispatch-order tile prefix table; tiles are dispatched costliest curve (most
//                             samples) first (ragged_order).  The period of a lane is rebuilt with numpy's
//                             linspace rule (j*step + start, two roundings - the unit is built with
//                             -ffp-contract=off - and exactly `stop` at the last index), not uploaded.  The sample loop is
//                             pdm_chunks.inc, the text of pdm_scan_kernel's; the <BLOCK, SPLIT> instance is the one
//                             the single call takes for a grid of < 131 072 periods (<256, 4>, or <64, 1> when
//                             that histogram does not fit 150 KB of LDS), and so is the epilogue (pdm_common.h).
//   pdm_ragged_finish_kernel  one workgroup per curve: the sub-harmonic averaging of
//                             phase.py:_average_with_double_period (every read sees the scan's values), then the
//                             output row and, for a peak table, a pitched [B][pitch] copy in FSeries order
//                             (ascending frequency: the period index reversed when stop > start, kept when the
//                             grid descends), negated for the kinds whose signal
//                             is a minimum (PDM, conditional entropy) so that pdc_peaks_topk_dev ranks their dips.
//                             The caller fills the pad with NaN; why the pad keeps scipy's answers, and the one
//                             half-maximum artefact it leaves, is explained in ragged.hip / periodicity_hip.h.
//
// The host entries' device slots, groups, budget and peak table are the shared driver's (ragged.hip); this unit
// sizes and runs one group.
//
// Bit identity: for a curve whose single call runs unsplit (n < 8192 samples, P < 131 072 periods) every value is
// computed by the same instructions on the same inputs in the same order.  Longer curves are split over workgroups
// by the single call (another summation order) and agree to rounding.
#include "pdc_internal.h"

#include <cmath>
#include <vector>

using namespace pdc;

namespace {

#include "pdm_common.h"

constexpr int kPTile = 64;   // trial periods per workgroup: BLOCK / SPLIT of both instances
constexpr int kFinBlock = 256;

struct RaggedPhaseArgs {
    const double *t, *x;                          // samples of every curve; x = the magnitude bins for CE
    const int64_t *offsets, *poff;                // [B + 1] samples, periods
    const double *start, *step, *stop;            // [B] the linspace description of each grid
    const double *sigma;                          // [B] PDM's np.var(values, ddof=1), else nullptr
    const double *signif;                         // [B] 1 - 11 / N**0.8 (sub-harmonic averaging), or nullptr
    const int64_t *otile, *order;                 // [m + 1] tile prefix in dispatch order, [m] curve at each position
    int64_t m, tiles;
    int nb, nc;
    double *stat;                                 // [B][3] mean, max |t|, sum (x - mean)^2
    double *raw;                                  // [P_total] the scan's statistic
    double *out;                                  // [P_total] or nullptr (may be `raw`)
    double *pitched;                              // [B][pitch] or nullptr
    int64_t pitch;
};

// np.linspace(start, stop, count)[j]: y = j * step; y += start; y[-1] = stop (count > 1).  With count == 1 the host
// passes step = stop - start (numpy's `y * delta`).
__device__ __forceinline__ double linspace_at(int64_t j, int64_t count, double start, double step, double stop) {
    if (count > 1 && j == count - 1) return stop;
    return __dadd_rn(__dmul_rn((double)j, step), start);
}

template <int BLOCK, bool CE>
__global__ __launch_bounds__(BLOCK) void pdm_ragged_prep_kernel(RaggedPhaseArgs ra) {
    __shared__ double red[BLOCK / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t off = ra.offsets[b], n = ra.offsets[b + 1] - off;
    const double *t = ra.t + off, *x = ra.x + off;
    // (pdm_scan_kernel's unsplit statistics, statement for statement)
    double acc = 0.0, tmax = 0.0;
    for (int64_t i = tid; i < n; i += BLOCK) {
        acc += x[i];
        const double at = __builtin_fabs(t[i]);
        tmax = at > tmax ? at : tmax;
    }
    const double mean = block_reduce<BLOCK>(acc, red, false) / (double)n;
    tmax = block_reduce<BLOCK>(tmax, red, true);
    acc = 0.0;
    for (int64_t i = tid; i < n && !CE; i += BLOCK) {
        const double d = x[i] - mean;
        acc += d * d;
    }
    const double q_total = block_reduce<BLOCK>(acc, red, false);
    if (tid == 0) {
        ra.stat[b * 3 + 0] = mean;
        ra.stat[b * 3 + 1] = tmax;
        ra.stat[b * 3 + 2] = q_total;
    }
}

template <int BLOCK, int SPLIT, int KIND>
__global__ __launch_bounds__(BLOCK) void pdm_ragged_scan_kernel(RaggedPhaseArgs ra) {
    static_assert(BLOCK / SPLIT == kPTile, "one tile of trial periods per workgroup");
    constexpr bool CE = KIND == 2;   // counts only
    constexpr bool GL = false;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int64_t L = blockIdx.x;
    // dispatch position: the p with otile[p] <= L < otile[p + 1] (every listed curve has >= 1 tile)
    int64_t lo = 0, hi = ra.m - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (ra.otile[mid] <= L) lo = mid;
        else hi = mid - 1;
    }
    const int64_t curve = ra.order[lo];
    const int64_t tile = L - ra.otile[lo];
    const int64_t off = ra.offsets[curve];
    const int64_t n = ra.offsets[curve + 1] - off;
    const int64_t po = ra.poff[curve];
    const int64_t np = ra.poff[curve + 1] - po;
    const struct {
        const double *t, *x;
    } a{ra.t + off, ra.x + off};   // (the names pdm_chunks.inc reads)

    const int mag = KIND == 2 ? ra.nc : 1;
    const int m0 = CE ? ra.nb : ra.nb * ra.nc;
    const int nbins = (m0 + 1) * mag;
    double2 *stage = reinterpret_cast<double2 *>(lds_raw);
    constexpr int kStage = kChunk > BLOCK ? kChunk : BLOCK;
    double *hsum = reinterpret_cast<double *>(stage + kStage);
    const int ncw = CE ? (nbins + 1) / 2 : nbins;
    unsigned *hcnt = reinterpret_cast<unsigned *>(hsum + (CE ? 0 : (size_t)nbins * BLOCK));
    double *edge = reinterpret_cast<double *>(hcnt + (size_t)ncw * BLOCK);
    const int tid = threadIdx.x;

    for (int k = tid; k < m0 + 2; k += BLOCK) edge[k] = (double)k / (double)m0;
    for (int k = 0; k < nbins; ++k)
        if (!CE) hsum[k * BLOCK + tid] = 0.0;
    for (int k = 0; k < ncw; ++k) hcnt[k * BLOCK + tid] = 0u;

    const double mean = ra.stat[curve * 3 + 0], tmax = ra.stat[curve * 3 + 1], q_total = ra.stat[curve * 3 + 2];
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), part = wave % SPLIT;
    const int slot = (wave / SPLIT) * 64 + (tid & 63);
    const int64_t pidx = tile * kPTile + slot;
    const double period = pidx < np ? linspace_at(pidx, np, ra.start[curve], ra.step[curve], ra.stop[curve]) : 1.0;
    const double rp = 1.0 / period;
    const double dm0 = (double)m0;
    const double eps = dm0 * (8.9e-16 * tmax * __builtin_fabs(rp) + 8.9e-16);
    const double thr = 0.5 - eps;
    double q_over = 0.0;
    double q_nan = 0.0;
    const int64_t s_begin = 0, s_end = n;
#include "pdm_chunks.inc"
    if (part != 0 || pidx >= np) return;
    auto sum_at = [&](int b) { return hsum[b * BLOCK + tid]; };
    auto cnt_at = [&](int b) {
        return CE ? (long long)((hcnt[(b >> 1) * BLOCK + tid] >> ((b & 1) * 16)) & 0xFFFFu) : (long long)hcnt[b * BLOCK + tid];
    };
    double v;
    if (CE) v = ce_from_bins(cnt_at, m0, mag);
    else if (KIND == 1) v = aov_from_bins(sum_at, cnt_at, m0, q_total - q_nan);
    else v = theta_from_bins(sum_at, cnt_at, m0, ra.nc, q_total, q_nan, q_over, ra.sigma[curve]);
    ra.raw[po + pidx] = v;
}

// Sub-harmonic averaging (phase.py:_average_with_double_period) and the output rows of one curve.
template <bool DIP>
__global__ __launch_bounds__(kFinBlock) void pdm_ragged_finish_kernel(RaggedPhaseArgs ra) {
    const int64_t b = blockIdx.x;
    const int64_t po = ra.poff[b], np = ra.poff[b + 1] - po;
    const double start = ra.start[b], step = ra.step[b], stop = ra.stop[b];
    const bool sub = ra.signif != nullptr;   // (the host requires np >= 2 then)
    const double significant = sub ? ra.signif[b] : 0.0;
    const double spacing = sub ? linspace_at(1, np, start, step, stop) - linspace_at(0, np, start, step, stop) : 1.0;
    const double lead = start / spacing, half = stop / 2.0;
    // FSeries order is ascending frequency 1 / p: the reversed period index on an ascending grid, the period index
    // on a descending (or constant) one - for grids whose periods have one sign, which the caller ensures
    const bool rev = stop > start;
    const double *raw = ra.raw + po;
    for (int64_t j = threadIdx.x; j < np; j += kFinBlock) {
        double v = raw[j];
        if (sub && v < significant && linspace_at(j, np, start, step, stop) <= half) {
            // np.round(2 * here + shortest / spacing).astype(int): half-to-even, then numpy's indexing
            int64_t d = (int64_t)rint((double)(2 * j) + lead);
            if (d < 0) d += np;
            v = d >= 0 && d < np ? (v + raw[d]) / 2 : __builtin_nan("");
        }
        if (ra.out && ra.out != ra.raw) ra.out[po + j] = v;
        if (ra.pitched) ra.pitched[b * ra.pitch + (rev ? np - 1 - j : j)] = DIP ? -v : v;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
bool is_dip(int kind) { return kind != 1; }   // PDM theta and the conditional entropy are minimal at the period

// The one instance per statistic and bin counts: `last` = highest histogram bin, bytes per bin 12 (sum + count) or
// 4 (counts only), and whether the <256, 4> histogram fits 150 KB of LDS (else <64, 1>) - pdm.hip's choice.
struct Shape {
    int last, bpb, block;
    size_t lds;
};
Shape shape_of(int kind, int nb, int nc) {
    if (kind == 1) nc = 1;
    const int m0 = kind == 2 ? nb : nb * nc;
    Shape s;
    s.last = kind == 2 ? (nb + 1) * nc - 1 : m0;
    s.bpb = kind == 2 ? 4 : 12;
    s.block = lds_bytes(s.last, 256, s.bpb) > 150 * 1024 ? 64 : 256;
    s.lds = lds_bytes(s.last, s.block, s.bpb);
    return s;
}

// Workspace of one launch over B curves: per-curve statistics, the metadata tables, the scan's rows; with k > 0
// also the peak-table tail (ragged_table_bytes).
struct PhaseLayout {
    int64_t stat, meta, raw, pitched, total;
};
constexpr int kMetaArrays = 9;   // offsets | poff | otile | order (int64) | start | step | stop | sigma | signif, B + 1 each
enum { M_OFF, M_POFF, M_OTILE, M_ORDER, M_START, M_STEP, M_STOP, M_SIGMA, M_SIGNIF };

PhaseLayout phase_layout(int64_t n_curves, int64_t p_total, int64_t p_max, int k) {
    PhaseLayout w;
    Carve c;
    w.stat = c.take(n_curves * 24);
    w.meta = c.take(kMetaArrays * (n_curves + 1) * 8);
    w.raw = c.take(p_total * 8);
    w.pitched = c.at;
    w.total = w.pitched + ragged_table_bytes(n_curves, p_max, k);
    return w;
}

const char *kind_name(int kind) { return kind == 0 ? "pdm" : (kind == 1 ? "aov" : "cond_entropy"); }

// Checks the host-side description of a batch; the same text for every entry point.
int validate(const char *what, int kind, const int64_t *offsets, int64_t n_curves, const double *start,
             const double *step, const double *stop, const int64_t *poff, const double *sigma, const double *signif,
             int nb, int nc) {
    PDC_REQUIRE(kind >= 0 && kind <= 2, "%s: kind must be 0 (PDM), 1 (AoV) or 2 (conditional entropy), got %d", what, kind);
    PDC_REQUIRE(offsets && start && step && stop && poff, "%s: NULL argument", what);
    PDC_REQUIRE(kind != 0 || sigma, "%s: PDM needs sigma[]", what);
    PDC_REQUIRE(nb >= 1 && nc >= 1, "%s: bin counts must be positive", what);
    const Shape s = shape_of(kind, nb, nc);
    PDC_REQUIRE(s.last <= 190, "%s: %d histogram bins exceed the 191 that fit in LDS", what, s.last + 1);
    auto curve = [&](int64_t b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        PDC_REQUIRE(kind != 2 || n <= kCellSamples,
                    "%s: curve %lld has %lld samples; a conditional-entropy batch bins a whole curve in one workgroup "
                    "of 16-bit cells (at most %lld samples)", what, (long long)b, (long long)n, (long long)kCellSamples);
        PDC_REQUIRE(!signif || poff[b + 1] - poff[b] >= 2,
                    "%s: curve %lld: sub-harmonic averaging needs at least two trial periods", what, (long long)b);
        return PDC_OK;
    };
    return ragged_validate(what, offsets, poff, "p_offsets", n_curves, kPTile,
                           "periods: the grids are too large for one launch", curve);
}

template <typename Kernel>
int launch_scan(Kernel kernel, int block, const Shape &s, int64_t tiles, hipStream_t st, const RaggedPhaseArgs &a) {
    PDC_TRY(allow_dynamic_lds((const void *)kernel, 150 * 1024));
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3((unsigned)block), s.lds, st, a);
    return PDC_OK;
}

// Every launch of one group of curves.  Metadata come from the host (offsets, p_offsets rebased to the group), the
// sample arrays and the workspace are on the device.
int phase_ragged_dev(int kind, int device, hipStream_t st, const double *d_t, const double *d_x, const int64_t *offsets,
                     int64_t n_curves, const double *start, const double *step, const double *stop, const int64_t *poff,
                     const double *sigma, const double *signif, int nb, int nc, double *d_out, double *d_pitched,
                     int64_t pitch, void *work, int64_t work_bytes, std::vector<int64_t> &host_meta, bool wait_meta) {
    const int64_t n_total = offsets[n_curves], p_total = poff[n_curves];
    const PhaseLayout w = phase_layout(n_curves, p_total, 0, 0);   // (the pitched copy is the caller's)
    PDC_REQUIRE(work && work_bytes >= w.total, "phase_ragged: workspace too small (%lld < %lld bytes)",
                (long long)work_bytes, (long long)w.total);
    PDC_REQUIRE(n_total == 0 || (d_t && d_x), "phase_ragged: t and x must not be NULL");
    if (kind == 1) nc = 1;
    PDC_TRY(use_device(device));
    char *base = static_cast<char *>(work);
    // metadata: one upload; dispatch order = ragged_order (costliest curve first)
    RaggedMeta meta(host_meta, kMetaArrays, n_curves, base + w.meta);
    meta.fill_offsets(offsets, poff);
    meta.fill_linspace(M_START, start, step, stop);
    for (int64_t b = 0; b < n_curves; ++b) {
        meta.f64(M_SIGMA)[b] = sigma ? sigma[b] : 1.0;
        meta.f64(M_SIGNIF)[b] = signif ? signif[b] : 0.0;
    }
    const int64_t m = ragged_order(offsets, poff, n_curves, kPTile, meta.i64(M_ORDER), meta.i64(M_OTILE));
    const int64_t tiles = meta.i64(M_OTILE)[m];
    PDC_TRY(meta.upload(st, wait_meta));

    RaggedPhaseArgs a = {};
    a.t = d_t;
    a.x = d_x;
    a.offsets = meta.d_i64(M_OFF);
    a.poff = meta.d_i64(M_POFF);
    a.otile = meta.d_i64(M_OTILE);
    a.order = meta.d_i64(M_ORDER);
    a.start = meta.d_f64(M_START);
    a.step = meta.d_f64(M_STEP);
    a.stop = meta.d_f64(M_STOP);
    a.sigma = meta.d_f64(M_SIGMA);
    a.signif = signif ? meta.d_f64(M_SIGNIF) : nullptr;
    a.m = m;
    a.tiles = tiles;
    a.nb = nb;
    a.nc = nc;
    a.stat = reinterpret_cast<double *>(base + w.stat);
    // the scan writes the caller's rows directly unless the finishing pass still has to read them
    a.raw = d_out && !signif ? d_out : reinterpret_cast<double *>(base + w.raw);
    a.out = d_out;
    a.pitched = d_pitched;
    a.pitch = pitch;
    const Shape s = shape_of(kind, nb, nc);
    const bool ce = kind == 2;
    if (s.block == 64) {
        if (ce) hipLaunchKernelGGL((pdm_ragged_prep_kernel<64, true>), dim3((unsigned)n_curves), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((pdm_ragged_prep_kernel<64, false>), dim3((unsigned)n_curves), dim3(64), 0, st, a);
    } else {
        if (ce) hipLaunchKernelGGL((pdm_ragged_prep_kernel<256, true>), dim3((unsigned)n_curves), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((pdm_ragged_prep_kernel<256, false>), dim3((unsigned)n_curves), dim3(256), 0, st, a);
    }
    PDC_HIP(hipGetLastError());
    if (tiles > 0) {
        if (s.block == 64) {
            if (kind == 2) PDC_TRY(launch_scan(pdm_ragged_scan_kernel<64, 1, 2>, 64, s, tiles, st, a));
            else if (kind == 1) PDC_TRY(launch_scan(pdm_ragged_scan_kernel<64, 1, 1>, 64, s, tiles, st, a));
            else PDC_TRY(launch_scan(pdm_ragged_scan_kernel<64, 1, 0>, 64, s, tiles, st, a));
        } else {
            if (kind == 2) PDC_TRY(launch_scan(pdm_ragged_scan_kernel<256, 4, 2>, 256, s, tiles, st, a));
            else if (kind == 1) PDC_TRY(launch_scan(pdm_ragged_scan_kernel<256, 4, 1>, 256, s, tiles, st, a));
            else PDC_TRY(launch_scan(pdm_ragged_scan_kernel<256, 4, 0>, 256, s, tiles, st, a));
        }
        PDC_HIP(hipGetLastError());
    }
    if (signif || d_pitched) {
        if (is_dip(kind)) hipLaunchKernelGGL(pdm_ragged_finish_kernel<true>, dim3((unsigned)n_curves), dim3(kFinBlock), 0, st, a);
        else hipLaunchKernelGGL(pdm_ragged_finish_kernel<false>, dim3((unsigned)n_curves), dim3(kFinBlock), 0, st, a);
        PDC_HIP(hipGetLastError());
    }
    return PDC_OK;
}

// ---- host entries: ragged_run (ragged.hip) deals the curves to device slots and runs each slot's groups ----------
RaggedSlots g_slots;

// What one host call computes and where its results go (caller's host arrays, any may be NULL); rows = p_offsets.
struct PhaseJob : RaggedBatch {
    int kind, nb, nc;
    const double *t, *x;
    const double *start, *step, *stop, *sigma, *signif;
    double *out;

    PhaseJob(int kind_, const double *t_, const double *x_, const int64_t *offsets_, const double *start_,
             const double *step_, const double *stop_, const int64_t *p_offsets, const double *sigma_,
             const double *significant, int nb_, int nc_, double *out_)
        : kind(kind_), nb(nb_), nc(kind_ == 1 ? 1 : nc_), t(t_), x(x_), start(start_), step(step_), stop(stop_),
          sigma(kind_ == 0 ? sigma_ : nullptr), signif(significant), out(out_) {
        offsets = offsets_;
        rows = p_offsets;
        negate_heights = is_dip(kind_);
    }

    // The slot buffer of the group [c0, c1) whose longest grid has p_max periods: inputs | out | workspace.
    struct Bytes {
        int64_t in_t, in_x, out, work, total;
    };
    Bytes bytes(int64_t c0, int64_t c1, int64_t p_max) const {
        const int64_t n = offsets[c1] - offsets[c0], np = rows[c1] - rows[c0], B = c1 - c0;
        Bytes g;
        Carve c;
        g.in_t = c.take(n * 8);
        g.in_x = c.take(n * 8);
        g.out = c.take(out ? np * 8 : 0);
        g.work = c.at;
        g.total = g.work + phase_layout(B, np, p_max, k).total;
        return g;
    }
    int64_t group_bytes(int64_t c0, int64_t c1, int64_t p_max) const override { return bytes(c0, c1, p_max).total; }

    int run_group(RaggedSlot &s, int64_t c0, int64_t c1, int64_t p_max, double *pitched) const override {
        const RaggedGroup g(*this, s, c0, c1);
        const Bytes at = bytes(c0, c1, p_max);
        PDC_TRY(g.upload(at.in_t, t));
        PDC_TRY(g.upload(at.in_x, x));
        PDC_TRY(phase_ragged_dev(kind, s.device, g.st, g.at<double>(at.in_t), g.at<double>(at.in_x), g.off.data(), g.B,
                                 start + c0, step + c0, stop + c0, g.roff.data(), sigma ? sigma + c0 : nullptr,
                                 signif ? signif + c0 : nullptr, nb, nc, g.at_if<double>(out, at.out), pitched, p_max,
                                 g.buf + at.work, at.total - at.work, s.meta, false));
        return g.rows_back(out, at.out);
    }
};

int phase_host(const char *what, const PhaseJob &j, int64_t n_curves, const int *devices, int n_devices) {
    PDC_REQUIRE(j.offsets[n_curves] == 0 || (j.t && j.x), "%s: t and x must not be NULL", what);
    if (j.kind == 2)   // the magnitude bins index the cell histogram: reject what is not one of 0 .. n_mag-1
        for (int64_t b = 0; b < n_curves; ++b)
            for (int64_t i = j.offsets[b]; i < j.offsets[b + 1]; ++i)
                PDC_REQUIRE(j.x[i] >= 0.0 && j.x[i] < (double)j.nc,
                            "%s: curve %lld: mag_bin[%lld] = %g is not a bin index in 0 .. %d", what, (long long)b,
                            (long long)(i - j.offsets[b]), j.x[i], j.nc - 1);
    return ragged_run(what, g_slots, j, n_curves, devices, n_devices);
}

}  // namespace

// Frees the per-slot buffers and streams of the ragged phase-scan host entries (pdc_release()).
int pdc::release_phase_ragged() { return g_slots.release(); }

extern "C" {

int pdc_test_phase_ragged_groups(int64_t *groups) {
    PDC_REQUIRE(groups, "pdc_test_phase_ragged_groups: NULL argument");
    std::lock_guard<std::mutex> lk(g_slots.mutex);
    *groups = g_slots.groups;
    return PDC_OK;
}

int64_t pdc_phase_ragged_work_bytes(int64_t n_curves, int64_t p_total, int64_t p_max, int k) {
    if (n_curves < 1 || p_total < 0 || p_max < 0 || k < 0) return -1;
    return phase_layout(n_curves, p_total, p_max, k).total;
}

int pdc_phase_scan_ragged_dev(int kind, int device, void *stream, const double *d_t, const double *d_x,
                              const int64_t *offsets, int64_t n_curves, const double *start, const double *step,
                              const double *stop, const int64_t *p_offsets, const double *sigma,
                              const double *significant, int nb, int nc, double *d_out, double *d_pitched, int64_t pitch,
                              void *work, int64_t work_bytes) {
    PDC_TRY(validate("phase_ragged_dev", kind, offsets, n_curves, start, step, stop, p_offsets, sigma, significant, nb, nc));
    PDC_REQUIRE(d_out || d_pitched, "phase_ragged_dev: no output requested");
    if (d_pitched) PDC_TRY(ragged_check_pitch("phase_ragged_dev", p_offsets, n_curves, pitch, "periods"));
    std::vector<int64_t> meta;
    return phase_ragged_dev(kind, device, (hipStream_t)stream, d_t, d_x, offsets, n_curves, start, step, stop, p_offsets,
                            kind == 0 ? sigma : nullptr, significant, nb, nc, d_out, d_pitched, pitch, work, work_bytes,
                            meta, true);
}

int pdc_phase_scan_ragged(int kind, const double *t, const double *x, const int64_t *offsets, int64_t n_curves,
                          const double *start, const double *step, const double *stop, const int64_t *p_offsets,
                          const double *sigma, const double *significant, int nb, int nc, double *out,
                          const int *devices, int n_devices) {
    PDC_TRY(validate("phase_ragged", kind, offsets, n_curves, start, step, stop, p_offsets, sigma, significant, nb, nc));
    PDC_REQUIRE(out, "phase_ragged: no output requested");
    const PhaseJob j(kind, t, x, offsets, start, step, stop, p_offsets, sigma, significant, nb, nc, out);
    return phase_host(kind_name(kind), j, n_curves, devices, n_devices);
}

int pdc_phase_ragged_peaks(int kind, const double *t, const double *x, const int64_t *offsets, int64_t n_curves,
                           const double *start, const double *step, const double *stop, const int64_t *p_offsets,
                           const double *sigma, const double *significant, int nb, int nc, int k, int by_prominence,
                           int64_t *count_out, int64_t *idx_out, double *height_out, double *prominence_out,
                           int64_t *half_lo_out, int64_t *half_hi_out, double *out, const int *devices, int n_devices) {
    PDC_TRY(validate("phase_ragged_peaks", kind, offsets, n_curves, start, step, stop, p_offsets, sigma, significant, nb,
                     nc));
    PhaseJob j(kind, t, x, offsets, start, step, stop, p_offsets, sigma, significant, nb, nc, out);
    PDC_TRY(j.want_table("phase_ragged_peaks", k, by_prominence, count_out, idx_out, height_out, prominence_out,
                         half_lo_out, half_hi_out, out != nullptr));
    return phase_host(kind_name(kind), j, n_curves, devices, n_devices);
}

}  // extern "C"
