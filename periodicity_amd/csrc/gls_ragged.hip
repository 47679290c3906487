// GLS over a batch of light curves that each keep their OWN frequency grid ("ragged" grids): GLS.batch.
//
// A survey runs GLS()(s) and period_at_highest_peak over a catalogue (reference spectral.py:88-132 per
// curve, then core.py:944-978 on each result; its own batch is the bootstrap loop at spectral.py:140-152).
// GLS builds each curve's grid from that curve's data - df = 1/(baseline n), fmin = df/2, fmax =
// 0.5/median_dt (spectral.py:88-97) - so two curves almost never share one, and the shared-grid batch of
// gls.hip does not apply.  Here curve b owns samples [offsets[b], offsets[b+1]) and bins
// f0[b] + j delta[b], j < nf_b = f_offsets[b+1] - f_offsets[b] (numpy's arange fill rule), written to
// power[f_offsets[b] + j].
//
// Decomposition
//   gls_ragged_prep_kernel   one workgroup per curve: the weights, centring, YY and time origin t0 = t[0]
//                            of gls_prep_kernel, and the same 48-byte record per sample, rotated by the
//                            curve's own delta[b].
//   gls_ragged_scan_kernel   one workgroup per (curve, tile of 1024 bins), found by a scalar binary search
//                            in a tile prefix table.  The rotation tables, the scalar pipeline and the
//                            three-term recurrence are the shared ones of gls_sums.h (K = 8, one wave per
//                            64-lane column, two columns); the epilogue (gls_epilogue.h) is fused.  Tiles
//                            are dispatched costliest curve first (ragged_order, cost ~ n_b), so that the long
//                            curves do not run alone at the end of the launch.  Optionally also writes a pitched
//                            [B][pitch] copy of the spectra (the caller fills the pad with NaN) for the
//                            peak table of peaks.hip.
//   gls_ragged_peak_kernel   NaN-aware max / argmax per curve from the per-tile partials (the rule of
//                            gls_peak_kernel: first maximum on ties, -1 / NaN for a row without a finite bin).
//
// The host entries' device slots, groups, budget and peak table are the shared driver's (ragged.hip); this unit
// sizes and runs one group.  Designed for survey curves (1e2 - 1e4 samples, grids of ~2.5 N bins): no sample parts,
// no balanced pieces (one huge curve has its own path in gls.hip).
#include "pdc_internal.h"
#include "gls_epilogue.h"
#include "gls_sums.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace pdc;

namespace {

constexpr int kRK = 8;                    // trial frequencies per thread
constexpr int kRBlock = 128;              // two waves: one 64-lane column of frequencies each
constexpr int kRCols = kRBlock / 64;
constexpr int64_t kRTile = (int64_t)kRBlock * kRK;   // 1024 bins per tile
constexpr int kRChunk = 64;               // samples per rotation-table chunk: two threads per sample = the block
constexpr int kRPrepBlock = 256;

struct RaggedPrepArgs {
    const double *t, *y, *dy;      // dy may be NULL (unit errors)
    const int64_t *offsets;        // [B + 1]
    const double *delta;           // [B]
    int fit_mean;
    double *rec;                   // [n_total][6]
    double *scal;                  // [B][4] = {YY, sum w, sum err^-2, t0}
};

struct RaggedArgs {
    const double *rec, *scal;
    const int64_t *offsets, *foff;   // [B + 1] samples, bins
    const double *f0, *delta;        // [B]
    const int64_t *ctile;            // [B + 1] tile prefix in curve order (where a tile's partial goes)
    const int64_t *otile;            // [m + 1] tile prefix in dispatch order (curves with >= 1 tile only)
    const int64_t *order;            // [m] curve at each dispatch position
    int64_t m, tiles;
    int psd;
    double *power;                   // [nf_total] or nullptr
    double *pitched;                 // [B][pitch] or nullptr
    int64_t pitch;
    double *blk_max;                 // [tiles] or nullptr
    int64_t *blk_arg;
};

// ---- prologue: spectral.py:99-108, 120, per curve, rotated by the curve's own delta (gls_sums.h) ---------------
__global__ __launch_bounds__(kRPrepBlock) void gls_ragged_prep_kernel(RaggedPrepArgs a) {
    __shared__ double red[kRPrepBlock / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t off = a.offsets[b];
    const int64_t n = a.offsets[b + 1] - off;
    const double *t = a.t + off;
    const double *y = a.y + off;
    const double *dy = a.dy ? a.dy + off : nullptr;
    const double t0 = n > 0 ? t[0] : 0.0;
    const double delta = a.delta[b];
    double W, ybar;
    weights_and_mean<kRPrepBlock>(y, dy, n, a.fit_mean, red, W, ybar);
    double yy = 0.0, wsum = 0.0;
    double *rec = a.rec + off * 6;
    for (int64_t i = tid; i < n; i += kRPrepBlock) {
        const double tp = t[i] - t0;
        const double w = inv_var(dy, i) / W;
        const double yc = y[i] - ybar;
        const double wy = w * yc;
        yy += wy * yc;
        wsum += w;
        const double rw = sqrt(w);  // the scan carries sqrt(w) sin / sqrt(w) cos
        put_record(rec + i * 6, rw * yc, rw, delta, tp);
    }
    yy = block_sum<kRPrepBlock>(yy, red);
    wsum = block_sum<kRPrepBlock>(wsum, red);
    if (tid == 0) {
        double *s = a.scal + b * 4;
        s[0] = yy;
        s[1] = wsum;
        s[2] = W;
        s[3] = t0;
    }
}

// ---- the scan: a (curve, tile) lookup per workgroup, then the pieces of gls_sums.h at K = 8 -----------------
template <bool FIT_MEAN>
__global__ __launch_bounds__(kRBlock) void gls_ragged_scan_kernel(RaggedArgs a) {
    // per sample: {sin, cos} of theta_tile + 8 q Theta, q < 8 COLS, scaled by sqrt(w) | {sin, cos}(b Theta), b < 8
    __shared__ double2 tab[kRChunk + 1][kRCols * 8 + 8 + 1];   // + 1 row: the read-ahead; + 1 column: bank spread
    __shared__ double red_v[kRBlock / 64];
    __shared__ long long red_i[kRBlock / 64];
    const int tid = threadIdx.x;
    const int64_t L = blockIdx.x;
    if (L >= a.tiles) return;
    // dispatch position: the p with otile[p] <= L < otile[p + 1] (every listed curve has >= 1 tile)
    int64_t lo = 0, hi = a.m - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.otile[mid] <= L) lo = mid;
        else hi = mid - 1;
    }
    const int64_t curve = a.order[lo];
    const int64_t tile = L - a.otile[lo];
    const int64_t off = a.offsets[curve];
    const int64_t n = a.offsets[curve + 1] - off;
    const int64_t fo = a.foff[curve];
    const int64_t nf = a.foff[curve + 1] - fo;
    const double f0 = a.f0[curve], delta = a.delta[curve];
    const int col = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t jt = tile * kRTile;
    const int64_t jl = jt + (col * 64 + lane) * (int64_t)kRK;
    // numpy's arange fill rule: start + i*delta, two roundings (no fma)
    const double f_tile = __dadd_rn(f0, __dmul_rn((double)jt, delta));
    const double kdelta = (double)kRK * delta;   // spacing of the threads' first frequencies (exact)

    double Sh[kRK], Ch[kRK], S[kRK], C[kRK], SS[kRK], SC[kRK];
#pragma unroll
    for (int k = 0; k < kRK; ++k) Sh[k] = Ch[k] = S[k] = C[k] = SS[k] = SC[k] = 0.0;

    const int slot_a = col * 8 + (lane >> 3), slot_b = kRCols * 8 + (lane & 7);
    const double *recs = a.rec + off * 6;   // (the workspace keeps the two spare records after the last curve)
    scan_stretch<kRChunk, kRK>(
        tab, recs, n, 0, n, tid, slot_a, slot_b,
        [&](double2 *row, const int64_t i, const bool real) {   // two threads per sample: the whole block
            const double tp = real ? recs[i * 6 + 5] : 0.0;
            const double sqw = real ? recs[i * 6 + 1] : 0.0;
            fill_rotation_tables<kRCols>(row, tid & 1, tp, kdelta, f_tile, sqw);
        },
        [&](const Ahead &h, const int k, const double s, const double c) {
            const double wy = h.r[0], w = h.r[1];
            Sh[k] = __builtin_fma(wy, s, Sh[k]);
            Ch[k] = __builtin_fma(wy, c, Ch[k]);
            if (FIT_MEAN) {
                S[k] = __builtin_fma(w, s, S[k]);
                C[k] = __builtin_fma(w, c, C[k]);
            }
            SS[k] = __builtin_fma(s, s, SS[k]);
            SC[k] = __builtin_fma(s, c, SC[k]);
        });

    // fused epilogue (spectral.py:113-132); the 2-omega sums from sin 2a = 2 sin a cos a, cos 2a = 1 - 2 sin^2 a
    const double *sc = a.scal + curve * 4;
    const double YY = sc[0], Wsum = sc[1], Werr = sc[2];
    ArgMax best;
#pragma unroll
    for (int k = 0; k < kRK; ++k) {
        const int64_t j = jl + k;
        if (j < nf) {
            const double p = gls_power_from_sums<FIT_MEAN>(Sh[k], Ch[k], S[k], C[k], 2.0 * SC[k], Wsum - 2.0 * SS[k],
                                                           YY, Werr, a.psd);
            if (a.power) a.power[fo + j] = p;
            if (a.pitched) a.pitched[curve * a.pitch + j] = p;
            best.take(p, j);
        }
    }
    if (a.blk_max && best.block_fold<kRBlock / 64>(red_v, red_i, lane, col)) {   // lanes hold ascending index ranges
        const int64_t at = a.ctile[curve] + tile;
        a.blk_max[at] = best.v;
        a.blk_arg[at] = best.j;
    }
}

// per curve: the tile partials [ctile[b], ctile[b + 1]) folded in ascending order (gls_peak_kernel's rule)
__global__ __launch_bounds__(64) void gls_ragged_peak_kernel(const double *blk_max, const int64_t *blk_arg,
                                                             const int64_t *ctile, double *amax, int64_t *argmax) {
    const int64_t curve = blockIdx.x;
    const int64_t t0 = ctile[curve], t1 = ctile[curve + 1];
    ArgMax best;
    for (int64_t i = t0 + threadIdx.x; i < t1; i += 64) best.take_later(blk_max[i], blk_arg[i]);
    best.wave_fold();
    if (threadIdx.x == 0) {
        if (amax) amax[curve] = best.j >= 0 ? best.v : __builtin_nan("");
        if (argmax) argmax[curve] = best.j;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
int64_t tiles_of(int64_t nf) { return (nf + kRTile - 1) / kRTile; }

// Workspace of one launch over B curves: records (+ two spare ones for the scan's read-ahead), per-curve scalars,
// the metadata tables, the tile partials; with k > 0 also the peak-table tail (ragged_table_bytes).
struct RaggedLayout {
    int64_t rec, scal, meta, blk_max, blk_arg, pitched, total;
};
constexpr int kMetaArrays = 7;   // offsets | foff | ctile | otile | order (int64) | f0 | delta (double), B + 1 each
enum { M_OFF, M_FOFF, M_CTILE, M_OTILE, M_ORDER, M_F0, M_DELTA };

RaggedLayout ragged_layout(int64_t n_total, int64_t n_curves, int64_t nf_total, int64_t nf_max, int k) {
    const int64_t tiles_max = nf_total / kRTile + n_curves;   // >= sum of ceil(nf_b / 1024)
    RaggedLayout w;
    Carve c;
    w.rec = c.take((n_total + 2) * 48);
    w.scal = c.take(n_curves * 32);
    w.meta = c.take(kMetaArrays * (n_curves + 1) * 8);
    w.blk_max = c.take(tiles_max * 8);
    w.blk_arg = c.take(tiles_max * 8);
    w.pitched = c.at;
    w.total = w.pitched + ragged_table_bytes(n_curves, nf_max, k);
    return w;
}

// Checks the host-side description of a batch; the same text for every entry point.
int validate(const char *what, const int64_t *offsets, int64_t n_curves, const double *f0, const double *delta,
             const int64_t *f_offsets) {
    PDC_REQUIRE(offsets && f0 && delta && f_offsets, "%s: NULL argument", what);
    auto grid = [&](int64_t b) {
        PDC_REQUIRE(std::isfinite(f0[b]) && std::isfinite(delta[b]) && delta[b] > 0.0,
                    "%s: curve %lld: f0 and delta must be finite and delta > 0 (f0 = %g, delta = %g)", what, (long long)b,
                    f0[b], delta[b]);
        return PDC_OK;
    };
    return ragged_validate(what, offsets, f_offsets, "f_offsets", n_curves, kRTile,
                           "bins: the grid is too large for one launch", grid);
}

// Every workgroup-visible launch of one group of curves.  Metadata come from the host (offsets, f_offsets rebased
// to the group), the sample arrays and the workspace are on the device.
int ragged_dev(int device, hipStream_t st, const double *d_t, const double *d_y, const double *d_dy,
               const int64_t *offsets, int64_t n_curves, const double *f0, const double *delta, const int64_t *foff,
               int fit_mean, int psd, double *d_power, double *d_pitched, int64_t pitch, double *d_amax,
               int64_t *d_argmax, void *work, int64_t work_bytes, std::vector<int64_t> &host_meta, bool wait_meta) {
    const int64_t n_total = offsets[n_curves], nf_total = foff[n_curves];
    const RaggedLayout w = ragged_layout(n_total, n_curves, nf_total, 0, 0);   // (the pitched copy is the caller's)
    PDC_REQUIRE(work && work_bytes >= w.total, "gls_ragged: workspace too small (%lld < %lld bytes)",
                (long long)work_bytes, (long long)w.total);
    PDC_REQUIRE(n_total == 0 || (d_t && d_y), "gls_ragged: t and y must not be NULL");
    PDC_TRY(use_device(device));
    char *base = static_cast<char *>(work);
    // metadata: one upload; dispatch order = ragged_order (costliest curve first)
    RaggedMeta meta(host_meta, kMetaArrays, n_curves, base + w.meta);
    meta.fill_offsets(offsets, foff);
    std::copy(f0, f0 + n_curves, meta.f64(M_F0));
    std::copy(delta, delta + n_curves, meta.f64(M_DELTA));
    int64_t *m_ctile = meta.i64(M_CTILE);
    for (int64_t b = 0; b < n_curves; ++b) m_ctile[b + 1] = m_ctile[b] + tiles_of(foff[b + 1] - foff[b]);
    const int64_t m = ragged_order(offsets, foff, n_curves, kRTile, meta.i64(M_ORDER), meta.i64(M_OTILE));
    const int64_t tiles = m_ctile[n_curves];
    PDC_TRY(meta.upload(st, wait_meta));

    RaggedPrepArgs p;
    p.t = d_t;
    p.y = d_y;
    p.dy = d_dy;
    p.offsets = meta.d_i64(M_OFF);
    p.delta = meta.d_f64(M_DELTA);
    p.fit_mean = fit_mean;
    p.rec = reinterpret_cast<double *>(base + w.rec);
    p.scal = reinterpret_cast<double *>(base + w.scal);
    hipLaunchKernelGGL(gls_ragged_prep_kernel, dim3((unsigned)n_curves), dim3(kRPrepBlock), 0, st, p);
    PDC_HIP(hipGetLastError());
    const bool peaks = d_amax || d_argmax;
    if (tiles > 0) {
        RaggedArgs a;
        a.rec = p.rec;
        a.scal = p.scal;
        a.offsets = p.offsets;
        a.foff = meta.d_i64(M_FOFF);
        a.f0 = meta.d_f64(M_F0);
        a.delta = p.delta;
        a.ctile = meta.d_i64(M_CTILE);
        a.otile = meta.d_i64(M_OTILE);
        a.order = meta.d_i64(M_ORDER);
        a.m = m;
        a.tiles = tiles;
        a.psd = psd;
        a.power = d_power;
        a.pitched = d_pitched;
        a.pitch = pitch;
        a.blk_max = peaks ? reinterpret_cast<double *>(base + w.blk_max) : nullptr;
        a.blk_arg = peaks ? reinterpret_cast<int64_t *>(base + w.blk_arg) : nullptr;
        if (fit_mean) hipLaunchKernelGGL(gls_ragged_scan_kernel<true>, dim3((unsigned)tiles), dim3(kRBlock), 0, st, a);
        else hipLaunchKernelGGL(gls_ragged_scan_kernel<false>, dim3((unsigned)tiles), dim3(kRBlock), 0, st, a);
        PDC_HIP(hipGetLastError());
    }
    if (peaks) {
        hipLaunchKernelGGL(gls_ragged_peak_kernel, dim3((unsigned)n_curves), dim3(64), 0, st,
                           reinterpret_cast<const double *>(base + w.blk_max),
                           reinterpret_cast<const int64_t *>(base + w.blk_arg), meta.d_i64(M_CTILE), d_amax, d_argmax);
        PDC_HIP(hipGetLastError());
    }
    return PDC_OK;
}

// ---- host entries: ragged_run (ragged.hip) deals the curves to device slots and runs each slot's groups ----------
RaggedSlots g_slots;

// What one host call computes and where its results go (caller's host arrays, any may be NULL); rows = f_offsets.
struct RaggedJob : RaggedBatch {
    const double *t, *y, *dy;
    const double *f0, *delta;
    int fit_mean, psd;
    double *power, *amax = nullptr;
    int64_t *argmax = nullptr;

    RaggedJob(const double *t_, const double *y_, const double *dy_, const int64_t *offsets_, const double *f0_,
              const double *delta_, const int64_t *f_offsets, int fit_mean_, int psd_, double *power_out)
        : t(t_), y(y_), dy(dy_), f0(f0_), delta(delta_), fit_mean(fit_mean_ ? 1 : 0), psd(psd_ ? 1 : 0), power(power_out) {
        offsets = offsets_;
        rows = f_offsets;
    }

    // The slot buffer of the group [c0, c1) whose longest grid has nf_max bins: inputs | power | amax | argmax | workspace.
    struct Bytes {
        int64_t in_t, in_y, in_dy, pow, amax, arg, work, total;
    };
    Bytes bytes(int64_t c0, int64_t c1, int64_t nf_max) const {
        const int64_t n = offsets[c1] - offsets[c0], nf = rows[c1] - rows[c0], B = c1 - c0;
        Bytes g;
        Carve c;
        g.in_t = c.take(n * 8);
        g.in_y = c.take(n * 8);
        g.in_dy = c.take(dy ? n * 8 : 0);
        g.pow = c.take(power ? nf * 8 : 0);
        g.amax = c.take(amax ? B * 8 : 0);
        g.arg = c.take(argmax ? B * 8 : 0);
        g.work = c.at;
        g.total = g.work + ragged_layout(n, B, nf, nf_max, k).total;
        return g;
    }
    int64_t group_bytes(int64_t c0, int64_t c1, int64_t nf_max) const override { return bytes(c0, c1, nf_max).total; }

    int run_group(RaggedSlot &s, int64_t c0, int64_t c1, int64_t nf_max, double *pitched) const override {
        const RaggedGroup g(*this, s, c0, c1);
        const Bytes at = bytes(c0, c1, nf_max);
        PDC_TRY(g.upload(at.in_t, t));
        PDC_TRY(g.upload(at.in_y, y));
        PDC_TRY(g.upload(at.in_dy, dy));
        PDC_TRY(ragged_dev(s.device, g.st, g.at<double>(at.in_t), g.at<double>(at.in_y), g.at_if<double>(dy, at.in_dy),
                           g.off.data(), g.B, f0 + c0, delta + c0, g.roff.data(), fit_mean, psd,
                           g.at_if<double>(power, at.pow), pitched, nf_max, g.at_if<double>(amax, at.amax),
                           g.at_if<int64_t>(argmax, at.arg), g.buf + at.work, at.total - at.work, s.meta, false));
        PDC_TRY(g.rows_back(power, at.pow));
        PDC_TRY(g.curves_back(amax, at.amax));
        return g.curves_back(argmax, at.arg);
    }
};

int ragged_host(const char *what, const RaggedJob &j, int64_t n_curves, const int *devices, int n_devices) {
    PDC_REQUIRE(j.offsets[n_curves] == 0 || (j.t && j.y), "%s: t and y must not be NULL", what);
    return ragged_run(what, g_slots, j, n_curves, devices, n_devices);
}

}  // namespace

// Frees the per-slot buffers and streams of the ragged host entries (pdc_release()).
int pdc::release_ragged() { return g_slots.release(); }

extern "C" {

int64_t pdc_gls_ragged_work_bytes(int64_t n_total, int64_t n_curves, int64_t nf_total, int64_t nf_max, int k) {
    if (n_total < 0 || n_curves < 1 || nf_total < 0 || nf_max < 0 || k < 0) return -1;
    return ragged_layout(n_total, n_curves, nf_total, nf_max, k).total;
}

int pdc_gls_scan_ragged_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy,
                            const int64_t *offsets, int64_t n_curves, const double *f0, const double *delta,
                            const int64_t *f_offsets, int fit_mean, int psd, double *d_power, double *d_pitched,
                            int64_t pitch, double *d_amax, int64_t *d_argmax, void *work, int64_t work_bytes) {
    PDC_TRY(validate("gls_ragged_dev", offsets, n_curves, f0, delta, f_offsets));
    PDC_REQUIRE(d_power || d_pitched || d_amax || d_argmax, "gls_ragged_dev: no output requested");
    if (d_pitched) PDC_TRY(ragged_check_pitch("gls_ragged_dev", f_offsets, n_curves, pitch, "bins"));
    std::vector<int64_t> meta;
    return ragged_dev(device, (hipStream_t)stream, d_t, d_y, d_dy, offsets, n_curves, f0, delta, f_offsets, fit_mean, psd,
                      d_power, d_pitched, pitch, d_amax, d_argmax, work, work_bytes, meta, true);
}

int pdc_gls_scan_ragged(const double *t, const double *y, const double *dy, const int64_t *offsets, int64_t n_curves,
                        const double *f0, const double *delta, const int64_t *f_offsets, int fit_mean, int psd,
                        double *power_out, double *amax_out, int64_t *argmax_out, const int *devices, int n_devices) {
    PDC_TRY(validate("gls_ragged", offsets, n_curves, f0, delta, f_offsets));
    PDC_REQUIRE(power_out || amax_out || argmax_out, "gls_ragged: no output requested");
    RaggedJob j(t, y, dy, offsets, f0, delta, f_offsets, fit_mean, psd, power_out);
    j.amax = amax_out;
    j.argmax = argmax_out;
    return ragged_host("gls_ragged", j, n_curves, devices, n_devices);
}

int pdc_gls_ragged_peaks(const double *t, const double *y, const double *dy, const int64_t *offsets, int64_t n_curves,
                         const double *f0, const double *delta, const int64_t *f_offsets, int fit_mean, int psd, int k,
                         int by_prominence, int64_t *count_out, int64_t *idx_out, double *height_out,
                         double *prominence_out, int64_t *half_lo_out, int64_t *half_hi_out, double *power_out,
                         const int *devices, int n_devices) {
    PDC_TRY(validate("gls_ragged_peaks", offsets, n_curves, f0, delta, f_offsets));
    RaggedJob j(t, y, dy, offsets, f0, delta, f_offsets, fit_mean, psd, power_out);
    PDC_TRY(j.want_table("gls_ragged_peaks", k, by_prominence, count_out, idx_out, height_out, prominence_out, half_lo_out,
                         half_hi_out, power_out != nullptr));
    return ragged_host("gls_ragged_peaks", j, n_curves, devices, n_devices);
}

}  // extern "C"
