// Weighted wavelet Z-transform (Foster 1996, AJ 112, 1709) of an unevenly sampled curve as an exact direct summation on
// gfx950: at every (time shift tau, trial frequency f) the weighted least-squares fit of a constant plus a sinusoid under
// a Gaussian window whose width scales with the period,
//     w_i = err_i^-2 exp(-c omega^2 (t_i - tau)^2),   omega = 2 pi f,
// reduced on the device to the ridge (per tau the best frequency) and the best cell.  Definitions: periodicity_hip.h.
//
// The reference has no such statistic (its timefrequency.WPS needs even sampling): PARITY UNPINNED BY THE REFERENCE.
//
// Decomposition
//   wwz_prep_kernel     one workgroup: s_i = err^-2 / sum err^-2, the global weighted mean, one 48-byte record per sample
//                       {y - mean, s, cos(2 pi delta t'), sin(2 pi delta t'), 2 cos(2 pi delta t'), t' = t - t[0]}.
//   wwz_bounds_kernel   one thread per (tau, tile): the support [lo, hi) of the tile, two binary searches over the sorted
//                       times for the samples whose exponent c (2 pi f_lo)^2 (t - tau)^2 at the tile's LOWEST frequency
//                       is at most 746 - past it the weight is exactly 0 in fp64 at every frequency of the tile.
//   wwz_scan_kernel<K>  blockIdx = (tile, tau row of the launch).  One workgroup streams the samples [lo, hi) through
//                       scan_stretch (gls_sums.h): trig from the rotation tables and walk_grid, unchanged.  The window
//                       along a thread's K consecutive frequencies is a Gaussian in the bin index, so it follows
//                           g[k+1] = g[k] r[k],  r[k+1] = r[k] q,  q = exp(-2 A delta^2),  A = c (2 pi)^2 (t - tau)^2:
//                       two multiplies per pair, products only, every factor <= 1.  A and q are made once per (sample,
//                       tile) by the threads that fill the rotation tables and wait in LDS; the seeds g[0] = exp(-A f^2)
//                       and r[0] = exp(-A delta (2 f + delta)) at the thread's first frequency f are one software exp
//                       each per (sample, thread), amortised over K.  Ten running sums per frequency (20 K VGPRs):
//                       sum w, w^2, w c, w s, w c^2, w c s, w y, w y c, w y s, w y^2; sum w s^2 = sum w - sum w c^2.
//                       Epilogue: S, the 3 x 3 Cholesky with its back substitution (the amplitude needs the coefficients,
//                       which cholesky_quadratic of harmonic_sums.h does not give: typed out here), the three planes where
//                       taken, and one ArgMax partial (value, bin, amplitude) per (tau, tile) over the eligible bins.
//   wwz_fold_kernel     one workgroup: per tau the tiles in ascending order into the ridge, the ridge in ascending row
//                       order into the best cell, the support sizes into `visited`.
// No atomics: the same bits from call to call.  A launch takes at most 65535 rows; the partials of every row stay in the
// workspace and the fold runs once behind the last launch, so no bit depends on the rows per launch.
// No sample parts: a plane of few tiles x few tau underfills the device.
#include "pdc_internal.h"
#include "gls_sums.h"

#include <cmath>

using namespace pdc;

namespace {

constexpr int kBlock = 256;
constexpr int kPrepBlock = 1024;
constexpr int kChunk = 64;       // samples per rotation-table chunk
constexpr int kFreqs = 8;        // frequencies per thread
constexpr int kTile = kBlock * kFreqs;
constexpr int64_t kMaxRows = 65535;     // rows of one launch (the grid's second dimension)
constexpr double kCutExponent = 746.0;  // exp(-x) is exactly 0 in fp64 from x = 745.14 on

struct WwzPrepArgs {
    const double *t, *y, *dy;
    int64_t n;
    double delta;
    double *rec;   // [n + 2][6] (the scan reads one record ahead)
};

struct WwzPart {   // one (tau, tile): the support, and what the scan leaves for the fold
    int64_t lo, hi;   // samples [lo, hi)
    double v, amp;    // the tile's best eligible WWZ and its amplitude
    int64_t j;        // its bin, -1: none
};

struct WwzArgs {
    const double *rec, *t, *tau;   // tau: [ntau] on the device
    int64_t n, tiles, ntau, nf;
    double f0, delta, cdecay, min_neff;   // cdecay = c (2 pi)^2
    int64_t row0;                         // first row of this launch
    WwzPart *part;                        // [ntau][tiles]
    double *wwz, *amp, *neff;             // [ntau][nf] planes | NULL
    double *ridge_wwz, *ridge_amp;        // [ntau] (outputs, or workspace where the caller takes none)
    int64_t *ridge_bin;
    double *best;                         // [1] | NULL
    int64_t *best_at, *visited;           // [2] (row, bin) | NULL, [1] | NULL
};

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// f0 + j delta by numpy's arange fill rule: two roundings, no fma
__device__ __forceinline__ double grid_frequency(double f0, double delta, int64_t j) {
    return __dadd_rn(f0, __dmul_rn((double)j, delta));
}

// exp(-x) for x >= 0 (gfx950 has no fp64 transcendental unit): x = k ln 2 - r with |r| <= ln 2 / 2 in two exact steps,
// the Taylor series of exp(r / 64) to degree 5 (|r / 64| <= 0.0055: remainder 4e-17), six squarings, ldexp: five fma
// and six multiplies, and three literal coefficients where the series in r itself takes twelve - every literal of the
// hot loop costs an SGPR pair across it.  Rounding: 64 times that of 1 + r / 64, 7e-15 relative, next to the 8e-14 that
// the rounding of an exponent of 746 costs anyway.  Denormal results round once, in ldexp; from x = 745.14 on the result
// is exactly 0, as np.exp gives it.  x is clamped at 800 so that k stays an int; a NaN gives 0.
__device__ __forceinline__ double exp_neg(double x) {
    const double t = -__builtin_fmin(x, 800.0);
    const double kf = __builtin_rint(t * 1.44269504088896338700e+00);
    double r = __builtin_fma(kf, -6.93147180369123816490e-01, t);   // ln 2, high part: 32 trailing zero bits
    r = ldexp(__builtin_fma(kf, -1.90821492927058770002e-10, r), -6);
    double p = 1.0 / 120.0;
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
#pragma unroll
    for (int sq = 0; sq < 6; ++sq) p *= p;
    return ldexp(p, (int)kf);
}

// ---- prologue: weights as GLS takes them, y centred on its global weighted mean ----------------------------------------
__global__ __launch_bounds__(kPrepBlock) void wwz_prep_kernel(WwzPrepArgs a) {
    __shared__ double red[kPrepBlock / 64];
    const int tid = threadIdx.x;
    const double t0 = a.t[0];
    double W, ybar;
    weights_and_mean<kPrepBlock>(a.y, a.dy, a.n, 1, red, W, ybar);
    for (int64_t i = tid; i < a.n; i += kPrepBlock)
        put_record(a.rec + i * 6, a.y[i] - ybar, inv_var(a.dy, i) / W, a.delta, a.t[i] - t0);
    put_spare_records(a.rec, a.n, tid);
}

// ---- support cut -------------------------------------------------------------------------------------------------------
// Times never decrease, so on either side of tau the exponent at f_lo is monotone in the sample index: lo is the first
// sample that is not (before tau and past the cut), hi the first from lo on that is (behind tau and past the cut).  Any
// input - times out of order, a NaN - gives 0 <= lo <= hi <= n.
__global__ __launch_bounds__(kBlock) void wwz_bounds_kernel(WwzArgs a) {
    const int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= a.ntau * a.tiles) return;
    const int64_t row = cell / a.tiles, tile = cell % a.tiles;
    const double tau = a.tau[row];
    const double f_lo = grid_frequency(a.f0, a.delta, tile * kTile);
    const double scale = a.cdecay * (f_lo * f_lo);
    const auto past_cut = [&](const double d) { return scale * (d * d) > kCutExponent; };
    int64_t lo = 0, len = a.n;
    while (len > 0) {   // first i with !(t[i] < tau && past_cut)
        const int64_t half = len >> 1;
        const double ti = a.t[lo + half];
        if (ti < tau && past_cut(ti - tau)) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    int64_t hi = lo;
    len = a.n - lo;
    while (len > 0) {   // first i >= lo with t[i] > tau && past_cut
        const int64_t half = len >> 1;
        const double ti = a.t[hi + half];
        if (ti > tau && past_cut(ti - tau)) {
            len = half;
        } else {
            hi += half + 1;
            len -= half + 1;
        }
    }
    a.part[cell].lo = lo;
    a.part[cell].hi = hi;
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
// One bin from its ten sums.  Everything is divided by W first, so S[0][0] = 1 and the first Cholesky column is the
// first column of S; with z the forward substitution of b, z[0] = <1, y> and Vy = a^T b - <1, y>^2 = z[1]^2 + z[2]^2,
// taken in that form (no cancellation).
struct WwzCell {
    double wwz, amp, neff;
};
__device__ __forceinline__ WwzCell wwz_cell(double W, double W2, double C, double S, double CC, double CS, double Y,
                                            double YC, double YS, double YY) {
    WwzCell out;
    if (!(W > 0.0)) {
        out.wwz = out.amp = quiet_nan();
        out.neff = 0.0;
        return out;
    }
    out.neff = W * W / W2;
    const double inv = 1.0 / W;
    const double c1 = C * inv, s1 = S * inv, cc = CC * inv, cs = CS * inv, ss = (W - CC) * inv;
    const double y1 = Y * inv, yc = YC * inv, ys = YS * inv, yy = YY * inv;
    const double d1 = cc - c1 * c1;
    const double l11 = __builtin_sqrt(d1);
    const double l21 = (cs - s1 * c1) / l11;
    const double d2 = (ss - s1 * s1) - l21 * l21;
    const double l22 = __builtin_sqrt(d2);
    const bool bad = !(d1 > 0.0) || !(d1 < HUGE_VAL) || !(d2 > 0.0) || !(d2 < HUGE_VAL);
    const double z1 = (yc - c1 * y1) / l11;
    const double z2 = ((ys - s1 * y1) - l21 * z1) / l22;
    const double a3 = z2 / l22;
    const double a2 = (z1 - l21 * a3) / l11;
    const double vy = z1 * z1 + z2 * z2;
    const double vx = yy - y1 * y1;
    out.wwz = bad ? quiet_nan() : (out.neff - 3.0) * vy / (2.0 * (vx - vy));
    out.amp = bad ? quiet_nan() : __builtin_sqrt(a2 * a2 + a3 * a3);
    return out;
}

template <int K>
__global__ __launch_bounds__(kBlock) void wwz_scan_kernel(WwzArgs a) {
    constexpr int COLS = kBlock / 64;   // 64-lane columns of the tile
    __shared__ double2 tab[kChunk + 1][COLS * 8 + 8 + 1];   // as mhgls_scan_kernel
    __shared__ double2 win[kChunk];                         // per sample of the chunk: {A, q = exp(-2 A delta^2)}
    __shared__ double red_v[COLS];
    __shared__ long long red_i[COLS];
    __shared__ long long best_bin;
    // What the fills need of the row and the tile waits in LDS (the first read is behind the stretch's first barrier):
    // in scalar registers across the hot loop these values, with the epilogue's arguments, are more than a wave has.
    __shared__ double fill_const[5];   // tau - t[0], c (2 pi)^2, 2 delta^2, K delta, f_tile

    const int64_t tile = blockIdx.x;
    const int64_t row = a.row0 + blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int col = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t jt = tile * (int64_t)(kBlock * K);
    const int64_t jl = jt + (int64_t)tid * K;
    WwzPart *part = a.part + (row * a.tiles + tile);
    if (tid == 0) {
        fill_const[0] = a.tau[row] - a.t[0];   // the window takes t - tau as t' - (tau - t[0]), t' from the record
        fill_const[1] = a.cdecay;
        fill_const[2] = 2.0 * (a.delta * a.delta);
        fill_const[3] = (double)K * a.delta;   // spacing of the threads' first frequencies (exact)
        fill_const[4] = grid_frequency(a.f0, a.delta, jt);
    }
    const double f_first = grid_frequency(a.f0, a.delta, jl);   // this thread's first frequency
    const double f_sq = f_first * f_first;                          // g[0] = exp(-A f_sq)
    const double f_lin = a.delta * (2.0 * f_first + a.delta);       // r[0] = exp(-A f_lin)
    const int64_t lo = part->lo, hi = part->hi;

    double W[K], W2[K], C[K], S[K], CC[K], CS[K], Y[K], YC[K], YS[K], YY[K];
#pragma unroll
    for (int k = 0; k < K; ++k) W[k] = W2[k] = C[k] = S[k] = CC[k] = CS[k] = Y[k] = YC[k] = YS[k] = YY[k] = 0.0;

    // scan_stretch accumulates the samples of a chunk in order, one call of the walk per sample: `seen` counts them, so
    // seen % kChunk is the sample's place in the chunk and in `win`.
    int seen = 0;
    double g = 0.0, r = 0.0, q = 0.0;
    const int slot_a = col * 8 + (lane >> 3), slot_b = COLS * 8 + (lane & 7);
    scan_stretch<kChunk, K>(
        tab, a.rec, a.n, lo, hi, tid, slot_a, slot_b,
        [&](double2 *trow, const int64_t i, const bool real) {   // (sin, cos) unscaled; the even thread: the window
            const double tp = real ? a.rec[i * 6 + 5] : 0.0;
            fill_rotation_tables<COLS>(trow, tid & 1, tp, fill_const[3], fill_const[4], 1.0);
            if (!(tid & 1)) {
                const double d = real ? tp - fill_const[0] : 0.0;
                const double A = fill_const[1] * (d * d);
                win[(i - lo) % kChunk] = make_double2(A, exp_neg(A * fill_const[2]));
            }
        },
        [&](const Ahead &h, const int k, const double s, const double c) {
            if (k == 0) {
                const double2 wn = win[seen % kChunk];
                ++seen;
                g = exp_neg(wn.x * f_sq);
                r = exp_neg(wn.x * f_lin);
                q = wn.y;
            }
            const double wg = h.r[1] * g;
            const double wy = wg * h.r[0];
            const double wc = wg * c, ws = wg * s;
            W[k] += wg;
            W2[k] = __builtin_fma(wg, wg, W2[k]);
            C[k] += wc;
            S[k] += ws;
            CC[k] = __builtin_fma(wc, c, CC[k]);
            CS[k] = __builtin_fma(wc, s, CS[k]);
            Y[k] += wy;
            YC[k] = __builtin_fma(wy, c, YC[k]);
            YS[k] = __builtin_fma(wy, s, YS[k]);
            YY[k] = __builtin_fma(wy, h.r[0], YY[k]);
            if (k + 1 < K) {
                g *= r;
                r *= q;
            }
        });

    // Epilogue.  A thread's bins ascend, so do the threads': ArgMax keeps the lowest bin of equal maxima.
    ArgMax am;
    double am_amp = 0.0;
    const int64_t at = row * a.nf;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t j = jl + k;
        if (j < a.nf) {
            const WwzCell cell = wwz_cell(W[k], W2[k], C[k], S[k], CC[k], CS[k], Y[k], YC[k], YS[k], YY[k]);
            if (a.wwz) a.wwz[at + j] = cell.wwz;
            if (a.amp) a.amp[at + j] = cell.amp;
            if (a.neff) a.neff[at + j] = cell.neff;
            if (cell.neff >= a.min_neff) {
                const long long before = am.j;
                am.take(cell.wwz, j);
                if (am.j != before) am_amp = cell.amp;
            }
        }
    }
    const long long own_j = am.j;   // (the fold below overwrites am)
    const bool first = am.block_fold<COLS>(red_v, red_i, lane, col);
    if (first) {
        best_bin = am.j;
        part->v = am.j < 0 ? quiet_nan() : am.v;
        part->j = am.j;
        if (am.j < 0) part->amp = quiet_nan();
    }
    __syncthreads();
    if (own_j >= 0 && own_j == best_bin) part->amp = am_amp;   // the one thread whose bin won
}

// ---- ridge, best cell, visited -----------------------------------------------------------------------------------------
// The tiles of one row in ascending order (ascending bins): value NaN, bin -1 where no tile has an eligible bin.
__device__ __forceinline__ void fold_row(const WwzArgs &a, int64_t row, ArgMax &rm, double &amp) {
    amp = quiet_nan();
    for (int64_t tile = 0; tile < a.tiles; ++tile) {
        const WwzPart &part = a.part[row * a.tiles + tile];
        const long long before = rm.j;
        rm.take_later(part.v, part.j);
        if (rm.j != before) amp = part.amp;
    }
}

// One workgroup.  Wave w takes the w-th run of rows, its lanes interleaved: a lane sees ascending rows, wave_fold
// compares the rows of equal maxima, the waves fold in order.
__global__ __launch_bounds__(kPrepBlock) void wwz_fold_kernel(WwzArgs a) {
    constexpr int WAVES = kPrepBlock / 64;
    __shared__ double red_v[WAVES];
    __shared__ long long red_i[WAVES];
    __shared__ long long red_n[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t run = (a.ntau + WAVES - 1) / WAVES;
    const int64_t beg = wave * run, end = beg + run < a.ntau ? beg + run : a.ntau;
    ArgMax best;
    long long visited = 0;
    for (int64_t row = beg + lane; row < end; row += 64) {
        ArgMax rm;
        double amp;
        fold_row(a, row, rm, amp);
        a.ridge_bin[row] = rm.j;
        a.ridge_wwz[row] = rm.j < 0 ? quiet_nan() : rm.v;
        a.ridge_amp[row] = amp;
        if (rm.j >= 0) best.take(rm.v, row);
        for (int64_t tile = 0; tile < a.tiles; ++tile) {
            const WwzPart &part = a.part[row * a.tiles + tile];
            visited += part.hi - part.lo;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) visited += __shfl_down(visited, o, 64);
    if (lane == 0) red_n[wave] = visited;
    if (!best.block_fold<WAVES>(red_v, red_i, lane, wave)) return;   // (its barrier covers red_n)
    if (a.visited) {
        long long total = 0;
        for (int wv = 0; wv < WAVES; ++wv) total += red_n[wv];
        a.visited[0] = total;
    }
    if (a.best) a.best[0] = best.j < 0 ? quiet_nan() : best.v;
    if (a.best_at) {
        ArgMax rm;   // the winning row's bin: its tiles once more, the same order
        double amp;
        if (best.j >= 0) fold_row(a, best.j, rm, amp);
        a.best_at[0] = best.j;
        a.best_at[1] = rm.j;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct WwzDispatch {
    int k, rows;
    int64_t launches;
};
thread_local WwzDispatch g_last = {};

// records | one WwzPart per (tau, tile) | ridge (value, amplitude, bin) for a caller that takes none
struct WwzPlan {
    int64_t tiles, at_part, at_ridge_wwz, at_ridge_amp, at_ridge_bin, total;
};

WwzPlan wwz_plan(int64_t n, int64_t nf, int64_t ntau) {
    WwzPlan p;
    p.tiles = (nf + kTile - 1) / kTile;
    const int64_t cells = p.tiles * ntau;
    Carve c;
    c.take((n + 2) * 48);
    p.at_part = c.take(cells * (int64_t)sizeof(WwzPart));
    p.at_ridge_wwz = c.take(ntau * 8);
    p.at_ridge_amp = c.take(ntau * 8);
    p.at_ridge_bin = c.take(ntau * 8);
    p.total = c.at;
    return p;
}

bool wwz_sizes_ok(int64_t n, int64_t nf, int64_t ntau) {
    if (n < 4 || nf < 1 || ntau < 1 || n > ((int64_t)1 << 50)) return false;
    const int64_t tiles = (nf + kTile - 1) / kTile;
    return tiles < ((int64_t)1 << 31) - 8 && ntau <= (((int64_t)1 << 56) / tiles) && ntau <= (((int64_t)1 << 59) / nf);
}

int wwz_validate(int64_t n, double f0, double delta, int64_t nf, int64_t ntau, double decay, double min_neff,
                 bool any_output) {
    PDC_REQUIRE(std::isfinite(f0) && f0 >= 0.0, "wwz: the first frequency must be finite and not negative");
    PDC_REQUIRE(std::isfinite(delta) && delta > 0.0, "wwz: the grid step must be finite and positive");
    PDC_REQUIRE(nf >= 1, "wwz: at least one frequency is needed (got %lld)", (long long)nf);
    PDC_REQUIRE(n >= 4, "wwz: three parameters are fitted, at least 4 samples are needed (got %lld)", (long long)n);
    PDC_REQUIRE(ntau >= 1, "wwz: at least one time shift is needed (got %lld)", (long long)ntau);
    PDC_REQUIRE(std::isfinite(decay) && decay > 0.0, "wwz: the decay constant must be finite and positive");
    PDC_REQUIRE(std::isfinite(min_neff), "wwz: min_neff must be finite");
    PDC_REQUIRE(wwz_sizes_ok(n, nf, ntau), "wwz: plane too large");
    PDC_REQUIRE(any_output, "wwz: every output is NULL");
    return PDC_OK;
}

// `work`: wwz_plan(...).total bytes.  Outputs are device pointers, any of them NULL.
int wwz_enqueue(hipStream_t st, const double *d_t, const double *d_y, const double *d_dy, int64_t n, double f0,
                double delta, int64_t nf, const double *d_tau, int64_t ntau, double decay, double min_neff,
                const WwzPlan &plan, double *d_wwz, double *d_amp, double *d_neff, int64_t *d_ridge_bin,
                double *d_ridge_wwz, double *d_ridge_amp, double *d_best, int64_t *d_best_at, int64_t *d_visited,
                void *work) {
    char *base = static_cast<char *>(work);
    WwzPrepArgs p;
    p.t = d_t;
    p.y = d_y;
    p.dy = d_dy;
    p.n = n;
    p.delta = delta;
    p.rec = reinterpret_cast<double *>(base);
    hipLaunchKernelGGL(wwz_prep_kernel, dim3(1), dim3(kPrepBlock), 0, st, p);
    PDC_HIP(hipGetLastError());
    WwzArgs a;
    a.rec = p.rec;
    a.t = d_t;
    a.tau = d_tau;
    a.n = n;
    a.tiles = plan.tiles;
    a.ntau = ntau;
    a.nf = nf;
    a.f0 = f0;
    a.delta = delta;
    a.cdecay = decay * (4.0 * M_PI * M_PI);
    a.min_neff = min_neff;
    a.row0 = 0;
    a.part = reinterpret_cast<WwzPart *>(base + plan.at_part);
    a.wwz = d_wwz;
    a.amp = d_amp;
    a.neff = d_neff;
    a.ridge_wwz = d_ridge_wwz ? d_ridge_wwz : reinterpret_cast<double *>(base + plan.at_ridge_wwz);
    a.ridge_amp = d_ridge_amp ? d_ridge_amp : reinterpret_cast<double *>(base + plan.at_ridge_amp);
    a.ridge_bin = d_ridge_bin ? d_ridge_bin : reinterpret_cast<int64_t *>(base + plan.at_ridge_bin);
    a.best = d_best;
    a.best_at = d_best_at;
    a.visited = d_visited;
    const int64_t cells = plan.tiles * ntau;
    hipLaunchKernelGGL(wwz_bounds_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
    PDC_HIP(hipGetLastError());
    const int64_t rows = ntau < kMaxRows ? ntau : kMaxRows;
    g_last = {kFreqs, (int)rows, (ntau + rows - 1) / rows};
    for (int64_t row0 = 0; row0 < ntau; row0 += rows) {
        a.row0 = row0;
        const int64_t here = ntau - row0 < rows ? ntau - row0 : rows;
        hipLaunchKernelGGL((wwz_scan_kernel<kFreqs>), dim3((unsigned)plan.tiles, (unsigned)here), dim3(kBlock), 0, st, a);
        PDC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(wwz_fold_kernel, dim3(1), dim3(kPrepBlock), 0, st, a);
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

}  // namespace

extern "C" {

int64_t pdc_wwz_tile_bins(void) { return kTile; }

int64_t pdc_wwz_work_bytes(int64_t n, int64_t nf, int64_t ntau) {
    if (!wwz_sizes_ok(n, nf, ntau)) return -1;
    return wwz_plan(n, nf, ntau).total;
}

int pdc_wwz_last_dispatch(int *k, int *rows_per_launch, int64_t *launches) {
    if (k) *k = g_last.k;
    if (rows_per_launch) *rows_per_launch = g_last.rows;
    if (launches) *launches = g_last.launches;
    return PDC_OK;
}

int pdc_wwz_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                     double f0, double delta, int64_t nf, const double *d_tau, int64_t ntau, double decay,
                     double min_neff, double *d_wwz, double *d_amp, double *d_neff, int64_t *d_ridge_bin,
                     double *d_ridge_wwz, double *d_ridge_amp, double *d_best, int64_t *d_best_at, int64_t *d_visited) {
    PDC_TRY(wwz_validate(n, f0, delta, nf, ntau, decay, min_neff,
                         d_wwz || d_amp || d_neff || d_ridge_bin || d_ridge_wwz || d_ridge_amp || d_best || d_best_at ||
                             d_visited));
    PDC_REQUIRE(d_t && d_y && d_tau, "wwz: NULL argument");
    PDC_TRY(use_device(device));
    const WwzPlan plan = wwz_plan(n, nf, ntau);
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, plan.total, &work));
    return wwz_enqueue(st, d_t, d_y, d_dy, n, f0, delta, nf, d_tau, ntau, decay, min_neff, plan, d_wwz, d_amp, d_neff,
                       d_ridge_bin, d_ridge_wwz, d_ridge_amp, d_best, d_best_at, d_visited, work);
}

int pdc_wwz_scan(const double *t, const double *y, const double *dy, int64_t n, double f0, double delta, int64_t nf,
                 const double *tau, int64_t ntau, double decay, double min_neff, double *wwz_out, double *amp_out,
                 double *neff_out, int64_t *ridge_bin_out, double *ridge_wwz_out, double *ridge_amp_out, double *best_out,
                 int64_t *best_at_out, int64_t *visited_out, int device) {
    PDC_TRY(wwz_validate(n, f0, delta, nf, ntau, decay, min_neff,
                         wwz_out || amp_out || neff_out || ridge_bin_out || ridge_wwz_out || ridge_amp_out || best_out ||
                             best_at_out || visited_out));
    PDC_REQUIRE(t && y && tau, "wwz: NULL argument");
    for (int64_t i = 0; i < n; ++i) {
        PDC_REQUIRE(std::isfinite(t[i]), "wwz: t[%lld] is not finite", (long long)i);
        PDC_REQUIRE(i == 0 || t[i] >= t[i - 1], "wwz: the times must not decrease (t[%lld] < t[%lld])", (long long)i,
                    (long long)(i - 1));
    }
    for (int64_t r = 0; r < ntau; ++r)
        PDC_REQUIRE(std::isfinite(tau[r]), "wwz: tau[%lld] is not finite", (long long)r);
    HostCall hc(device);
    PDC_TRY(hc.status);
    const WwzPlan plan = wwz_plan(n, nf, ntau);
    double *d_t = hc.in(SLOT_IN0, t, n * 8), *d_y = hc.in(SLOT_IN1, y, n * 8), *d_dy = hc.in(SLOT_IN2, dy, n * 8);
    double *d_tau = hc.in(SLOT_IN3, tau, ntau * 8);
    // the planes share one block, the small outputs another: ridge bin | wwz | amplitude | best | best_at | visited
    const int64_t plane = ntau * nf * 8;
    Carve cp;
    const int64_t at_wwz = cp.take(wwz_out ? plane : 0), at_amp = cp.take(amp_out ? plane : 0),
                  at_neff = cp.take(neff_out ? plane : 0);
    char *d_planes = cp.at > 0 ? hc.out<char>(SLOT_OUT0, cp.at) : nullptr;
    Carve c;
    const int64_t at_bin = c.take(ntau * 8), at_rw = c.take(ntau * 8), at_ra = c.take(ntau * 8), at_best = c.take(8),
                  at_best_at = c.take(16), at_visited = c.take(8);
    char *d_small = hc.out<char>(SLOT_OUT1, c.at);
    void *d_work = hc.reserve(SLOT_WORK, plan.total);
    PDC_TRY(hc.status);
    double *d_wwz = wwz_out ? reinterpret_cast<double *>(d_planes + at_wwz) : nullptr;
    double *d_amp = amp_out ? reinterpret_cast<double *>(d_planes + at_amp) : nullptr;
    double *d_neff = neff_out ? reinterpret_cast<double *>(d_planes + at_neff) : nullptr;
    int64_t *d_bin = ridge_bin_out ? reinterpret_cast<int64_t *>(d_small + at_bin) : nullptr;
    double *d_rw = ridge_wwz_out ? reinterpret_cast<double *>(d_small + at_rw) : nullptr;
    double *d_ra = ridge_amp_out ? reinterpret_cast<double *>(d_small + at_ra) : nullptr;
    double *d_best = best_out ? reinterpret_cast<double *>(d_small + at_best) : nullptr;
    int64_t *d_best_at = best_at_out ? reinterpret_cast<int64_t *>(d_small + at_best_at) : nullptr;
    int64_t *d_visited = visited_out ? reinterpret_cast<int64_t *>(d_small + at_visited) : nullptr;
    PDC_TRY(wwz_enqueue(hc.stream(), d_t, d_y, d_dy, n, f0, delta, nf, d_tau, ntau, decay, min_neff, plan, d_wwz, d_amp,
                        d_neff, d_bin, d_rw, d_ra, d_best, d_best_at, d_visited, d_work));
    hc.back(wwz_out, d_wwz, plane);
    hc.back(amp_out, d_amp, plane);
    hc.back(neff_out, d_neff, plane);
    hc.back(ridge_bin_out, d_bin, ntau * 8);
    hc.back(ridge_wwz_out, d_rw, ntau * 8);
    hc.back(ridge_amp_out, d_ra, ntau * 8);
    hc.back(best_out, d_best, 8);
    hc.back(best_at_out, d_best_at, 16);
    hc.back(visited_out, d_visited, 8);
    return hc.finish();
}

}  // extern "C"
