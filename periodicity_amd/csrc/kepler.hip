// The Keplerian periodogram (Zechmeister & Kurster 2009, A&A 496, 577, section 4) as an exact direct summation on
// gfx950: per trial frequency the best weighted least-squares fit of a Keplerian orbit over a grid of eccentricities
// and periastron phases.  The fit is linear in (cos nu, sin nu, 1), nu the true anomaly, so a cell (frequency, e, m0)
// costs one Kepler solve per sample and six running sums; power = b^T M^-1 b / YY as in mhgls.hip.
//
// The reference (its spectral.py) has no such class: PARITY UNPINNED BY THE REFERENCE.
// The weights, the centring, the grid rule and the two normalisations are those of GLS (spectral.py:99-108, 129-132).
//
// Decomposition
//   kepler_prep_kernel   one workgroup: weights, weighted mean, YY, sum w y, one 32-byte record {w, w y_c, t', 0} per
//                        sample, and one 32-byte record per cell {e, m0 reduced to [-1/2, 1/2], the starter's slope
//                        constant, sqrt(1 - e^2)}; a cell whose e or m0 is out of range gets e = NaN (every value NaN).
//   kepler_scan_kernel   a workgroup owns a tile of 256 frequencies and one group of KC cells, a thread one frequency
//                        and its KC cells: 6 KC running sums (12 KC VGPRs).  The sample records come through the scalar
//                        cache one ahead; the phase frac(f t') of a (sample, frequency) is the exact product reduced
//                        in cycles (frac_product, no seed and no recurrence: five of the ~124 KC instructions of a
//                        sample) and is shared by the thread's cells.  Per cell one call of true_anomaly and six fmas.
//                        Epilogue: cholesky_quadratic per cell, the group's (max, lowest argmax) to a workspace row,
//                        the cells to the cube where it is wanted.
//   kepler_fold_kernel   a thread per bin: the groups' rows in ascending cell order (np.nanmax / np.nanargmax), and
//                        the best bin of each tile to the workspace.
//   kepler_best_kernel   one workgroup: the tiles' best bins in ascending order, carried from slab to slab.  (One
//                        workgroup doing both took 2.0 of 12.6 ms at 200 samples x 1e4 bins x 1280 cells.)
//   kepler_anomaly_kernel  true_anomaly on a list of (phase, e) pairs: what pdc_kepler_anomaly runs.
// No atomics, every sum in one fixed order: the same bits from call to call, and a cell's bits depend on its
// (e, m0) and the curve alone - not on its place in the lists, its group or the slab of its bin.
#include "pdc_internal.h"
#include "harmonic_sums.h"

#include <cmath>

using namespace pdc;

namespace {

constexpr int kBlock = 256;        // frequencies per tile, one per thread
constexpr int kPrepBlock = 1024;
constexpr int kCells = 4;          // KC: cells per thread
constexpr int kMaxCells = 65535;   // ne * nm (the groups are the grid's second dimension)
constexpr double kMaxEcc = 0.95;

__device__ __forceinline__ double quiet_nan() { return __builtin_nan(""); }

// numpy's arange fill rule: start + j * delta, two roundings (no fma)
__device__ __forceinline__ double grid_frequency(double f0, double delta, int64_t j) {
    return __dadd_rn(f0, __dmul_rn((double)j, delta));
}

// ---- the Kepler solve -----------------------------------------------------------------------------------------------
struct KepCell {
    double e, m0, a1, root;   // m0 in [-1/2, 1/2] cycles; a1 = 1.6 pi / ((pi^2 - 6)(1 + e)); root = sqrt((1 - e)(1 + e))
};

__device__ __forceinline__ KepCell make_cell(double e, double m0) {
    KepCell c;
    const bool ok = e >= 0.0 && e <= kMaxEcc && m0 >= 0.0 && m0 < 1.0;
    c.e = ok ? e : quiet_nan();
    c.m0 = m0 - __builtin_rint(m0);   // exact
    c.a1 = (1.6 * M_PI / (M_PI * M_PI - 6.0)) / (1.0 + e);
    c.root = __builtin_sqrt((1.0 - e) * (1.0 + e));
    return c;
}

// 1 / x from the hardware estimate (about 24 bits) and STEPS Newton steps: 0 for a value that only steers the next
// approximation, 1 (48 bits) for a correction term, 2 for a result.  No scaling of denormals: x is of order one here.
template <int STEPS>
__device__ __forceinline__ double reciprocal(double x) {
    double r = __builtin_amdgcn_rcp(x);
#pragma unroll
    for (int s = 0; s < STEPS; ++s) r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return r;
}

// cos and sin of the true anomaly at mean anomaly m CYCLES (any value of a few cycles) of an orbit of eccentricity e in
// [0, 0.95].  Fixed trip count, no table, no branch (Markley 1995, Celest. Mech. Dyn. Astron. 63, 101): the anomaly is
// folded to M in [0, pi]; the starter E1 is the root of the cubic that the Pade approximant of sin makes of Kepler's
// equation, within 4e-4 rad of E (its cube root and square root are taken in fp32, its quotient by the bare hardware
// estimate: an error of 3e-6 there moves E1 by as much, measured); one fifth-order correction d5 leaves less than
// 1e-15 rad.  sin E, cos E are sincos(E1) turned by d5 (|d5| <= 4e-4: the series to d5^4), so one sincos per solve.
//     cos nu = 1 - (1 + e)(1 - cos E) / (1 - e cos E),   sin nu = sqrt(1 - e^2) sin E / (1 - e cos E)
// - the first in this form because it is exactly 1 at E = 0 whatever the quotient rounds to; the sign of m goes to sin nu.
__device__ __forceinline__ void true_anomaly(double m, const double e, const double a1, const double root, double &cn,
                                             double &sn) {
    constexpr double kA0 = 3.0 * M_PI * M_PI / (M_PI * M_PI - 6.0);
    m -= __builtin_rint(m);   // exact: [-1/2, 1/2] cycles
    const double Ma = __builtin_fabs(m) * (2.0 * M_PI);
    const double ome = 1.0 - e;
    // starter
    const double alpha = __builtin_fma(a1, M_PI - Ma, kA0);
    const double d = __builtin_fma(alpha, e, 3.0 * ome);
    const double ad = alpha * d;
    const double M2 = Ma * Ma;
    const double q = __builtin_fma(2.0 * ad, ome, -M2);
    const double r = __builtin_fma(3.0 * ad, d - ome, M2) * Ma;
    const double q2 = q * q;
    const double disc = __builtin_fmax(__builtin_fma(q2, q, r * r), 0.0);
    const float x = (float)r + __builtin_amdgcn_sqrtf((float)disc);
    const double w = (double)__builtin_amdgcn_exp2f(__builtin_amdgcn_logf(x) * (2.0f / 3.0f));   // x^(2/3)
    const double den = __builtin_fma(w + q, w, q2);
    const double E1 = __builtin_fma(2.0 * r, w, Ma * den) * reciprocal<0>(d * den);
    double s, c;
    sincos_cycles_half(E1 * (0.5 / M_PI), s, c);   // (E1 is at most half a cycle: no quadrant logic)
    // fifth-order correction
    const double f2 = e * s, f3 = e * c;
    const double f0 = (E1 - f2) - Ma;
    const double f1 = 1.0 - f3;
    const double h2 = 0.5 * f2, h3 = f3 * (1.0 / 6.0), h4 = f2 * (-1.0 / 24.0);
    const double d3 = -f0 * reciprocal<0>(__builtin_fma(-f0 * h2, reciprocal<0>(f1), f1));
    const double d4 = -f0 * reciprocal<0>(__builtin_fma(d3, __builtin_fma(d3, h3, h2), f1));
    const double d5 =
        -f0 * reciprocal<1>(__builtin_fma(d4, __builtin_fma(d4, __builtin_fma(d4, h4, h3), h2), f1));
    // (sin, cos)(E1 + d5)
    const double dd = d5 * d5;
    const double sd = __builtin_fma(d5 * dd, -1.0 / 6.0, d5);
    const double cd = __builtin_fma(dd, __builtin_fma(dd, 1.0 / 24.0, -0.5), 1.0);
    const double sE = __builtin_fma(s, cd, c * sd);
    const double cE = __builtin_fma(c, cd, -(s * sd));
    const double inv = reciprocal<2>(__builtin_fma(-e, cE, 1.0));
    cn = __builtin_fma(-(1.0 + e) * (1.0 - cE), inv, 1.0);
    const double sa = root * sE * inv;
    sn = m < 0.0 ? -sa : sa;
}

// ---- prologue: weights, centring and YY as GLS takes them (spectral.py:99-108, 120) ---------------------------------
struct KepPrepArgs {
    const double *t, *y, *dy, *ecc, *m0;
    int64_t n;
    int ne, nm, cells_padded, fit_mean;
    double *rec;      // [n + 1][4] (the scan reads one record ahead)
    KepCell *cells;   // [cells_padded]: the last real cell repeated behind the real ones
    double *scal;     // {YY, sum w, sum err^-2, sum w y}
};

__global__ __launch_bounds__(kPrepBlock) void kepler_prep_kernel(KepPrepArgs a) {
    __shared__ double red[kPrepBlock / 64];
    const int tid = threadIdx.x;
    const double t0 = a.t[0];
    double W, ybar;
    weights_and_mean<kPrepBlock>(a.y, a.dy, a.n, a.fit_mean, red, W, ybar);
    double yy = 0.0, wsum = 0.0, y1 = 0.0;
    double4 *rec = reinterpret_cast<double4 *>(a.rec);
    for (int64_t i = tid; i < a.n; i += kPrepBlock) {
        const double w = inv_var(a.dy, i) / W;
        const double yc = a.y[i] - ybar;
        const double wy = w * yc;
        yy += wy * yc;
        wsum += w;
        y1 += wy;
        rec[i] = make_double4(w, wy, a.t[i] - t0, 0.0);
    }
    if (tid == 0) rec[a.n] = make_double4(0.0, 0.0, 0.0, 0.0);   // read ahead, never accumulated
    const int cells = a.ne * a.nm;
    for (int c = tid; c < a.cells_padded; c += kPrepBlock) {
        const int cell = c < cells ? c : cells - 1;
        a.cells[c] = make_cell(a.ecc[cell / a.nm], a.m0[cell % a.nm]);
    }
    yy = block_sum<kPrepBlock>(yy, red);
    wsum = block_sum<kPrepBlock>(wsum, red);
    y1 = block_sum<kPrepBlock>(y1, red);
    if (tid == 0) {
        a.scal[0] = yy;
        a.scal[1] = wsum;
        a.scal[2] = W;
        a.scal[3] = y1;
    }
}

// ---- the scan -------------------------------------------------------------------------------------------------------
struct KepBest {   // the best bin so far, carried from slab to slab
    double v;
    long long bin, cell;
};

struct KepArgs {
    const double *rec, *scal;
    const KepCell *cells;
    int64_t n, nf;
    double f0, delta;
    int cell_count, groups, fit_mean, psd;
    int64_t bin0, slab_bins;   // the slab of this launch: bins [bin0, bin0 + slab_bins), a multiple of the tile but the last
    double *row_v;             // [groups][slab_pitch]: a group's largest cell of a bin, NaN where it has none
    int32_t *row_c;            //                      ... and its index, -1
    int64_t slab_pitch;
    double *cube, *power;      // caller's, any may be NULL
    int32_t *cell;
    KepBest *part, *carry;     // [slab tiles]: a tile's best bin; the best bin of the slabs so far
    double *best;
    int64_t *best_at;
    int first, last;           // slab
};

// KC cells per thread: 6 KC accumulators.  Basis order (cos nu, sin nu, 1): the constant comes LAST, as in mhgls.hip,
// so the fit without a floating mean is the same factorisation stopped one column early.
template <int KC>
__global__ __launch_bounds__(kBlock) void kepler_scan_kernel(KepArgs a) {
    const int tid = threadIdx.x;
    const int group = blockIdx.y;
    const int64_t jl = (int64_t)blockIdx.x * kBlock + tid;   // bin of this thread within the slab
    const int64_t j = a.bin0 + jl;
    const double f = grid_frequency(a.f0, a.delta, j);       // (finite past the grid too: computed, never stored)
    using ccell = __attribute__((address_space(4))) const KepCell;
    const ccell *cell = reinterpret_cast<const ccell *>(reinterpret_cast<uintptr_t>(a.cells)) + group * KC;
    const cd4 *rec = reinterpret_cast<const cd4 *>(reinterpret_cast<uintptr_t>(a.rec));

    double C[KC], S[KC], CC[KC], CS[KC], YC[KC], YS[KC];
#pragma unroll
    for (int q = 0; q < KC; ++q) C[q] = S[q] = CC[q] = CS[q] = YC[q] = YS[q] = 0.0;

    d4 cur = rec[0];
    for (int64_t i = 0; i < a.n; ++i) {
        const d4 next = rec[i + 1];
        const double w = cur[0], wy = cur[1];
        const double phi = frac_product(f, cur[2]);
#pragma unroll
        for (int q = 0; q < KC; ++q) {
            double cn, sn;
            true_anomaly(phi - cell[q].m0, cell[q].e, cell[q].a1, cell[q].root, cn, sn);
            const double wc = w * cn;
            C[q] = __builtin_fma(w, cn, C[q]);
            S[q] = __builtin_fma(w, sn, S[q]);
            CC[q] = __builtin_fma(wc, cn, CC[q]);
            CS[q] = __builtin_fma(wc, sn, CS[q]);
            YC[q] = __builtin_fma(wy, cn, YC[q]);
            YS[q] = __builtin_fma(wy, sn, YS[q]);
        }
        cur = next;
    }

    const double YY = a.scal[0], Wsum = a.scal[1], Werr = a.scal[2], Y1 = a.scal[3];
    ArgMax am;   // the cells ascend: the lowest of equal maxima stays
#pragma unroll
    for (int q = 0; q < KC; ++q) {
        const int c = group * KC + q;
        if (c < a.cell_count) {
            const double b[3] = {YC[q], YS[q], Y1};
            const double quad = cholesky_quadratic<3>(
                [&](const int r, const int col) {   // sum w sin^2 = sum w - sum w cos^2
                    if (r == 0) return CC[q];
                    if (r == 1) return col == 0 ? CS[q] : Wsum - CC[q];
                    return col == 0 ? C[q] : (col == 1 ? S[q] : Wsum);
                },
                b, a.fit_mean ? 3 : 2);
            const double p = normalised_power(quad, a.psd, Werr, YY);
            if (a.cube && j < a.nf) a.cube[j * a.cell_count + c] = p;
            am.take(p, c);
        }
    }
    if (j < a.nf) {
        a.row_v[group * a.slab_pitch + jl] = am.j < 0 ? quiet_nan() : am.v;
        a.row_c[group * a.slab_pitch + jl] = (int32_t)am.j;
    }
}

// ---- per bin the best cell, per tile and over all bins the best bin --------------------------------------------------
// The groups of one bin in ascending order (ascending cells).
__device__ __forceinline__ ArgMax fold_bin(const KepArgs &a, int64_t jl) {
    ArgMax bm;
    for (int g = 0; g < a.groups; ++g) bm.take_later(a.row_v[g * a.slab_pitch + jl], a.row_c[g * a.slab_pitch + jl]);
    return bm;
}

// A workgroup per tile of the slab, a thread per bin: power and cell of the bin, and the tile's best bin (the lowest of
// equal maxima: threads, lanes and waves hold ascending bins) to the workspace.
__global__ __launch_bounds__(kBlock) void kepler_fold_kernel(KepArgs a) {
    constexpr int WAVES = kBlock / 64;
    __shared__ double red_v[WAVES];
    __shared__ long long red_i[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t jl = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    ArgMax best;
    if (jl < a.slab_bins) {
        const ArgMax bm = fold_bin(a, jl);
        const double v = bm.j < 0 ? quiet_nan() : bm.v;
        if (a.power) a.power[a.bin0 + jl] = v;
        if (a.cell) a.cell[a.bin0 + jl] = (int32_t)bm.j;
        if (bm.j >= 0) best.take(v, a.bin0 + jl);
    }
    if (!best.block_fold<WAVES>(red_v, red_i, lane, wave)) return;
    KepBest part = {0.0, best.j, -1};
    if (best.j >= 0) {
        part.v = best.v;
        part.cell = fold_bin(a, best.j - a.bin0).j;
    }
    a.part[blockIdx.x] = part;
}

// One workgroup: the tiles' best bins in ascending order, and the slabs before this one.  Wave w takes the w-th run of
// tiles, its lanes interleaved; wave_fold compares the bins of equal maxima, the waves fold in order.
__global__ __launch_bounds__(kPrepBlock) void kepler_best_kernel(KepArgs a) {
    constexpr int WAVES = kPrepBlock / 64;
    __shared__ double red_v[WAVES];
    __shared__ long long red_i[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tiles = (a.slab_bins + kBlock - 1) / kBlock;
    const int64_t run = (tiles + WAVES - 1) / WAVES;
    const int64_t beg = wave * run, end = beg + run < tiles ? beg + run : tiles;
    ArgMax best;
    for (int64_t tile = beg + lane; tile < end; tile += 64)
        if (a.part[tile].bin >= 0) best.take(a.part[tile].v, a.part[tile].bin);
    if (!best.block_fold<WAVES>(red_v, red_i, lane, wave)) return;
    KepBest so_far = {0.0, -1, -1};
    if (!a.first) so_far = *a.carry;
    if (best.j >= 0 && (so_far.bin < 0 || best.v > so_far.v)) so_far = a.part[(best.j - a.bin0) / kBlock];   // a later slab never wins a tie
    *a.carry = so_far;
    if (a.last) {
        if (a.best) a.best[0] = so_far.bin < 0 ? quiet_nan() : so_far.v;
        if (a.best_at) {
            a.best_at[0] = so_far.bin;
            a.best_at[1] = so_far.cell;
        }
    }
}

// ---- the solver on its own -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void kepler_anomaly_kernel(const double *phase, const double *e, int64_t count,
                                                                double *cos_out, double *sin_out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        const KepCell c = make_cell(e[i], 0.0);
        double cn, sn;
        true_anomaly(phase[i] - c.m0, c.e, c.a1, c.root, cn, sn);
        cos_out[i] = cn;
        sin_out[i] = sn;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct KepDispatch {
    int kc, groups;
    int64_t launches;
};
thread_local KepDispatch g_last = {};

// records | cells | scalars | carry | row values | row cells | the tiles' best bins, from the rows on for one slab of bins
struct KepPlan {
    int groups, cells_padded;
    int64_t tiles, slab_tiles, at_cells, at_scal, at_carry, at_row_v, at_row_c, at_part, total;
};

bool kep_sizes_ok(int64_t n, int64_t nf, int64_t ne, int64_t nm, bool want_cube) {
    if (n < 4 || n > ((int64_t)1 << 50) || nf < 1 || ne < 1 || nm < 1 || ne > kMaxCells || nm > kMaxCells ||
        ne * nm > kMaxCells)
        return false;
    if ((nf + kBlock - 1) / kBlock >= ((int64_t)1 << 31) - 8) return false;
    return !want_cube || nf <= (((int64_t)1 << 45) / (ne * nm));   // (a cube of 2^48 bytes)
}

// The slab is the whole grid unless PDC_WORK_BUDGET_GB asks for less: then as many tiles as fit, at least one.
KepPlan kep_plan(int64_t n, int64_t nf, int cells) {
    KepPlan p;
    p.groups = (cells + kCells - 1) / kCells;
    p.cells_padded = p.groups * kCells;
    p.tiles = (nf + kBlock - 1) / kBlock;
    Carve c;
    c.take((n + 1) * 32);
    p.at_cells = c.take(p.cells_padded * (int64_t)sizeof(KepCell));
    p.at_scal = c.take(32);
    p.at_carry = c.take(sizeof(KepBest));
    p.slab_tiles = p.tiles;
    const int64_t per_tile = (int64_t)p.groups * kBlock * 12 + (int64_t)sizeof(KepBest);   // its rows (value + index), its best bin
    const int64_t fixed = c.at + 3 * 256;                                                   // (the three parts' roundings)
    const int64_t budget = work_budget();
    if (budget > 0 && fixed + p.tiles * per_tile > budget) {
        const int64_t fit = (budget - fixed) / per_tile;
        p.slab_tiles = fit < 1 ? 1 : fit;
    }
    p.at_row_v = c.take(p.groups * p.slab_tiles * kBlock * 8);
    p.at_row_c = c.take(p.groups * p.slab_tiles * kBlock * 4);
    p.at_part = c.take(p.slab_tiles * (int64_t)sizeof(KepBest));
    p.total = c.at;
    return p;
}

int kep_validate(int64_t n, double f0, double delta, int64_t nf, int64_t ne, int64_t nm, const double *ecc,
                 const double *m0, bool any_output, bool want_cube) {
    PDC_REQUIRE(std::isfinite(f0) && f0 >= 0.0, "kepler: the first frequency must be finite and not negative");
    PDC_REQUIRE(std::isfinite(delta) && delta > 0.0, "kepler: the grid step must be finite and positive");
    PDC_REQUIRE(nf >= 1, "kepler: at least one frequency is needed (got %lld)", (long long)nf);
    PDC_REQUIRE(n >= 4, "kepler: three parameters are fitted, at least 4 samples are needed (got %lld)", (long long)n);
    PDC_REQUIRE(ne >= 1 && nm >= 1 && ne <= kMaxCells && nm <= kMaxCells && ne * nm <= kMaxCells,
                "kepler: 1 <= ne, 1 <= nm and ne * nm <= %d are needed (got %lld x %lld)", kMaxCells, (long long)ne,
                (long long)nm);
    if (ecc)   // (host lists only: the `_dev` form cannot look at them)
        for (int64_t k = 0; k < ne; ++k)
            PDC_REQUIRE(ecc[k] >= 0.0 && ecc[k] <= kMaxEcc, "kepler: ecc[%lld] is not in [0, %.2f]", (long long)k, kMaxEcc);
    if (m0)
        for (int64_t l = 0; l < nm; ++l)
            PDC_REQUIRE(m0[l] >= 0.0 && m0[l] < 1.0, "kepler: m0[%lld] is not in [0, 1)", (long long)l);
    PDC_REQUIRE(any_output, "kepler: every output is NULL");
    PDC_REQUIRE(kep_sizes_ok(n, nf, ne, nm, want_cube), "kepler: grid too large");
    return PDC_OK;
}

// `work`: plan.total bytes.  Inputs and outputs are device pointers, any output may be NULL.
int kep_enqueue(hipStream_t st, const double *d_t, const double *d_y, const double *d_dy, int64_t n, double f0,
                double delta, int64_t nf, const double *d_ecc, int ne, const double *d_m0, int nm, int fit_mean, int psd,
                const KepPlan &plan, double *d_power, int32_t *d_cell, double *d_cube, double *d_best,
                int64_t *d_best_at, void *work) {
    char *base = static_cast<char *>(work);
    KepPrepArgs p;
    p.t = d_t;
    p.y = d_y;
    p.dy = d_dy;
    p.ecc = d_ecc;
    p.m0 = d_m0;
    p.n = n;
    p.ne = ne;
    p.nm = nm;
    p.cells_padded = plan.cells_padded;
    p.fit_mean = fit_mean;
    p.rec = reinterpret_cast<double *>(base);
    p.cells = reinterpret_cast<KepCell *>(base + plan.at_cells);
    p.scal = reinterpret_cast<double *>(base + plan.at_scal);
    hipLaunchKernelGGL(kepler_prep_kernel, dim3(1), dim3(kPrepBlock), 0, st, p);
    PDC_HIP(hipGetLastError());
    KepArgs a;
    a.rec = p.rec;
    a.scal = p.scal;
    a.cells = p.cells;
    a.n = n;
    a.nf = nf;
    a.f0 = f0;
    a.delta = delta;
    a.cell_count = ne * nm;
    a.groups = plan.groups;
    a.fit_mean = fit_mean;
    a.psd = psd;
    a.row_v = reinterpret_cast<double *>(base + plan.at_row_v);
    a.row_c = reinterpret_cast<int32_t *>(base + plan.at_row_c);
    a.slab_pitch = plan.slab_tiles * kBlock;
    a.cube = d_cube;
    a.power = d_power;
    a.cell = d_cell;
    a.carry = reinterpret_cast<KepBest *>(base + plan.at_carry);
    a.part = reinterpret_cast<KepBest *>(base + plan.at_part);
    a.best = d_best;
    a.best_at = d_best_at;
    g_last = {kCells, plan.groups, (plan.tiles + plan.slab_tiles - 1) / plan.slab_tiles};
    for (int64_t tile0 = 0; tile0 < plan.tiles; tile0 += plan.slab_tiles) {
        const int64_t here = plan.tiles - tile0 < plan.slab_tiles ? plan.tiles - tile0 : plan.slab_tiles;
        a.bin0 = tile0 * kBlock;
        a.slab_bins = nf - a.bin0 < here * kBlock ? nf - a.bin0 : here * kBlock;
        a.first = tile0 == 0;
        a.last = tile0 + here == plan.tiles;
        hipLaunchKernelGGL((kepler_scan_kernel<kCells>), dim3((unsigned)here, (unsigned)plan.groups), dim3(kBlock), 0, st,
                           a);
        PDC_HIP(hipGetLastError());
        hipLaunchKernelGGL(kepler_fold_kernel, dim3((unsigned)here), dim3(kBlock), 0, st, a);
        PDC_HIP(hipGetLastError());
        hipLaunchKernelGGL(kepler_best_kernel, dim3(1), dim3(kPrepBlock), 0, st, a);
        PDC_HIP(hipGetLastError());
    }
    return PDC_OK;
}

}  // namespace

extern "C" {

int pdc_kepler_cell_group(void) { return kCells; }

int64_t pdc_kepler_tile_bins(void) { return kBlock; }

int64_t pdc_kepler_work_bytes(int64_t n, int64_t nf, int64_t ne, int64_t nm, int want_cube) {
    if (!kep_sizes_ok(n, nf, ne, nm, want_cube != 0)) return -1;
    return kep_plan(n, nf, (int)(ne * nm)).total;
}

int pdc_kepler_last_dispatch(int *kc, int *groups, int64_t *launches) {
    if (kc) *kc = g_last.kc;
    if (groups) *groups = g_last.groups;
    if (launches) *launches = g_last.launches;
    return PDC_OK;
}

int pdc_kepler_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                        double f0, double delta, int64_t nf, const double *d_ecc, int64_t ne, const double *d_m0,
                        int64_t nm, int fit_mean, int psd, double *d_power, int32_t *d_cell, double *d_cube,
                        double *d_best, int64_t *d_best_at) {
    PDC_TRY(kep_validate(n, f0, delta, nf, ne, nm, nullptr, nullptr, d_power || d_cell || d_cube || d_best || d_best_at,
                         d_cube != nullptr));
    PDC_REQUIRE(d_t && d_y && d_ecc && d_m0, "kepler: NULL argument");
    PDC_TRY(use_device(device));
    const KepPlan plan = kep_plan(n, nf, (int)(ne * nm));
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, plan.total, &work));
    return kep_enqueue(st, d_t, d_y, d_dy, n, f0, delta, nf, d_ecc, (int)ne, d_m0, (int)nm, fit_mean, psd, plan, d_power,
                       d_cell, d_cube, d_best, d_best_at, work);
}

int pdc_kepler_scan(const double *t, const double *y, const double *dy, int64_t n, double f0, double delta, int64_t nf,
                    const double *ecc, int64_t ne, const double *m0, int64_t nm, int fit_mean, int psd, double *power_out,
                    int32_t *cell_out, double *cube_out, double *best_out, int64_t *best_at_out, int device) {
    PDC_REQUIRE(ecc && m0, "kepler: NULL argument");
    PDC_TRY(kep_validate(n, f0, delta, nf, ne, nm, ecc, m0, power_out || cell_out || cube_out || best_out || best_at_out,
                         cube_out != nullptr));
    PDC_REQUIRE(t && y, "kepler: NULL argument");
    for (int64_t i = 0; i < n; ++i) PDC_REQUIRE(std::isfinite(t[i]), "kepler: t[%lld] is not finite", (long long)i);
    HostCall hc(device);
    PDC_TRY(hc.status);
    const KepPlan plan = kep_plan(n, nf, (int)(ne * nm));
    double *d_t = hc.in(SLOT_IN0, t, n * 8), *d_y = hc.in(SLOT_IN1, y, n * 8), *d_dy = hc.in(SLOT_IN2, dy, n * 8);
    Carve cl;   // the two lists share a block
    const int64_t at_ecc = cl.take(ne * 8), at_m0 = cl.take(nm * 8);
    char *d_lists = hc.out<char>(SLOT_IN3, cl.at);
    const int64_t cube_bytes = nf * ne * nm * 8;
    double *d_cube = cube_out ? hc.out<double>(SLOT_OUT0, cube_bytes) : nullptr;
    Carve c;    // the small outputs another: power | cell | best | best_at
    const int64_t at_power = c.take(nf * 8), at_cell = c.take(nf * 4), at_best = c.take(8), at_best_at = c.take(16);
    char *d_small = hc.out<char>(SLOT_OUT1, c.at);
    void *d_work = hc.reserve(SLOT_WORK, plan.total);
    PDC_TRY(hc.status);
    hc.put(d_lists + at_ecc, ecc, ne * 8);
    hc.put(d_lists + at_m0, m0, nm * 8);
    PDC_TRY(hc.status);
    double *d_power = power_out ? reinterpret_cast<double *>(d_small + at_power) : nullptr;
    int32_t *d_cell = cell_out ? reinterpret_cast<int32_t *>(d_small + at_cell) : nullptr;
    double *d_best = best_out ? reinterpret_cast<double *>(d_small + at_best) : nullptr;
    int64_t *d_best_at = best_at_out ? reinterpret_cast<int64_t *>(d_small + at_best_at) : nullptr;
    PDC_TRY(kep_enqueue(hc.stream(), d_t, d_y, d_dy, n, f0, delta, nf, reinterpret_cast<double *>(d_lists + at_ecc), (int)ne,
                        reinterpret_cast<double *>(d_lists + at_m0), (int)nm, fit_mean, psd, plan, d_power, d_cell, d_cube,
                        d_best, d_best_at, d_work));
    hc.back(power_out, d_power, nf * 8);
    hc.back(cell_out, d_cell, nf * 4);
    hc.back(cube_out, d_cube, cube_bytes);
    hc.back(best_out, d_best, 8);
    hc.back(best_at_out, d_best_at, 16);
    return hc.finish();
}

int pdc_kepler_anomaly(const double *phase, const double *e, int64_t count, double *cos_out, double *sin_out, int device) {
    PDC_REQUIRE(count >= 0 && count <= ((int64_t)1 << 40), "kepler_anomaly: the count must be 0 .. 2^40");
    if (count == 0) return PDC_OK;
    PDC_REQUIRE(phase && e && cos_out && sin_out, "kepler_anomaly: NULL argument");
    for (int64_t i = 0; i < count; ++i) {
        PDC_REQUIRE(std::isfinite(phase[i]), "kepler_anomaly: phase[%lld] is not finite", (long long)i);
        PDC_REQUIRE(e[i] >= 0.0 && e[i] <= kMaxEcc, "kepler_anomaly: e[%lld] is not in [0, %.2f]", (long long)i, kMaxEcc);
    }
    HostCall hc(device);
    PDC_TRY(hc.status);
    double *d_phase = hc.in(SLOT_IN0, phase, count * 8), *d_e = hc.in(SLOT_IN1, e, count * 8);
    double *d_cos = hc.out<double>(SLOT_OUT0, count * 8), *d_sin = hc.out<double>(SLOT_OUT1, count * 8);
    PDC_TRY(hc.status);
    const int64_t blocks = (count + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(kepler_anomaly_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, hc.stream(),
                       d_phase, d_e, count, d_cos, d_sin);
    PDC_HIP(hipGetLastError());
    hc.back(cos_out, d_cos, count * 8);
    hc.back(sin_out, d_sin, count * 8);
    return hc.finish();
}

}  // extern "C"
