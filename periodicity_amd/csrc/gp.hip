// Gaussian-process likelihood scans on gfx950: the log-likelihood of one unevenly sampled curve under many celerite
// kernels (Foreman-Mackey, Agol, Ambikasaran & Angus 2017, AJ 154, 220; the overflow-free recursion of Foreman-Mackey
// 2018, RNAAS 2, 31) - one per hyper-parameter vector of a grid, an MCMC ensemble or a nested sampler's live points.
// The reference (its gp.py) evaluates `gp.compute(...); gp.log_likelihood(y)` once per vector on the CPU through
// celerite2; here a lane owns a candidate and every lane of a wave reads the same sample.
//
// A candidate is J terms (a, b, c, nu) - k(D) = sum_j exp(-c_j |D|) (a_j cos 2 pi nu_j D + b_j sin 2 pi nu_j |D|), a real
// term is b = nu = 0 - a jitter s and a mean.  With R = 2J, per sample n (tau_n = t_n - t_0, never decreasing):
//     U = (a cos + b sin, a sin - b cos)_j,  V = (cos, sin)_j  of 2 pi nu_j tau_n,   P = exp(-c_j (tau_n - tau_n-1))
//     S <- P o (S + D W W^T) o P^T,  f <- P o (f + W z)        (from the sample before; S = 0, f = 0 at the first)
//     D = var_n + s + sum a - U S U^T,   W = (V - S U^T) / D,   z = y_n - mean - U f
//     ln L = -1/2 sum (z^2 / D + ln D) - N/2 ln 2 pi.
// With fit_mean a second solve z1 = 1 - U f1 on the all-ones vector shares S, D, W:
//     mean = sum z z1 / D  /  sum z1^2 / D,   ln L(mean) = ln L(0) + 1/2 (sum z z1 / D)^2 / sum z1^2 / D.
//
// Decomposition
//   gp_prep_kernel       a thread per sample: its 32-byte record {tau, tau - tau_before, y, var}.
//   gp_pack_kernel       a thread per candidate of the slab: its J x 4 coefficients from the caller's [M][J][4] to the
//                        workspace's [J][4][slab], which the scan's first loads read coalesced.
//   gp_loglike_kernel    <J, FIT_MEAN>: a lane per candidate, S (R (R + 1) / 2), f (R) and f1 (R) in registers.  A
//                        workgroup is one wave; it stages kChunk records in LDS and every lane reads the same address.
//                        Per (sample, term) one sincos_cycles of frac(nu tau) and one exp_neg; per sample one division;
//                        sum ln D as a running product (LogProduct), one log per lane.  No branch depends on a value:
//                        a candidate whose D is not a positive finite number keeps running on whatever it holds, its
//                        status keeps the first such sample (1-based), its ln L is -inf.
//   gp_fold_kernel       a thread per period over its nq cells: the largest finite ln L (the first of equal ones),
//                        its cell, its mean, and logsumexp of the finite cells - ln nq; per tile of 256 periods the best.
//   gp_best_kernel       one workgroup: the tiles' best periods in ascending order.
// No atomics.  A candidate's bits depend on its coefficients and the curve alone: not on its index, on M, on the
// candidates beside it or on the slabs PDC_WORK_BUDGET_GB cuts M into.
#include "pdc_internal.h"
#include "gls_sums.h"
#include "gp_terms.h"

#include <cmath>

using namespace pdc;

namespace {

constexpr int kBlock = 64;         // candidates per workgroup: one wave
constexpr int kChunk = 128;        // sample records staged in LDS at a time
constexpr int kFoldBlock = 256;    // periods per fold tile
constexpr int kBestBlock = 1024;
constexpr int kMaxCells = 65535;   // nq
constexpr int64_t kMaxSamples = ((int64_t)1 << 31) - 1;    // status is a 32-bit sample index
constexpr int64_t kMaxCandidates = (int64_t)1 << 40;
constexpr int64_t kMaxPeriods = (int64_t)1 << 38;          // 2^30 fold tiles of 256
constexpr int64_t kMaxSlab = (int64_t)1 << 30;             // candidates of one launch (2^24 workgroups)

__device__ __forceinline__ double quiet_nan() { return __builtin_nan(""); }
__device__ __forceinline__ bool is_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }   // (false for NaN)

struct GpArgs {
    const double *t_rel, *y, *var;   // [n]
    int64_t n;
    double4 *rec;                    // [n]
    const double *coeff;             // caller's [M][J][4]
    double *coef;                    // workspace [J][4][pitch]
    const double *jitter, *mean;     // [M]; mean may be NULL
    int64_t m0, count, pitch;        // the slab: candidates [m0, m0 + count)
    double *loglike, *mean_out;      // [M], any may be NULL
    int32_t *status;
};

__global__ __launch_bounds__(256) void gp_prep_kernel(GpArgs p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const double tau = p.t_rel[i];
    p.rec[i] = make_double4(tau, i == 0 ? 0.0 : tau - p.t_rel[i - 1], p.y[i], p.var[i]);
}

template <int J>
__global__ __launch_bounds__(256) void gp_pack_kernel(GpArgs p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.count) return;
    const double *src = p.coeff + (p.m0 + i) * (J * 4);
#pragma unroll
    for (int e = 0; e < J * 4; ++e) p.coef[e * p.pitch + i] = src[e];
}

template <int J, bool FIT_MEAN>
__global__ __launch_bounds__(kBlock) void gp_loglike_kernel(GpArgs p) {
    constexpr int R = 2 * J;
    constexpr int NS = R * (R + 1) / 2;
    __shared__ double4 stage[kChunk];
    const int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = at < p.count;
    const int64_t il = live ? at : p.count - 1;   // a lane past the slab runs the last candidate again and stores nothing
    const int64_t m = p.m0 + il;

    double a[J], b[J], c[J], nu[J];
    double diag = p.jitter[m];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        a[j] = p.coef[(j * 4 + 0) * p.pitch + il];
        b[j] = p.coef[(j * 4 + 1) * p.pitch + il];
        c[j] = p.coef[(j * 4 + 2) * p.pitch + il];
        nu[j] = p.coef[(j * 4 + 3) * p.pitch + il];
        diag += a[j];
    }
    const double mu = (!FIT_MEAN && p.mean) ? p.mean[m] : 0.0;

    double S[NS], f[R], f1[R];
#pragma unroll
    for (int e = 0; e < NS; ++e) S[e] = 0.0;
#pragma unroll
    for (int i = 0; i < R; ++i) f[i] = f1[i] = 0.0;
    double q = 0.0, q01 = 0.0, q11 = 0.0;
    LogProduct lnd;
    int bad_at = 0;

    for (int64_t base = 0; base < p.n; base += kChunk) {
        const int len = (int)(p.n - base < kChunk ? p.n - base : kChunk);
        __syncthreads();
        for (int s = threadIdx.x; s < len; s += kBlock) stage[s] = p.rec[base + s];
        __syncthreads();
        for (int s = 0; s < len; ++s) {
            const double4 r = stage[s];   // {tau, dtau, y, var}: one address for the wave
            double U[R], V[R], P[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                double sn, cs;
                sincos_cycles(frac_product(nu[j], r.x), sn, cs);
                P[j] = exp_neg(c[j] * r.y);
                U[2 * j] = __builtin_fma(a[j], cs, b[j] * sn);
                U[2 * j + 1] = __builtin_fma(a[j], sn, -(b[j] * cs));
                V[2 * j] = cs;
                V[2 * j + 1] = sn;
            }
            // the step from the sample before: S <- P o S o P^T, f <- P o f (S and f already hold + D W W^T, + W z)
#pragma unroll
            for (int ji = 0; ji < J; ++ji)
#pragma unroll
                for (int jk = ji; jk < J; ++jk) {
                    const double pp = P[ji] * P[jk];
#pragma unroll
                    for (int i = 2 * ji; i < 2 * ji + 2; ++i)
#pragma unroll
                        for (int k = 2 * jk; k < 2 * jk + 2; ++k)
                            if (i <= k) S[sym_index<R>(i, k)] *= pp;
                }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                f[i] *= P[i / 2];
                if (FIT_MEAN) f1[i] *= P[i / 2];
            }
            // D, W, z
            double SU[R], usu = 0.0, uf = 0.0, uf1 = 0.0;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < R; ++k) acc = __builtin_fma(S[sym_index<R>(i, k)], U[k], acc);
                SU[i] = acc;
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                usu = __builtin_fma(U[i], SU[i], usu);
                uf = __builtin_fma(U[i], f[i], uf);
                if (FIT_MEAN) uf1 = __builtin_fma(U[i], f1[i], uf1);
            }
            const double D = (r.w + diag) - usu;
            const double inv = 1.0 / D;
            const double z = (r.z - mu) - uf;
            const double z1 = 1.0 - uf1;
            q = __builtin_fma(z * z, inv, q);
            if (FIT_MEAN) {
                q01 = __builtin_fma(z * z1, inv, q01);
                q11 = __builtin_fma(z1 * z1, inv, q11);
            }
            lnd.times(D);
            const bool good = D > 0.0 && is_finite(D);
            bad_at = (bad_at == 0 && !good) ? (int)(base + s) + 1 : bad_at;
            // S += D W W^T = G W^T with G = V - S U^T = D W;  f += W z
            double W[R];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                SU[i] = V[i] - SU[i];
                W[i] = SU[i] * inv;
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
#pragma unroll
                for (int k = i; k < R; ++k) S[sym_index<R>(i, k)] = __builtin_fma(SU[i], W[k], S[sym_index<R>(i, k)]);
                f[i] = __builtin_fma(W[i], z, f[i]);
                if (FIT_MEAN) f1[i] = __builtin_fma(W[i], z1, f1[i]);
            }
        }
        lnd.carry();
    }

    constexpr double kHalfLog2Pi = 0.918938533204672741780;
    double ll = __builtin_fma(-(double)p.n, kHalfLog2Pi, -0.5 * (q + lnd.log()));
    double mean = mu;
    if (FIT_MEAN) {
        mean = q01 / q11;
        ll = __builtin_fma(0.5 * q01, mean, ll);
    }
    if (!live) return;
    if (p.loglike) p.loglike[m] = bad_at ? -__builtin_inf() : ll;
    if (p.mean_out) p.mean_out[m] = bad_at ? quiet_nan() : mean;
    if (p.status) p.status[m] = bad_at;
}

// ---- per period the best cell and the marginal, per tile and over all periods the best period ---------------------
struct GpBest {
    double v;
    long long period, cell;
};

struct GpFoldArgs {
    const double *cube, *means;   // [np][nq]
    int64_t np;
    int nq;
    double *profile, *marginal, *mean_out;   // [np], any may be NULL
    int32_t *cell;
    GpBest *part;                 // [tiles]
    double *best;
    int64_t *best_at;
};

__global__ __launch_bounds__(kFoldBlock) void gp_fold_kernel(GpFoldArgs a) {
    constexpr int WAVES = kFoldBlock / 64;
    __shared__ double red_v[WAVES];
    __shared__ long long red_i[WAVES];
    __shared__ int tile_cell[kFoldBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pi = (int64_t)blockIdx.x * kFoldBlock + threadIdx.x;
    ArgMax best;
    int cell = -1;
    if (pi < a.np) {
        const double *row = a.cube + pi * a.nq;
        double top = 0.0;
        for (int c = 0; c < a.nq; ++c) {
            const double v = row[c];
            if (is_finite(v) && (cell < 0 || v > top)) {
                top = v;
                cell = c;
            }
        }
        double sum = 0.0;
        for (int c = 0; c < a.nq; ++c) {
            const double v = row[c];
            if (is_finite(v)) sum += ::exp(v - top);
        }
        if (a.profile) a.profile[pi] = cell < 0 ? quiet_nan() : top;
        if (a.cell) a.cell[pi] = cell;
        if (a.marginal) a.marginal[pi] = cell < 0 ? -__builtin_inf() : (top + ::log(sum)) - ::log((double)a.nq);
        if (a.mean_out) a.mean_out[pi] = cell < 0 ? quiet_nan() : a.means[pi * a.nq + cell];
        if (cell >= 0) best.take(top, pi);
    }
    tile_cell[threadIdx.x] = cell;
    if (!best.block_fold<WAVES>(red_v, red_i, lane, wave)) return;   // (its barrier also publishes tile_cell)
    GpBest part = {0.0, best.j, -1};
    if (best.j >= 0) {
        part.v = best.v;
        part.cell = tile_cell[best.j - (int64_t)blockIdx.x * kFoldBlock];
    }
    a.part[blockIdx.x] = part;
}

// Wave w takes the w-th run of tiles, its lanes interleaved; wave_fold compares the periods of equal maxima, the waves
// fold in order: the lowest period of equal maxima stays.
__global__ __launch_bounds__(kBestBlock) void gp_best_kernel(GpFoldArgs a) {
    constexpr int WAVES = kBestBlock / 64;
    __shared__ double red_v[WAVES];
    __shared__ long long red_i[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tiles = (a.np + kFoldBlock - 1) / kFoldBlock;
    const int64_t run = (tiles + WAVES - 1) / WAVES;
    const int64_t beg = wave * run, end = beg + run < tiles ? beg + run : tiles;
    ArgMax best;
    for (int64_t tile = beg + lane; tile < end; tile += 64)
        if (a.part[tile].period >= 0) best.take(a.part[tile].v, a.part[tile].period);
    if (!best.block_fold<WAVES>(red_v, red_i, lane, wave)) return;
    if (a.best) a.best[0] = best.j < 0 ? quiet_nan() : best.v;
    if (a.best_at) {
        a.best_at[0] = best.j;
        a.best_at[1] = best.j < 0 ? -1 : a.part[best.j / kFoldBlock].cell;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct GpDispatch {
    int J, fit_mean;
    int64_t launches;
};
thread_local GpDispatch g_last = {};

bool gp_sizes_ok(int64_t n, int64_t M, int J) {
    return n >= 1 && n <= kMaxSamples && J >= 1 && J <= kGpMaxTerms && M >= 1 && M <= kMaxCandidates;
}

// records | for a scan: log-likelihoods [M] (unless the caller's cube takes them) | means [M] | the fold's tiles | the
// slab's coefficients.  The slab is all of M unless PDC_WORK_BUDGET_GB asks for less: then as many workgroups of candidates as
// fit, at least one.
struct GpPlan {
    int64_t slab, slabs, at_cube, at_means, at_part, at_coef, total;
};

GpPlan gp_plan(int64_t n, int64_t M, int J, bool want_cube, bool scan) {
    GpPlan p;
    Carve c;
    c.take(n * 32);
    p.at_cube = c.take(scan && !want_cube ? M * 8 : 0);   // (only the fold reads likelihoods and means back)
    p.at_means = c.take(scan ? M * 8 : 0);
    p.at_part = c.take(scan ? (M + kFoldBlock - 1) / kFoldBlock * (int64_t)sizeof(GpBest) : 0);
    const int64_t per = (int64_t)J * 32;
    p.slab = M < kMaxSlab ? M : kMaxSlab;
    const int64_t budget = work_budget();
    if (budget > 0 && c.at + up256(p.slab * per) > budget) {
        const int64_t fit = (budget - c.at) / (per * kBlock) * kBlock;
        p.slab = fit < kBlock ? kBlock : fit;
        if (p.slab > M) p.slab = M;
    }
    p.slabs = (M + p.slab - 1) / p.slab;
    p.at_coef = c.take(p.slab * per);
    p.total = c.at;
    return p;
}

int gp_validate(int64_t n, int J, int64_t M, int fit_mean, bool has_mean, bool any_output) {
    PDC_REQUIRE(n >= 1 && n <= kMaxSamples, "gp: 1 <= n < 2^31 samples are needed (got %lld)", (long long)n);
    PDC_REQUIRE(J >= 1 && J <= kGpMaxTerms, "gp: 1 <= J <= %d terms are needed (got %d)", kGpMaxTerms, J);
    PDC_REQUIRE(M >= 1 && M <= kMaxCandidates, "gp: 1 <= M <= 2^40 candidates are needed (got %lld)", (long long)M);
    PDC_REQUIRE(!(fit_mean && has_mean), "gp: fit_mean profiles the mean out, no mean may be given with it");
    PDC_REQUIRE(any_output, "gp: every output is NULL");
    return PDC_OK;
}

int gp_validate_scan(int64_t M, int64_t np, int64_t nq) {
    PDC_REQUIRE(np >= 1 && nq >= 1 && nq <= kMaxCells && np <= M && np * nq == M,
                "gp: np x nq must be M with 1 <= nq <= %d (got %lld x %lld for M = %lld)", kMaxCells, (long long)np,
                (long long)nq, (long long)M);
    PDC_REQUIRE(np <= kMaxPeriods, "gp: at most 2^38 periods (got %lld)", (long long)np);   // (the fold's tiles are a grid's x)
    return PDC_OK;
}

// The host form's look at its arrays.
int gp_check_arrays(const double *t_rel, const double *y, const double *var, int64_t n, const double *coeff, int J,
                    const double *jitter, const double *mean, int64_t M) {
    PDC_REQUIRE(t_rel && y && var && coeff && jitter, "gp: NULL argument");
    PDC_REQUIRE(t_rel[0] == 0.0, "gp: t_rel must start at 0 (it is t - t[0] of the sorted times)");
    for (int64_t i = 0; i < n; ++i) {
        PDC_REQUIRE(std::isfinite(t_rel[i]), "gp: t_rel[%lld] is not finite", (long long)i);
        PDC_REQUIRE(i == 0 || t_rel[i] >= t_rel[i - 1], "gp: t_rel must never decrease (at %lld)", (long long)i);
        PDC_REQUIRE(std::isfinite(y[i]), "gp: y[%lld] is not finite", (long long)i);
        PDC_REQUIRE(std::isfinite(var[i]) && var[i] >= 0.0, "gp: var[%lld] is not finite and >= 0", (long long)i);
    }
    for (int64_t m = 0; m < M; ++m) {
        for (int e = 0; e < J * 4; ++e)
            PDC_REQUIRE(std::isfinite(coeff[m * J * 4 + e]), "gp: a coefficient of candidate %lld is not finite",
                        (long long)m);
        for (int j = 0; j < J; ++j)
            PDC_REQUIRE(coeff[(m * J + j) * 4 + 2] >= 0.0, "gp: c of term %d of candidate %lld is negative", j,
                        (long long)m);
        PDC_REQUIRE(std::isfinite(jitter[m]) && jitter[m] >= 0.0, "gp: jitter[%lld] is not finite and >= 0", (long long)m);
        PDC_REQUIRE(!mean || std::isfinite(mean[m]), "gp: mean[%lld] is not finite", (long long)m);
    }
    return PDC_OK;
}

template <int J>
void gp_launch_slab(hipStream_t st, const GpArgs &p, int fit_mean) {
    hipLaunchKernelGGL(gp_pack_kernel<J>, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, st, p);
    const dim3 grid((unsigned)((p.count + kBlock - 1) / kBlock));
    if (fit_mean)
        hipLaunchKernelGGL((gp_loglike_kernel<J, true>), grid, dim3(kBlock), 0, st, p);
    else
        hipLaunchKernelGGL((gp_loglike_kernel<J, false>), grid, dim3(kBlock), 0, st, p);
}

// `work`: plan.total bytes.  Inputs and outputs are device pointers; fold == NULL: the likelihoods alone.
int gp_enqueue(hipStream_t st, const double *d_t, const double *d_y, const double *d_var, int64_t n, const double *d_coeff,
               int J, const double *d_jitter, const double *d_mean, int64_t M, int fit_mean, const GpPlan &plan,
               double *d_loglike, double *d_mean_out, int32_t *d_status, GpFoldArgs *fold, void *work) {
    char *base = static_cast<char *>(work);
    GpArgs p;
    p.t_rel = d_t;
    p.y = d_y;
    p.var = d_var;
    p.n = n;
    p.rec = reinterpret_cast<double4 *>(base);
    p.coeff = d_coeff;
    p.coef = reinterpret_cast<double *>(base + plan.at_coef);
    p.jitter = d_jitter;
    p.mean = d_mean;
    p.pitch = plan.slab;
    p.loglike = d_loglike;
    p.mean_out = d_mean_out;
    p.status = d_status;
    if (fold) {   // the fold reads every likelihood and every mean
        if (!p.loglike) p.loglike = reinterpret_cast<double *>(base + plan.at_cube);
        if (!p.mean_out) p.mean_out = reinterpret_cast<double *>(base + plan.at_means);
    }
    g_last = {J, fit_mean ? 1 : 0, plan.slabs};
    hipLaunchKernelGGL(gp_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    PDC_HIP(hipGetLastError());
    for (int64_t m0 = 0; m0 < M; m0 += plan.slab) {
        p.m0 = m0;
        p.count = M - m0 < plan.slab ? M - m0 : plan.slab;
        switch (J) {
            case 1: gp_launch_slab<1>(st, p, fit_mean); break;
            case 2: gp_launch_slab<2>(st, p, fit_mean); break;
            case 3: gp_launch_slab<3>(st, p, fit_mean); break;
            default: gp_launch_slab<4>(st, p, fit_mean); break;
        }
        PDC_HIP(hipGetLastError());
    }
    if (fold) {
        fold->cube = p.loglike;
        fold->means = p.mean_out;
        fold->part = reinterpret_cast<GpBest *>(base + plan.at_part);
        const int64_t tiles = (fold->np + kFoldBlock - 1) / kFoldBlock;
        hipLaunchKernelGGL(gp_fold_kernel, dim3((unsigned)tiles), dim3(kFoldBlock), 0, st, *fold);
        PDC_HIP(hipGetLastError());
        hipLaunchKernelGGL(gp_best_kernel, dim3(1), dim3(kBestBlock), 0, st, *fold);
        PDC_HIP(hipGetLastError());
    }
    return PDC_OK;
}

// The host form of both entries: fold == NULL is pdc_gp_loglike.
int gp_host(const double *t_rel, const double *y, const double *var, int64_t n, const double *coeff, int J,
            const double *jitter, const double *mean, int64_t M, int fit_mean, double *loglike_out, double *mean_out,
            int32_t *status_out, int64_t np, int nq, double *profile_out, int32_t *cell_out, double *marginal_out,
            double *period_mean_out, double *best_out, int64_t *best_at_out, bool scan, int device) {
    PDC_TRY(gp_check_arrays(t_rel, y, var, n, coeff, J, jitter, mean, M));
    HostCall hc(device);
    PDC_TRY(hc.status);
    const GpPlan plan = gp_plan(n, M, J, loglike_out != nullptr, scan);
    Carve ci;   // t_rel | y | var | jitter | mean share a block
    const int64_t at_t = ci.take(n * 8), at_y = ci.take(n * 8), at_var = ci.take(n * 8), at_jit = ci.take(M * 8),
                  at_mean = ci.take(mean ? M * 8 : 0);
    char *d_in = hc.out<char>(SLOT_IN0, ci.at);
    const double *d_coeff = hc.in(SLOT_IN1, coeff, M * J * 32);
    Carve cm;   // the per-candidate outputs another: ln L | mean | status
    const int64_t at_ll = cm.take(loglike_out ? M * 8 : 0), at_mu = cm.take(mean_out ? M * 8 : 0),
                  at_st = cm.take(status_out ? M * 4 : 0);
    char *d_cand = hc.out<char>(SLOT_OUT0, cm.at + 256);
    Carve cp;   // the per-period outputs a third: profile | cell | marginal | mean | best | best_at
    const int64_t at_pr = cp.take(np * 8), at_ce = cp.take(np * 4), at_ma = cp.take(np * 8), at_pm = cp.take(np * 8),
                  at_best = cp.take(8), at_best_at = cp.take(16);
    char *d_per = hc.out<char>(SLOT_OUT1, cp.at);
    void *d_work = hc.reserve(SLOT_WORK, plan.total);
    PDC_TRY(hc.status);
    hc.put(d_in + at_t, t_rel, n * 8);
    hc.put(d_in + at_y, y, n * 8);
    hc.put(d_in + at_var, var, n * 8);
    hc.put(d_in + at_jit, jitter, M * 8);
    hc.put(d_in + at_mean, mean, M * 8);
    PDC_TRY(hc.status);
    double *d_ll = loglike_out ? reinterpret_cast<double *>(d_cand + at_ll) : nullptr;
    double *d_mu = mean_out ? reinterpret_cast<double *>(d_cand + at_mu) : nullptr;
    int32_t *d_st = status_out ? reinterpret_cast<int32_t *>(d_cand + at_st) : nullptr;
    GpFoldArgs fold = {};
    fold.np = np;
    fold.nq = nq;
    fold.profile = profile_out ? reinterpret_cast<double *>(d_per + at_pr) : nullptr;
    fold.cell = cell_out ? reinterpret_cast<int32_t *>(d_per + at_ce) : nullptr;
    fold.marginal = marginal_out ? reinterpret_cast<double *>(d_per + at_ma) : nullptr;
    fold.mean_out = period_mean_out ? reinterpret_cast<double *>(d_per + at_pm) : nullptr;
    fold.best = best_out ? reinterpret_cast<double *>(d_per + at_best) : nullptr;
    fold.best_at = best_at_out ? reinterpret_cast<int64_t *>(d_per + at_best_at) : nullptr;
    PDC_TRY(gp_enqueue(hc.stream(), reinterpret_cast<double *>(d_in + at_t), reinterpret_cast<double *>(d_in + at_y),
                       reinterpret_cast<double *>(d_in + at_var), n, d_coeff, J, reinterpret_cast<double *>(d_in + at_jit),
                       mean ? reinterpret_cast<double *>(d_in + at_mean) : nullptr, M, fit_mean, plan, d_ll, d_mu, d_st,
                       scan ? &fold : nullptr, d_work));
    hc.back(loglike_out, d_ll, M * 8);
    hc.back(mean_out, d_mu, M * 8);
    hc.back(status_out, d_st, M * 4);
    if (scan) {
        hc.back(profile_out, fold.profile, np * 8);
        hc.back(cell_out, fold.cell, np * 4);
        hc.back(marginal_out, fold.marginal, np * 8);
        hc.back(period_mean_out, fold.mean_out, np * 8);
        hc.back(best_out, fold.best, 8);
        hc.back(best_at_out, fold.best_at, 16);
    }
    return hc.finish();
}

}  // namespace

extern "C" {

int pdc_gp_max_terms(void) { return kGpMaxTerms; }

int pdc_gp_chunk_samples(void) { return kChunk; }

int64_t pdc_gp_work_bytes(int64_t n, int64_t M, int J, int want_cube) {
    if (!gp_sizes_ok(n, M, J)) return -1;
    return gp_plan(n, M, J, want_cube != 0, true).total;
}

int pdc_gp_last_dispatch(int *J, int *fit_mean, int64_t *launches) {
    if (J) *J = g_last.J;
    if (fit_mean) *fit_mean = g_last.fit_mean;
    if (launches) *launches = g_last.launches;
    return PDC_OK;
}

int pdc_gp_loglike_dev(int device, void *stream, const double *d_t_rel, const double *d_y, const double *d_var, int64_t n,
                       const double *d_coeff, int J, const double *d_jitter, const double *d_mean, int64_t M, int fit_mean,
                       double *d_loglike, double *d_mean_out, int32_t *d_status) {
    PDC_TRY(gp_validate(n, J, M, fit_mean, d_mean != nullptr, d_loglike || d_mean_out || d_status));
    PDC_REQUIRE(d_t_rel && d_y && d_var && d_coeff && d_jitter, "gp: NULL argument");
    const GpPlan plan = gp_plan(n, M, J, d_loglike != nullptr, false);
    PDC_TRY(use_device(device));
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, plan.total, &work));
    return gp_enqueue(st, d_t_rel, d_y, d_var, n, d_coeff, J, d_jitter, d_mean, M, fit_mean, plan, d_loglike, d_mean_out,
                      d_status, nullptr, work);
}

int pdc_gp_loglike(const double *t_rel, const double *y, const double *var, int64_t n, const double *coeff, int J,
                   const double *jitter, const double *mean, int64_t M, int fit_mean, double *loglike_out, double *mean_out,
                   int32_t *status_out, int device) {
    PDC_TRY(gp_validate(n, J, M, fit_mean, mean != nullptr, loglike_out || mean_out || status_out));
    return gp_host(t_rel, y, var, n, coeff, J, jitter, mean, M, fit_mean, loglike_out, mean_out, status_out, 1, 1, nullptr,
                   nullptr, nullptr, nullptr, nullptr, nullptr, false, device);
}

int pdc_gp_scan_dev(int device, void *stream, const double *d_t_rel, const double *d_y, const double *d_var, int64_t n,
                    const double *d_coeff, int J, const double *d_jitter, const double *d_mean, int64_t M, int fit_mean,
                    int64_t np, int64_t nq, double *d_profile, int32_t *d_cell, double *d_marginal, double *d_period_mean,
                    double *d_cube, double *d_best, int64_t *d_best_at) {
    PDC_TRY(gp_validate(n, J, M, fit_mean, d_mean != nullptr,
                        d_profile || d_cell || d_marginal || d_period_mean || d_cube || d_best || d_best_at));
    PDC_TRY(gp_validate_scan(M, np, nq));
    PDC_REQUIRE(d_t_rel && d_y && d_var && d_coeff && d_jitter, "gp: NULL argument");
    const GpPlan plan = gp_plan(n, M, J, d_cube != nullptr, true);
    PDC_TRY(use_device(device));
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, plan.total, &work));
    GpFoldArgs fold = {};
    fold.np = np;
    fold.nq = (int)nq;
    fold.profile = d_profile;
    fold.cell = d_cell;
    fold.marginal = d_marginal;
    fold.mean_out = d_period_mean;
    fold.best = d_best;
    fold.best_at = d_best_at;
    return gp_enqueue(st, d_t_rel, d_y, d_var, n, d_coeff, J, d_jitter, d_mean, M, fit_mean, plan, d_cube, nullptr, nullptr,
                      &fold, work);
}

int pdc_gp_scan(const double *t_rel, const double *y, const double *var, int64_t n, const double *coeff, int J,
                const double *jitter, const double *mean, int64_t M, int fit_mean, int64_t np, int64_t nq,
                double *profile_out, int32_t *cell_out, double *marginal_out, double *period_mean_out, double *cube_out,
                double *best_out, int64_t *best_at_out, int device) {
    PDC_TRY(gp_validate(n, J, M, fit_mean, mean != nullptr,
                        profile_out || cell_out || marginal_out || period_mean_out || cube_out || best_out || best_at_out));
    PDC_TRY(gp_validate_scan(M, np, nq));
    return gp_host(t_rel, y, var, n, coeff, J, jitter, mean, M, fit_mean, cube_out, nullptr, nullptr, np, (int)nq,
                   profile_out, cell_out, marginal_out, period_mean_out, best_out, best_at_out, true, device);
}

}  // extern "C"
