/*
 * TEST INFRASTRUCTURE — plain-C restatement of the reference's scan arithmetic, for parity
 * cases too large for the numpy oracle (oracle/scan_oracle.py is the primary statement; this
 * file is checked against it in tests/test_oracle_golden.py).  Never linked into the product.
 *
 * Paths cited are relative to /root/reference/src/periodicity/.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* S_j = sum_i h_i sin(2 pi f_j t_i), C_j likewise with cos: the definition at spectral.py:13-15,
 * evaluated directly in x87 80-bit long double. */
void oracle_trig_sums_exact(const double *t, const double *h, int64_t n, const double *freq,
                            int64_t nf, double *S, double *C) {
    const long double two_pi = 2.0L * acosl(-1.0L);
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < nf; ++j) {
        const long double w = two_pi * (long double)freq[j];
        long double s = 0.0L, c = 0.0L;
        for (int64_t i = 0; i < n; ++i) {
            const long double ph = w * (long double)t[i];
            s += (long double)h[i] * sinl(ph);
            c += (long double)h[i] * cosl(ph);
        }
        S[j] = (double)s;
        C[j] = (double)c;
    }
}

/* The six GLS sums with the phase REDUCED IN CYCLES before any rounding that scales with it: the checker for
 * error budgets of ~1e-14, where oracle_trig_sums_exact's 64-bit product 2 pi f t (2^-64 of the PHASE: 2e-14 rad
 * at 5e4 cycles) is itself the size of what is measured.  t' = t - t[0] in double, as the device takes it;
 * p = fl(f t'), e = fma(f, t', -p) is the product's exact remainder, p - rint(p) is exact, and
 * r = (long double)(p - rint(p)) + (long double)e carries f t' mod 1 with no rounding at all (|e| <= ulp(p) / 2 and
 * the 64-bit significand holds both terms whenever they are 11 bits apart or less; otherwise the rounding is
 * 2^-64 of a number below 1/2).  Then sinl / cosl of 2 pi r and long-double sums in sample order.  The weights come
 * as long double (hy = w y', h = w), so the caller's prologue need not round them to double; out = [nf][6] =
 * {Sh, Ch, S, C, S2, C2}, S2 and C2 at the doubled phase 2 r (exact).
 * tests/test_gls_error_budget_host.py pins it to integer arithmetic on lattice inputs, at 4e3 and 4e6 cycles. */
void oracle_gls_sums_reduced(const double *t, const long double *hy, const long double *h, int64_t n,
                             const double *freq, int64_t nf, long double *out) {
    const long double two_pi = 2.0L * acosl(-1.0L);
    const double t0 = n > 0 ? t[0] : 0.0;
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < nf; ++j) {
        const double f = freq[j];
        long double a[6] = {0.0L, 0.0L, 0.0L, 0.0L, 0.0L, 0.0L};
        for (int64_t i = 0; i < n; ++i) {
            const double tp = t[i] - t0;
            const double p = f * tp;
            const double e = fma(f, tp, -p);
            const long double r = (long double)(p - rint(p)) + (long double)e;
            const long double x = two_pi * r;
            const long double s = sinl(x), c = cosl(x), s2 = sinl(x + x), c2 = cosl(x + x);
            a[0] += hy[i] * s;
            a[1] += hy[i] * c;
            a[2] += h[i] * s;
            a[3] += h[i] * c;
            a[4] += h[i] * s2;
            a[5] += h[i] * c2;
        }
        for (int q = 0; q < 6; ++q) out[j * 6 + q] = a[q];
    }
}

/* numpy's float remainder for a positive divisor of 1 (Python modulo, phase.py:131,
 * core.py:544): fmod, then shift negative results up by the divisor. */
static double mod1(double q) {
    double r = fmod(q, 1.0);
    if (r != 0.0) {
        if (r < 0.0) r += 1.0;
    } else {
        r = copysign(0.0, 1.0);
    }
    return r;
}

/* PDM._pdm (phase.py:128-149) for every period.  The argsort at :132-134 only permutes the
 * inputs of order-independent masks, so bins are filled in sample order; the variance is the
 * two-pass mean-centred form of np.var(ddof=1). */
void oracle_pdm_scan(const double *t, const double *x, int64_t n, const double *periods,
                     int64_t n_periods, int nb, int nc, double sigma, double *theta) {
    const int m0 = nb * nc;
#pragma omp parallel
    {
        double *phi = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
#pragma omp for schedule(dynamic, 4)
        for (int64_t p = 0; p < n_periods; ++p) {
            for (int64_t i = 0; i < n; ++i) phi[i] = mod1(t[i] / periods[p]);
            double num = 0.0;
            int64_t n_sum = 0, good = 0;
            for (int k = 0; k < m0; ++k) {
                const double lo = (double)k / m0, hi = (double)(k + nc) / m0;
                const double wrap = (double)(k - (m0 - nc)) / m0;
                int64_t cnt = 0;
                double mean = 0.0;
                for (int64_t i = 0; i < n; ++i)
                    if ((phi[i] >= lo && phi[i] < hi) || phi[i] < wrap) {
                        ++cnt;
                        mean += x[i];
                    }
                if (cnt > 1) {
                    mean /= (double)cnt;
                    double ss = 0.0;
                    for (int64_t i = 0; i < n; ++i)
                        if ((phi[i] >= lo && phi[i] < hi) || phi[i] < wrap) {
                            const double d = x[i] - mean;
                            ss += d * d;
                        }
                    num += ss; /* (n_j - 1) * s_j */
                    n_sum += cnt;
                    ++good;
                }
            }
            theta[p] = (num / (double)(n_sum - good)) / sigma;
        }
        free(phi);
    }
}

typedef struct {
    double phi, m;
    int64_t idx;
} sl_item;

static int sl_cmp(const void *a, const void *b) {
    const sl_item *x = (const sl_item *)a, *y = (const sl_item *)b;
    if (x->phi < y->phi) return -1;
    if (x->phi > y->phi) return 1;
    return (x->idx > y->idx) - (x->idx < y->idx); /* stable: ties keep time order */
}

/* StringLength._stringlength (phase.py:45-51) through TSeries.fold (core.py:543-544) and the
 * stable sort by phase of the TSeries constructor (core.py:473-477): closed polygon, closing
 * segment not phase-wrapped. */
void oracle_stringlength_scan(const double *t, const double *m, int64_t n, const double *periods,
                              int64_t n_periods, double *ell) {
#pragma omp parallel
    {
        sl_item *it = (sl_item *)malloc(sizeof(sl_item) * (size_t)(n > 0 ? n : 1));
#pragma omp for schedule(dynamic, 4)
        for (int64_t p = 0; p < n_periods; ++p) {
            for (int64_t i = 0; i < n; ++i) {
                it[i].phi = mod1((t[i] - 0.0) / periods[p]);
                it[i].m = m[i];
                it[i].idx = i;
            }
            qsort(it, (size_t)n, sizeof(sl_item), sl_cmp);
            double sum = 0.0;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t k = (i + 1 == n) ? 0 : i + 1;
                sum += hypot(it[k].m - it[i].m, it[k].phi - it[i].phi);
            }
            ell[p] = sum;
        }
        free(it);
    }
}

/* ------------------------------------------------------------------------------------------------------------
 * Double-precision direct sums for EXHAUSTIVE parity at the BASELINE sizes (1e11 ... 1e12 pairs), where the
 * long-double evaluation above would take the better part of an hour.  Same definition (spectral.py:13-15:
 * S_j = sum_i h_i sin(2 pi f_j t_i), C_j with cos), evaluated pair by pair - no recurrence over frequencies or
 * samples, nothing shared with the device kernel's rotation scheme:
 *   phase in CYCLES  p = f t  with its rounding error recovered exactly, e = fma(f, t, -p); k = nearest integer
 *   (p - k is exact), r = (p - k) + e in [-1/2, 1/2] carries ONE rounding (the long-double path rounds a phase of
 *   up to 1e6 rad to 64 bits: this is the tighter of the two at large phases);
 *   quadrant n = round(4 r), z = r - n/4 (exact), a = 2 pi z in [-pi/4, pi/4] with 2 pi split in two doubles;
 *   sin a, cos a from the Cephes double-precision minimax polynomials for that interval (S. Moshier, sin.c:
 *   sincof / coscof, |error| < 1.1e-16), put back in their quadrant by swaps and sign flips;
 *   sin / cos of the doubled frequency by the double-angle identities on those two values (one more rounding
 *   each; a second reduction of 2p bought nothing measurable and cost 40 % of the run time).
 * Sums: blocks of 512 samples in double (SIMD lanes, `omp simd reduction`), blocks added in long double.
 * tests/test_oracle_golden.py pins it to oracle_trig_sums_exact (<= 1e-13 of sum |h|); the GPU suite re-proves
 * that on the sampled bins of each full-size config before it trusts it on all of them.
 * ---------------------------------------------------------------------------------------------------------- */
#define ORACLE_CLONES __attribute__((target_clones("avx512f", "fma", "default")))

static inline void sincos_cycles(double p, double e, double *s_out, double *c_out) {
    const double big = 6755399441055744.0; /* 1.5 * 2^52: adding and subtracting rounds to nearest integer */
    const double k = (p + big) - big;
    const double r = (p - k) + e;
    const double n4 = (4.0 * r + big) - big;
    const double z = r - 0.25 * n4;
    const double two_pi_hi = 6.283185307179586, two_pi_lo = 2.4492935982947064e-16;
    const double a = fma(z, two_pi_lo, z * two_pi_hi);
    const double zz = a * a;
    double ps = 1.58962301576546568060E-10;
    ps = ps * zz + -2.50507477628578072866E-8;
    ps = ps * zz + 2.75573136213857245213E-6;
    ps = ps * zz + -1.98412698295895385996E-4;
    ps = ps * zz + 8.33333333332211858878E-3;
    ps = ps * zz + -1.66666666666666307295E-1;
    const double sz = a + a * zz * ps;
    double pc = -1.13585365213876817300E-11;
    pc = pc * zz + 2.08757008419747316778E-9;
    pc = pc * zz + -2.75573141792967388112E-7;
    pc = pc * zz + 2.48015872888517045348E-5;
    pc = pc * zz + -1.38888888888730564116E-3;
    pc = pc * zz + 4.16666666666665929218E-2;
    const double cz = 1.0 - 0.5 * zz + zz * zz * pc;
    const double an = fabs(n4);
    const int swap = an == 1.0;
    const double s = swap ? cz : sz, c = swap ? sz : cz;
    *s_out = (n4 < -0.5 || an > 1.5) ? -s : s;
    *c_out = (n4 > 0.5 || n4 < -1.5) ? -c : c;
}

/* six sums of one frequency over a run of samples, ADDED to `acc`: (hy, h) at f and h at 2 f. */
ORACLE_CLONES
void oracle_gls_sums_f64_acc(const double *t, const double *hy, const double *h, int64_t n, double f,
                             long double *acc /* Sh Ch S C S2 C2 */) {
    for (int64_t b = 0; b < n; b += 512) {
        const int64_t m = (n - b < 512) ? n - b : 512;
        const double *tb = t + b, *hb = h + b, *yb = hy + b;
        double sh = 0, ch = 0, s1 = 0, c1 = 0, s2 = 0, c2 = 0;
#pragma omp simd reduction(+ : sh, ch, s1, c1, s2, c2)
        for (int64_t i = 0; i < m; ++i) {
            const double p = f * tb[i];
            const double e = fma(f, tb[i], -p);
            double s, c;
            sincos_cycles(p, e, &s, &c);
            const double sd = 2.0 * s * c, cd = (c - s) * (c + s); /* doubled frequency: exact identities, 1 ulp */
            sh += yb[i] * s;
            ch += yb[i] * c;
            s1 += hb[i] * s;
            c1 += hb[i] * c;
            s2 += hb[i] * sd;
            c2 += hb[i] * cd;
        }
        acc[0] += sh; acc[1] += ch; acc[2] += s1; acc[3] += c1; acc[4] += s2; acc[5] += c2;
    }
}

/* The grid is handed over as the doubles the caller scans (np.arange's own values or f0 + delta j), like
 * oracle_trig_sums_exact.  Tiles of 32 frequencies walk the samples in runs of 4096 (a run stays in the core's
 * L2 while the tile's frequencies pass over it); a frequency's additions happen in sample order whatever the
 * tiling, so the result does not depend on it or on the thread count. */
void oracle_gls_sums_f64(const double *t, const double *hy, const double *h, int64_t n, const double *freq,
                         int64_t nf, double *Sh, double *Ch, double *S, double *C, double *S2, double *C2) {
    enum { TILE = 32, RUN = 4096 };
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t j0 = 0; j0 < nf; j0 += TILE) {
        const int64_t nj = (nf - j0 < TILE) ? nf - j0 : TILE;
        long double acc[TILE][6];
        memset(acc, 0, sizeof acc);
        for (int64_t b = 0; b < n; b += RUN) {
            const int64_t m = (n - b < RUN) ? n - b : RUN;
            for (int64_t j = 0; j < nj; ++j)
                oracle_gls_sums_f64_acc(t + b, hy + b, h + b, m, freq[j0 + j], acc[j]);
        }
        for (int64_t j = 0; j < nj; ++j) {
            Sh[j0 + j] = (double)acc[j][0]; Ch[j0 + j] = (double)acc[j][1];
            S[j0 + j] = (double)acc[j][2];  C[j0 + j] = (double)acc[j][3];
            S2[j0 + j] = (double)acc[j][4]; C2[j0 + j] = (double)acc[j][5];
        }
    }
}

/* A batch of curves on one grid (C3: 4096 x 2000 samples x 5e4 frequencies): curve b owns samples
 * [offsets[b], offsets[b+1]); the six sums land in rows of nf.  One parallel region over (curve, tile) - a
 * 2000-sample curve is far too little work to spread over 256 threads by itself. */
void oracle_gls_sums_f64_batch(const double *t, const double *hy, const double *h, const int64_t *offsets,
                               int64_t n_curves, const double *freq, int64_t nf, double *Sh, double *Ch, double *S,
                               double *C, double *S2, double *C2) {
    enum { TILE = 32, RUN = 4096 };
    const int64_t tiles = (nf + TILE - 1) / TILE;
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t work = 0; work < n_curves * tiles; ++work) {
        const int64_t b = work / tiles, j0 = (work % tiles) * TILE;
        const int64_t nj = (nf - j0 < TILE) ? nf - j0 : TILE;
        const int64_t lo = offsets[b], n = offsets[b + 1] - offsets[b];
        long double acc[TILE][6];
        memset(acc, 0, sizeof acc);
        for (int64_t r = 0; r < n; r += RUN) {
            const int64_t m = (n - r < RUN) ? n - r : RUN;
            for (int64_t j = 0; j < nj; ++j)
                oracle_gls_sums_f64_acc(t + lo + r, hy + lo + r, h + lo + r, m, freq[j0 + j], acc[j]);
        }
        for (int64_t j = 0; j < nj; ++j) {
            const int64_t o = b * nf + j0 + j;
            Sh[o] = (double)acc[j][0]; Ch[o] = (double)acc[j][1];
            S[o] = (double)acc[j][2];  C[o] = (double)acc[j][3];
            S2[o] = (double)acc[j][4]; C2[o] = (double)acc[j][5];
        }
    }
}

/* ------------------------------------------------------------------------------------------------------------
 * The scans the reference only names (phase.py:11-15, TODO upstream: PARITY UNPINNED BY THE REFERENCE) in C, for
 * whole BASELINE-size period grids: literal restatements of scan_oracle.py's aov_theta / cond_entropy /
 * gl_log_s (the published formulas), checked against them in tests/test_oracle_golden.py.
 * ---------------------------------------------------------------------------------------------------------- */
double lgamma_r(double, int *);

/* scan_oracle.py:_phase_bins - searchsorted(arange(r + 1) / r, phi, "right") - 1, phi == 1.0 joins the last
 * bin, NaN belongs to none. */
static int phase_bin(double t, double period, int r) {
    const double phi = mod1(t / period);
    if (phi != phi) return -1;
    int g = (int)(phi * r);
    if (g > r - 1) g = r - 1;
    if (g < 0) g = 0;
    while (g > 0 && phi < (double)g / r) --g;
    while (g + 1 <= r - 1 && phi >= (double)(g + 1) / r) ++g;
    return g;
}

/* Schwarzenberg-Czerny 1989, eq. 1-3 (scan_oracle.py:aov_theta): two passes, bin means then residuals. */
void oracle_aov_scan(const double *t, const double *x, int64_t n, const double *periods, int64_t n_periods,
                     int n_bins, double *theta) {
#pragma omp parallel
    {
        int *k = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
        double *sum = (double *)malloc(sizeof(double) * (size_t)n_bins);
        int64_t *cnt = (int64_t *)malloc(sizeof(int64_t) * (size_t)n_bins);
#pragma omp for schedule(dynamic, 4)
        for (int64_t p = 0; p < n_periods; ++p) {
            int64_t ok = 0;
            long double total = 0.0L;
            for (int b = 0; b < n_bins; ++b) { sum[b] = 0.0; cnt[b] = 0; }
            for (int64_t i = 0; i < n; ++i) {
                k[i] = phase_bin(t[i], periods[p], n_bins);
                if (k[i] >= 0) { ++ok; total += x[i]; sum[k[i]] += x[i]; ++cnt[k[i]]; }
            }
            if (ok <= n_bins || n_bins < 2) { theta[p] = NAN; continue; }
            const double xbar = (double)(total / (long double)ok);
            double between = 0.0;
            for (int b = 0; b < n_bins; ++b)
                if (cnt[b]) {
                    sum[b] /= (double)cnt[b]; /* now the bin mean */
                    between += (double)cnt[b] * (sum[b] - xbar) * (sum[b] - xbar);
                }
            long double within = 0.0L;
            for (int64_t i = 0; i < n; ++i)
                if (k[i] >= 0) { const double d = x[i] - sum[k[i]]; within += d * d; }
            theta[p] = (between / (n_bins - 1)) / ((double)within / (double)(ok - n_bins));
        }
        free(k); free(sum); free(cnt);
    }
}

/* Graham et al. 2013, eq. 1 (scan_oracle.py:cond_entropy): H_c = sum p(m, phi) ln(p(phi) / p(m, phi)). */
void oracle_cond_entropy_scan(const double *t, const double *mag_bin, int64_t n, const double *periods,
                              int64_t n_periods, int n_phase, int n_mag, double *h) {
#pragma omp parallel
    {
        int64_t *cells = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n_phase * n_mag));
#pragma omp for schedule(dynamic, 4)
        for (int64_t p = 0; p < n_periods; ++p) {
            memset(cells, 0, sizeof(int64_t) * (size_t)(n_phase * n_mag));
            int64_t ok = 0;
            for (int64_t i = 0; i < n; ++i) {
                const int k = phase_bin(t[i], periods[p], n_phase);
                if (k >= 0) { ++ok; ++cells[k * n_mag + (int)mag_bin[i]]; }
            }
            if (ok == 0) { h[p] = NAN; continue; }
            double acc = 0.0;
            for (int k = 0; k < n_phase; ++k) {
                int64_t row = 0;
                for (int m = 0; m < n_mag; ++m) row += cells[k * n_mag + m];
                for (int m = 0; m < n_mag; ++m) {
                    const int64_t c = cells[k * n_mag + m];
                    if (c > 0) acc += (double)c / (double)ok * log((double)row / (double)c);
                }
            }
            h[p] = acc;
        }
        free(cells);
    }
}

/* Gregory & Loredo 1992, eq. 5.13-5.14 averaged over the bin offset (scan_oracle.py:gl_log_s). */
void oracle_gl_scan(const double *t, int64_t n, const double *periods, int64_t n_periods, int m, int n_offsets,
                    double *log_s) {
    const int fine = m * n_offsets;
#pragma omp parallel
    {
        int64_t *counts = (int64_t *)malloc(sizeof(int64_t) * (size_t)fine);
        double *terms = (double *)malloc(sizeof(double) * (size_t)n_offsets);
        int sign;
#pragma omp for schedule(dynamic, 4)
        for (int64_t p = 0; p < n_periods; ++p) {
            memset(counts, 0, sizeof(int64_t) * (size_t)fine);
            int64_t ok = 0;
            for (int64_t i = 0; i < n; ++i) {
                const int k = phase_bin(t[i], periods[p], fine);
                if (k >= 0) { ++ok; ++counts[k]; }
            }
            if (ok == 0) { log_s[p] = NAN; continue; }
            double top = -INFINITY;
            for (int off = 0; off < n_offsets; ++off) {
                double lg = 0.0;
                for (int b = 0; b < m; ++b) {
                    int64_t per_bin = 0;
                    for (int q = 0; q < n_offsets; ++q) per_bin += counts[(b * n_offsets + q + off) % fine];
                    lg += lgamma_r((double)per_bin + 1.0, &sign);
                }
                terms[off] = (double)ok * log((double)m) + lg - lgamma_r((double)ok + 1.0, &sign);
                if (terms[off] > top) top = terms[off];
            }
            double s = 0.0;
            for (int off = 0; off < n_offsets; ++off) s += exp(terms[off] - top);
            log_s[p] = top + log(s / n_offsets);
        }
        free(counts); free(terms);
    }
}

/* ------------------------------------------------------------------------------------------------------------
 * Supersmoother period search (scan_oracle.py: ss_smooth / supersmoother / supersmoother_stat; Friedman 1984
 * `supsmu` + `smooth`, periodic, unit weights; Reimann 1994) - the numpy oracle restated operation by operation in
 * the same 80-bit type, for whole period grids: 0.4 s a period at 5e4 samples in numpy, one thread.  The reference
 * has no Supersmoother.  Pinned to the numpy form in tests/test_oracle_golden.py.
 * ---------------------------------------------------------------------------------------------------------- */
static const double kSsSpans[3] = {0.05, 0.2, 0.5};

/* numpy's add.reduce over a contiguous double array (pairwise, blocks of 128, eight partial sums): the sums of
 * ss_average_ties and the final mean are taken with it, so that long tied runs round as they do there. */
static double np_pairwise_sum(const double *a, int64_t n) {
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        int64_t i;
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        for (i = 8; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

static int64_t ss_half_width(int64_t n, double span) {
    const int64_t ibw = (int64_t)(0.5 * span * (double)n + 0.5);
    return ibw > 2 ? ibw : 2;
}

/* `smooth`, label 90-110 */
static void ss_average_ties(const double *x, double *smo, int64_t n) {
    int64_t j = 0;
    while (j < n) {
        const int64_t j0 = j;
        while (j + 1 < n && x[j + 1] <= x[j]) ++j;
        if (j > j0) {
            const double mean = np_pairwise_sum(smo + j0, j - j0 + 1) / (double)(j - j0 + 1);
            for (int64_t i = j0; i <= j; ++i) smo[i] = mean;
        }
        ++j;
    }
}

typedef struct {
    long double *xc, *cx, *cxx, *cy, *cxy; /* n, then four prefix arrays of n + 1 */
} ss_work;

static int ss_work_alloc(ss_work *w, int64_t n) {
    const size_t m = (size_t)(n > 0 ? n : 1) + 1;
    w->xc = (long double *)malloc(sizeof(long double) * m * 5);
    if (!w->xc) return 0;
    w->cx = w->xc + m;
    w->cxx = w->cx + m;
    w->cy = w->cxx + m;
    w->cxy = w->cy + m;
    return 1;
}

/* abscissae relative to x[n / 2] and their two prefix sums: the same for every smooth of one folded curve */
static void ss_prefix_x(ss_work *w, const double *x, int64_t n) {
    w->cx[0] = w->cxx[0] = 0.0L;
    for (int64_t i = 0; i < n; ++i) {
        w->xc[i] = (long double)(x[i] - x[n / 2]);
        w->cx[i + 1] = w->cx[i] + w->xc[i];
        w->cxx[i + 1] = w->cxx[i] + w->xc[i] * w->xc[i];
    }
}

/* scan_oracle.ss_smooth, statement by statement; `smo` and `acvr` must not alias `y` */
static void ss_smooth_core(ss_work *w, const double *x, const double *y, int64_t n, double span, double vsmlsq, int cv,
                           double *smo, double *acvr) {
    const int64_t ibw = ss_half_width(n, span);
    const long double *xc = w->xc, *cx = w->cx, *cxx = w->cxx;
    long double *cy = w->cy, *cxy = w->cxy;
    cy[0] = cxy[0] = 0.0L;
    for (int64_t i = 0; i < n; ++i) {
        const long double yl = (long double)y[i];
        cy[i + 1] = cy[i] + yl;
        cxy[i + 1] = cxy[i] + xc[i] * yl;
    }
    const long double fbw = (long double)(2 * ibw + 1), v = (long double)vsmlsq;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t lo = j - ibw, hi = j + ibw + 1;
        const int low = lo < 0, high = hi > n;
        const int64_t wl = low ? n + lo : 0, wh = low ? n : (high ? hi - n : 0);
        const long double sh = low ? -1.0L : (high ? 1.0L : 0.0L), cw = (long double)(wh - wl);
        const int64_t lo_c = lo > 0 ? lo : 0, hi_c = hi < n ? hi : n;
        const long double mx = cx[hi_c] - cx[lo_c], ux = cx[wh] - cx[wl];
        const long double mxx = cxx[hi_c] - cxx[lo_c], uxx = cxx[wh] - cxx[wl];
        const long double my = cy[hi_c] - cy[lo_c], uy = cy[wh] - cy[wl];
        const long double mxy = cxy[hi_c] - cxy[lo_c], uxy = cxy[wh] - cxy[wl];
        const long double sx = mx + (ux + sh * cw), sxx = mxx + (uxx + 2.0L * sh * ux + cw);
        const long double sy = my + uy, sxy = mxy + (uxy + sh * uy);
        const long double xm = sx / fbw, ym = sy / fbw;
        const long double var = sxx - fbw * xm * xm, cvar = sxy - fbw * xm * ym;
        const long double a = var > v ? cvar / var : 0.0L;
        const long double s = a * (xc[j] - xm) + ym;
        smo[j] = (double)s;
        if (cv) {
            const long double d = xc[j] - xm;
            const long double h = 1.0L / fbw + (var > v ? d * d / var : 0.0L);
            const long double a1 = 1.0L - h;
            if (a1 > 0.0L)
                acvr[j] = (double)(fabsl((long double)y[j] - s) / a1);
            else
                acvr[j] = j > 0 ? acvr[j - 1] : 0.0; /* `smooth`, label 70: carried over from the point before */
        } else if (acvr) {
            acvr[j] = 0.0;
        }
    }
    ss_average_ties(x, smo, n);
}

/* returns 0, or -1 when the window of 2 ibw + 1 points does not fit (scan_oracle.ss_smooth raises) */
int oracle_ss_smooth(const double *x, const double *y, int64_t n, double span, double vsmlsq, int cv, double *smo,
                     double *acvr) {
    if (n < 1 || 2 * ss_half_width(n, span) + 1 > n) return -1;
    ss_work w;
    if (!ss_work_alloc(&w, n)) return -2;
    ss_prefix_x(&w, x, n);
    ss_smooth_core(&w, x, y, n, span, vsmlsq, cv, smo, acvr);
    free(w.xc);
    return 0;
}

/* scan_oracle.supersmoother on a sorted folded curve; buf holds 9 arrays of n doubles; the fit lands in buf[0 .. n) */
static void ss_supsmu(ss_work *w, const double *x, const double *y, int64_t n, double alpha, double *buf) {
    double *out = buf, *sm[3] = {buf + n, buf + 2 * n, buf + 3 * n}, *res[3] = {buf + 4 * n, buf + 5 * n, buf + 6 * n};
    double *acvr = buf + 7 * n, *tmp = buf + 8 * n;
    int64_t i = n / 4, j = 3 * (n / 4); /* 1-based in the Fortran: x(i), x(j) */
    double scale = x[j - 1] - x[(i > 1 ? i : 1) - 1];
    while (scale <= 0.0) { /* `supsmu`, label 30 */
        if (j < n) ++j;
        if (i > 1) --i;
        if (j >= n && i <= 1) break;
        scale = x[j - 1] - x[i - 1];
    }
    const double e = 1.0e-3 * scale, vsmlsq = e * e;
    ss_prefix_x(w, x, n);
    for (int k = 0; k < 3; ++k) {
        ss_smooth_core(w, x, y, n, kSsSpans[k], vsmlsq, 1, sm[k], acvr);
        ss_smooth_core(w, x, acvr, n, kSsSpans[1], vsmlsq, 0, res[k], NULL);
    }
    const int bass = alpha > 0.0 && alpha <= 10.0;
    for (int64_t q = 0; q < n; ++q) {
        int best = 0; /* first minimum: `if (sc(j,2i) < resmin)` */
        for (int k = 1; k < 3; ++k)
            if (res[k][q] < res[best][q]) best = k;
        const double resmin = res[best][q];
        double span = kSsSpans[best];
        if (bass && resmin < res[2][q] && resmin > 0.0) { /* R's guard: see scan_oracle.supersmoother */
            double ratio = resmin / res[2][q];
            if (ratio < 1.0e-7) ratio = 1.0e-7;
            span = span + (kSsSpans[2] - span) * pow(ratio, 10.0 - alpha);
        }
        tmp[q] = span;
    }
    ss_smooth_core(w, x, tmp, n, kSsSpans[1], vsmlsq, 0, acvr, NULL); /* acvr: the smoothed spans */
    for (int64_t q = 0; q < n; ++q) {
        double s = acvr[q];
        s = s < kSsSpans[0] ? kSsSpans[0] : (s > kSsSpans[2] ? kSsSpans[2] : s);
        const double f = s - kSsSpans[1];
        if (f >= 0.0) {
            const double fu = f / (kSsSpans[2] - kSsSpans[1]);
            tmp[q] = (1.0 - fu) * sm[1][q] + fu * sm[2][q];
        } else {
            const double fd = -f / (kSsSpans[1] - kSsSpans[0]);
            tmp[q] = (1.0 - fd) * sm[1][q] + fd * sm[0][q];
        }
    }
    ss_smooth_core(w, x, tmp, n, kSsSpans[0], vsmlsq, 0, out, NULL);
}

/* scan_oracle.supersmoother_scan: fold and stable sort as for StringLength, `supsmu`, mean absolute residual.
 * n < 5 (no room for the woofer window) gives NaN. */
void oracle_supersmoother_scan(const double *t, const double *y, int64_t n, const double *periods, int64_t n_periods,
                               double alpha, double *out) {
    if (n < 5) {
        for (int64_t p = 0; p < n_periods; ++p) out[p] = NAN;
        return;
    }
#pragma omp parallel
    {
        sl_item *it = (sl_item *)malloc(sizeof(sl_item) * (size_t)n);
        double *xs = (double *)malloc(sizeof(double) * (size_t)n * 11), *ys = xs + n, *buf = ys + n;
        ss_work w;
        const int ok = ss_work_alloc(&w, n) && it && xs;
#pragma omp for schedule(dynamic, 1)
        for (int64_t p = 0; p < n_periods; ++p) {
            if (!ok) { out[p] = NAN; continue; }
            for (int64_t i = 0; i < n; ++i) {
                it[i].phi = mod1((t[i] - 0.0) / periods[p]);
                it[i].m = y[i];
                it[i].idx = i;
            }
            qsort(it, (size_t)n, sizeof(sl_item), sl_cmp);
            for (int64_t i = 0; i < n; ++i) { xs[i] = it[i].phi; ys[i] = it[i].m; }
            ss_supsmu(&w, xs, ys, n, alpha, buf);
            for (int64_t i = 0; i < n; ++i) buf[n + i] = fabs(ys[i] - buf[i]);
            out[p] = np_pairwise_sum(buf + n, n) / (double)n;
        }
        free(it); free(xs); free(w.xc);
    }
}
