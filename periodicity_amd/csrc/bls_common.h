// Shared by bls.hip and bls_ragged.hip (inside an anonymous namespace of each, after pdc_internal.h, gls_sums.h,
// <climits> and <cmath>): the limits and their check, the prologue's body, the fixed-point record, the LDS layout of a
// workgroup's histogram, the binning loop, the box search and the write of one period's result.  What a kernel of
// either unit computes for a curve and a trial period is this text, so the single call and the batch give the same
// bits.
#pragma once

constexpr int kBlock = 256;
constexpr int kPrepBlock = 1024;
constexpr int kMaxBins = 2048;
constexpr int kMaxSlices = 1024;
constexpr double kScale = 1152921504606846976.0;   // 2^60

struct BlsRec {
    double t;
    long long qw, qs;
};

struct BlsArgs {
    const BlsRec *rec;
    const double *scal;
    int64_t n, z_len;   // z_len: samples per slice
    const double *periods;
    int n_bins, len_min, len_max, min_points, dips_only;
    unsigned long long *gr, *gs;   // [n_periods][n_bins]       (slices > 1)
    unsigned *gc;                  // [n_periods][n_bins + 1]
    double *power, *depth;         // depth, start_bin, box_bins may be NULL
    int32_t *start_bin, *box_bins;
};

template <int BLOCK>
__device__ __forceinline__ double block_max(double v, double *lds_waves) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_down(v, o, 64);
        v = u > v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds_waves[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = lds_waves[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) r = lds_waves[w] > r ? lds_waves[w] : r;
    return r;
}

// ---- prologue: weights and centring as GLS takes them, then the fixed-point records -----------------------------------
// Run by one workgroup of kPrepBlock threads on one curve: rec [n], scal = {YY, A, max |t|, bad}.
__device__ __forceinline__ void bls_prep_body(const double *t, const double *y, const double *dy, const int64_t n, BlsRec *rec,
                                              double *scal) {
    __shared__ double red[kPrepBlock / 64];
    const int tid = threadIdx.x;
    double acc = 0.0, nbad = 0.0, tmax = 0.0;
    for (int64_t i = tid; i < n; i += kPrepBlock) {
        const double e = dy ? dy[i] : 1.0, at = __builtin_fabs(t[i]);
        const double iv = 1.0 / (e * e);
        acc += iv;
        const bool ok = at < HUGE_VAL && __builtin_fabs(y[i]) < HUGE_VAL && __builtin_fabs(e) < HUGE_VAL && e != 0.0 && iv < HUGE_VAL;
        nbad += ok ? 0.0 : 1.0;
        tmax = at > tmax ? at : tmax;
    }
    const double W = block_sum<kPrepBlock>(acc, red);
    nbad = block_sum<kPrepBlock>(nbad, red);
    tmax = block_max<kPrepBlock>(tmax, red);
    if (nbad != 0.0 || !(W > 0.0) || !(W < HUGE_VAL)) {   // (also n == 0) every output is NaN / -1: no record is read
        if (tid == 0) {
            scal[0] = __builtin_nan("");
            scal[1] = scal[2] = 0.0;
            scal[3] = 1.0;
        }
        return;
    }
    acc = 0.0;
    for (int64_t i = tid; i < n; i += kPrepBlock) {
        acc += inv_var(dy, i) / W * y[i];
    }
    const double ybar = block_sum<kPrepBlock>(acc, red);
    double amax = 0.0;
    for (int64_t i = tid; i < n; i += kPrepBlock) {
        const double d = __builtin_fabs(y[i] - ybar);
        amax = d > amax ? d : amax;
    }
    const double A = block_max<kPrepBlock>(amax, red);
    double yy = 0.0;
    for (int64_t i = tid; i < n; i += kPrepBlock) {
        const double w = inv_var(dy, i) / W;
        const double yc = y[i] - ybar;
        yy += (w * yc) * yc;
        BlsRec r;
        r.t = t[i];
        r.qw = __builtin_llrint(w * kScale);
        r.qs = A > 0.0 ? __builtin_llrint(w * (yc / A) * kScale) : 0;
        rec[i] = r;
    }
    yy = block_sum<kPrepBlock>(yy, red);
    if (tid == 0) {
        scal[0] = yy;
        scal[1] = A;
        scal[2] = tmax;
        scal[3] = (yy > 0.0 && yy < HUGE_VAL && A > 0.0 && A < HUGE_VAL) ? 0.0 : 1.0;   // a constant y has no periodogram
    }
}

__device__ __forceinline__ void bls_write(const BlsArgs &a, int64_t p, double power, double depth, int start, int len) {
    a.power[p] = power;
    if (a.depth) a.depth[p] = depth;
    if (a.start_bin) a.start_bin[p] = start;
    if (a.box_bins) a.box_bins[p] = len;
}

// LDS of a workgroup: the histogram hr | hs [n_bins], hc [n_bins + 1] (the extra counter: samples whose phase is NaN),
// and - where the workgroup searches - the prefix sums pr | ps | pc [n_bins + len_max + 1].
struct BlsLds {
    long long *hr, *hs, *pr, *ps;
    unsigned *hc, *pc;
};
__device__ __forceinline__ BlsLds bls_lds(unsigned char *raw, int nb, int len_max, bool search) {
    const int m1 = search ? nb + len_max + 1 : 0;
    BlsLds l;
    l.hr = reinterpret_cast<long long *>(raw);
    l.hs = l.hr + nb;
    l.pr = l.hs + nb;
    l.ps = l.pr + m1;
    l.hc = reinterpret_cast<unsigned *>(l.ps + m1);
    l.pc = l.hc + nb + 1;
    return l;
}
size_t bls_lds_bytes(int nb, int len_max, bool search) {
    const size_t m1 = search ? (size_t)nb + len_max + 1 : 0;
    return (size_t)nb * 16 + m1 * 16 + ((size_t)nb + 1) * 4 + m1 * 4;
}
constexpr int kMaxLds = kMaxBins * 16 + 4096 * 16 + (kMaxBins + 1) * 4 + 4096 * 4;   // 122 884 B of the CU's 160 KiB

// ---- the search: run by the NT threads of a workgroup on the histogram of trial period p in LDS ---------------------
template <int NT>
__device__ void bls_search(const BlsArgs &a, const int64_t p, const BlsLds &l) {
    __shared__ long long w_r[NT / 64], w_s[NT / 64];
    __shared__ unsigned w_c[NT / 64];
    __shared__ double b_v[NT / 64];
    __shared__ int b_k[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nb = a.n_bins;
    if (l.hc[nb] != 0u) {   // a NaN phase (period 0 or NaN): this period only
        if (tid == 0) bls_write(a, p, __builtin_nan(""), __builtin_nan(""), -1, -1);
        return;
    }
    // prefix sums of the histogram extended by len_max wrap-around bins: thread `tid` owns a run of `chunk` entries
    const int M = nb + a.len_max, chunk = (M + NT - 1) / NT;
    const int b = tid * chunk < M ? tid * chunk : M, e = b + chunk < M ? b + chunk : M;
    long long ar = 0, as = 0;
    unsigned ac = 0u;
    for (int k = b; k < e; ++k) {
        const int j = k < nb ? k : k - nb;
        ar += l.hr[j];
        as += l.hs[j];
        ac += l.hc[j];
    }
    long long ir = ar, is = as;
    unsigned ic = ac;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long ur = __shfl_up(ir, o, 64), us = __shfl_up(is, o, 64);
        const unsigned uc = __shfl_up(ic, o, 64);
        if (lane >= o) {
            ir += ur;
            is += us;
            ic += uc;
        }
    }
    if (lane == 63) {
        w_r[wv] = ir;
        w_s[wv] = is;
        w_c[wv] = ic;
    }
    __syncthreads();
    long long run_r = ir - ar, run_s = is - as;
    unsigned run_c = ic - ac;
    for (int w = 0; w < wv; ++w) {
        run_r += w_r[w];
        run_s += w_s[w];
        run_c += w_c[w];
    }
    if (tid == 0) {
        l.pr[0] = 0;
        l.ps[0] = 0;
        l.pc[0] = 0u;
    }
    for (int k = b; k < e; ++k) {
        const int j = k < nb ? k : k - nb;
        run_r += l.hr[j];
        run_s += l.hs[j];
        run_c += l.hc[j];
        l.pr[k + 1] = run_r;
        l.ps[k + 1] = run_s;
        l.pc[k + 1] = run_c;
    }
    __syncthreads();

    // the windows: thread `tid` takes the start bins tid, tid + NT, ... at every length
    const long long r_total = l.pr[nb], n_total = (long long)l.pc[nb], min_points = a.min_points;
    double best = -1.0;
    int key = INT_MAX;   // L * 4096 + i of `best`: among equal SR the smaller L, then the smaller i
    for (int i = tid; i < nb; i += NT) {
        const long long r0 = l.pr[i], s0 = l.ps[i];
        const unsigned c0 = l.pc[i];
        for (int L = a.len_min; L <= a.len_max; ++L) {
            const long long R = l.pr[i + L] - r0, S = l.ps[i + L] - s0, c = (long long)(unsigned)(l.pc[i + L] - c0);
            const long long Rc = r_total - R;   // 1 - r, from the integers
            if (c >= min_points && n_total - c >= min_points && R > 0 && Rc > 0 && (!a.dips_only || S < 0)) {
                const double sd = (double)S;
                const double v = sd * sd / ((double)R * (double)Rc);
                const int k = L * 4096 + i;
                if (v > best || (v == best && k < key)) {
                    best = v;
                    key = k;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(best, o, 64);
        const int ok = __shfl_down(key, o, 64);
        if (ov > best || (ov == best && ok < key)) {
            best = ov;
            key = ok;
        }
    }
    if (lane == 0) {
        b_v[wv] = best;
        b_k[wv] = key;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < NT / 64; ++w)
        if (b_v[w] > best || (b_v[w] == best && b_k[w] < key)) {
            best = b_v[w];
            key = b_k[w];
        }
    if (key == INT_MAX) {   // no admissible box
        bls_write(a, p, __builtin_nan(""), __builtin_nan(""), -1, -1);
        return;
    }
    const int L = key >> 12, i = key & 4095;
    const double YY = a.scal[0], A = a.scal[1];
    const long long R = l.pr[i + L] - l.pr[i], S = l.ps[i + L] - l.ps[i];
    const double sd = (double)S, den = (double)R * (double)(r_total - R);
    // s = A S 2^-60, r = R 2^-60, 1 - r = Rc 2^-60
    bls_write(a, p, (sd * sd / den) * (A * A) / YY, -A * (sd / den * kScale), i, L);
}

// ---- binning --------------------------------------------------------------------------------------------------------
// The kBlock threads of a workgroup clear its histogram ...
__device__ __forceinline__ void bls_clear(const BlsLds &l, const int nb) {
    const int tid = threadIdx.x;
    for (int k = tid; k < nb; k += kBlock) {
        l.hr[k] = 0;
        l.hs[k] = 0;
    }
    for (int k = tid; k <= nb; k += kBlock) l.hc[k] = 0u;
    __syncthreads();
}

// ... and bin the samples [s_begin, s_end) of `rec` at one trial period (lane = sample, three LDS atomic adds per
// sample); tmax = max |t| of the whole curve.
__device__ __forceinline__ void bls_bin(const BlsRec *rec, const double tmax, const double period, const int nb,
                                        const int64_t s_begin, const int64_t s_end, const BlsLds &l) {
    const int tid = threadIdx.x;
    const double rp = 1.0 / period, dm0 = (double)nb;
    // the fast path of pdm_chunks.inc: u = frac(t * rp) * n_bins against the exact ((t / period) % 1) and the edges
    // k / n_bins, in units of u: quotient error <= 1.5 ulp(q) <= 3.4e-16 |q|, product / edge roundings 2.3e-16 n_bins;
    // doubled for safety.  A bin is accepted only when u is provably that far from every integer.
    const double eps = dm0 * (8.9e-16 * tmax * __builtin_fabs(rp) + 8.9e-16);
    const double thr = 0.5 - eps;
    for (int64_t g = s_begin + tid; g < s_end; g += kBlock) {
        const BlsRec r = rec[g];
        const double u = __builtin_amdgcn_fract(r.t * rp) * dm0;
        int k = (int)u;
        if (!(__builtin_fabs(__builtin_amdgcn_fract(u) - 0.5) < thr)) {
            // exact path: numpy's float remainder of the IEEE quotient, explicit edges
            const double qe = r.t / period;
            const double phi = qe - __builtin_floor(qe);
            if (phi != phi) {   // poisons the period
                atomicAdd(&l.hc[nb], 1u);
                continue;
            }
            k = (int)(phi * dm0);
            k = k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);
            while (k > 0 && phi < (double)k / dm0) --k;
            while (k < nb - 1 && phi >= (double)(k + 1) / dm0) ++k;   // phi == 1.0 stays in the last bin
        }
        k = k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);   // (never taken: the index of an LDS atomic is kept in bounds anyway)
        atomicAdd(reinterpret_cast<unsigned long long *>(&l.hr[k]), (unsigned long long)r.qw);
        atomicAdd(reinterpret_cast<unsigned long long *>(&l.hs[k]), (unsigned long long)r.qs);
        atomicAdd(&l.hc[k], 1u);
    }
    __syncthreads();
}

// ---- host side: the limits of every entry ---------------------------------------------------------------------------
struct BlsParams {
    int n_bins, len_min, len_max, min_points, dips_only, slices;
};

int bls_validate(const char *what, int64_t n, int64_t n_periods, const BlsParams &q) {
    PDC_REQUIRE(n >= 0 && n_periods >= 0, "%s: negative size", what);
    PDC_REQUIRE(n < ((int64_t)1 << 31) && n_periods < ((int64_t)1 << 31), "%s: at most 2^31 - 1 samples and trial periods", what);
    PDC_REQUIRE(q.n_bins >= 2 && q.n_bins <= kMaxBins, "%s: n_bins must be 2 .. %d (got %d)", what, kMaxBins, q.n_bins);
    PDC_REQUIRE(q.len_min >= 1 && q.len_min <= q.len_max && q.len_max <= q.n_bins - 1,
                "%s: box lengths need 1 <= len_min <= len_max <= n_bins - 1 (got %d .. %d of %d bins)", what, q.len_min,
                q.len_max, q.n_bins);
    PDC_REQUIRE(q.min_points >= 1, "%s: min_points must be at least 1 (got %d)", what, q.min_points);
    PDC_REQUIRE(q.slices >= 0 && q.slices <= kMaxSlices, "%s: slices must be 0 (chosen from the shape) .. %d (got %d)", what,
                kMaxSlices, q.slices);
    return PDC_OK;
}
