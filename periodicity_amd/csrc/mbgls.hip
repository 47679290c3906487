// Shared-phase multiband generalised Lomb-Scargle (VanderPlas & Ivezic 2015, ApJ 812, 18: the Nbase = H, Nband = 0 model)
// as an exact direct summation on gfx950: per trial frequency the weighted least-squares fit of ONE Fourier series of H
// harmonics common to all bands plus one floating offset PER BAND, power = b^T M^-1 b / YY.
//
// The reference has no such class: PARITY UNPINNED BY THE REFERENCE.  Weights, grid and the two normalisations are
// those of GLS; the per-band centring is for conditioning only (the offsets still float).
//
// The band-band block of M is diagonal (W_b = sum of a band's weights), so the offsets are eliminated exactly: with
// v_b = the band's share of (C_h, S_h), h <= H, and Y_b = sum over the band of w yc,
//     M' = M_hh - sum_b v_b v_b^T / W_b,   b' = b_h - sum_b v_b Y_b / W_b,   q0 = sum_b Y_b^2 / W_b,
//     b^T M^-1 b = q0 + b'^T M'^-1 b'.
//
// Decomposition
//   mbgls_prep_kernel   one workgroup: weights, per-band W_b, mean, Y_b, YY, and the 48-byte records of put_record
//                       GROUPED BY BAND (input order kept inside a band) with the table of band starts.  Each of its 16
//                       waves walks a sixteenth of the samples 64 at a time, once per band; a ballot on `label == b`
//                       and a prefix popcount give each sample its place: no atomics, the same bits at every call, and
//                       a label never indexes memory.
//   mbgls_scan_kernel   the tile (xcd_tile) and one scan_stretch of gls_sums.h PER BAND (a band that ends
//                       mid-chunk ends its stretch); the 6 H sums per frequency run across all bands (the ladder of
//                       add_fourier_sums typed out: gls_sums.h, who uses what); at a band's end v_b is the difference to a snapshot of (C_h, S_h) taken
//                       at the previous boundary, and the rank-one updates above go into H (2H + 1) + 2H registers
//                       per frequency - none of it grows with the number of bands.  Epilogue: cholesky_quadratic over
//                       the 2H harmonic columns, its entries fourier_entry minus the rank-one terms.
// Without fit_mean there are no offsets and no centring: the labels are not read and the curve is one stretch - the sums
// of mhgls.hip with fit_mean = 0.
#include "pdc_internal.h"
#include "harmonic_sums.h"

#include <cmath>

using namespace pdc;

namespace {

constexpr int kBlock = 256;
constexpr int kPrepBlock = 1024;
constexpr int kPrepWaves = kPrepBlock / 64;
constexpr int kChunk = 64;   // samples per rotation-table chunk
constexpr int kMaxTerms = 3;
// The prologue keeps its per-band and per-(band, wave) tables in LDS (17 KB, sized for 32 bands) and walks the curve once per
// band and pass.  Nothing in the scan depends on the cap.
constexpr int kMaxBands = 32;

// the scalar block behind the records, in doubles (the band starts are int64)
constexpr int kScalYY = 0, kScalWsum = 1, kScalWerr = 2, kScalBad = 3, kScalWb = 4, kScalYb = kScalWb + kMaxBands,
              kScalStart = kScalYb + kMaxBands, kScalCount = kScalStart + kMaxBands + 1;

struct MbPrepArgs {
    const double *t, *y, *dy;
    const int32_t *band;   // NULL: one band (no fit_mean)
    int64_t n;
    int n_bands, fit_mean;
    double delta;
    double *rec;    // [n + 2][6] (the scan reads ahead)
    double *scal;   // [kScalCount]
};

struct MbArgs {
    const double *rec, *scal;
    int64_t n, tiles;
    double f0, delta;
    int64_t j_begin, nf;
    int n_bands, fit_mean, psd;
    double *power;
};

// ---- prologue -------------------------------------------------------------------------------------------------------
// Four 64-sample groups per trip of a wave, their labels loaded before anything is stored (the loads overlap).
constexpr int kPrepUnroll = 4;

__device__ __forceinline__ int label_at(const int32_t *band, int64_t i, int64_t n) {
    return i < n ? (band ? band[i] : 0) : -1;   // (-1 matches no band)
}

__global__ __launch_bounds__(kPrepBlock) void mbgls_prep_kernel(MbPrepArgs a) {
    // Wave s owns segment s of the input (a sixteenth of it, whole 64-sample groups) for EVERY band: item (b, s) is
    // one walk of that segment that looks at band b only, so the items of a band, taken in the order of s, see the
    // band's samples in input order, and every sum over items is taken in that fixed order.
    __shared__ double red[kPrepWaves];
    __shared__ double s_p[kMaxBands][kPrepWaves], s_q[kMaxBands][kPrepWaves];   // per item: two partial sums
    __shared__ long long s_cnt[kMaxBands][kPrepWaves], s_at[kMaxBands][kPrepWaves];
    __shared__ double s_wb[kMaxBands], s_ybar[kMaxBands], s_yy[kMaxBands];
    __shared__ long long s_held[kMaxBands], s_start[kMaxBands + 1];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = a.n;
    const int B = a.n_bands;

    // t_min (in order t[0]), sum err^-2, and whether any label is out of range
    if (tid == 0) s_bad = 0;
    double tmin = HUGE_VAL, acc = 0.0;
    bool bad = false;
    for (int64_t i = tid; i < n; i += kPrepBlock) {
        tmin = __builtin_fmin(tmin, a.t[i]);
        acc += inv_var(a.dy, i);
        if (a.band) bad = bad || (unsigned)a.band[i] >= (unsigned)B;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tmin = __builtin_fmin(tmin, __shfl_down(tmin, o, 64));
    __syncthreads();
    if (lane == 0) red[wave] = tmin;
    if (bad) s_bad = 1;
    __syncthreads();
    tmin = red[0];
#pragma unroll
    for (int w = 1; w < kPrepWaves; ++w) tmin = __builtin_fmin(tmin, red[w]);
    const double W = block_sum<kPrepBlock>(acc, red);

    const int64_t seg = (((n + kPrepWaves - 1) / kPrepWaves) + 63) & ~(int64_t)63;
    const int64_t lo = (int64_t)wave * seg < n ? (int64_t)wave * seg : n;
    const int64_t hi = lo + seg < n ? lo + seg : n;

    // pass 1: per item its samples, sum w and sum w y
    for (int b = 0; b < B; ++b) {
        long long cnt = 0;
        double wsum = 0.0, wy = 0.0;
        for (int64_t base = lo; base < hi; base += 64 * kPrepUnroll) {
            int lbl[kPrepUnroll];
#pragma unroll
            for (int u = 0; u < kPrepUnroll; ++u) lbl[u] = label_at(a.band, base + u * 64 + lane, hi);
#pragma unroll
            for (int u = 0; u < kPrepUnroll; ++u) {
                const int64_t i = base + u * 64 + lane;
                const bool mine = lbl[u] == b;
                if (mine) {
                    const double w = inv_var(a.dy, i) / W;
                    wsum += w;
                    wy += w * a.y[i];
                }
                cnt += __popcll(__ballot(mine));
            }
        }
        wsum = wave_sum(wsum);
        wy = wave_sum(wy);
        if (lane == 0) {
            s_cnt[b][wave] = cnt;
            s_p[b][wave] = wsum;
            s_q[b][wave] = wy;
        }
    }
    __syncthreads();
    if (tid < B) {   // the band's items in order: its samples, W_b, its weighted mean, each item's place inside the band
        long long held = 0;
        double wsum = 0.0, wy = 0.0;
        for (int s = 0; s < kPrepWaves; ++s) {
            s_at[tid][s] = held;
            held += s_cnt[tid][s];
            wsum += s_p[tid][s];
            wy += s_q[tid][s];
        }
        s_held[tid] = held;
        s_wb[tid] = wsum;
        s_ybar[tid] = a.fit_mean ? wy / wsum : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        long long at = 0;
        for (int b = 0; b < B; ++b) {
            s_start[b] = at;
            at += s_held[b];
        }
        s_start[B] = at;   // (n, unless a label was out of range)
    }
    __syncthreads();

    // pass 2: the item's records from s_start[b] + s_at[b][wave] on; every place is below s_start[b + 1] <= n because
    // pass 1 counted the same matches
    for (int b = 0; b < B; ++b) {
        long long at = s_start[b] + s_at[b][wave];
        const double ybar = s_ybar[b];
        double yy = 0.0, y1 = 0.0;
        for (int64_t base = lo; base < hi; base += 64 * kPrepUnroll) {
            int lbl[kPrepUnroll];
#pragma unroll
            for (int u = 0; u < kPrepUnroll; ++u) lbl[u] = label_at(a.band, base + u * 64 + lane, hi);
#pragma unroll
            for (int u = 0; u < kPrepUnroll; ++u) {
                const int64_t i = base + u * 64 + lane;
                const bool mine = lbl[u] == b;
                const unsigned long long mask = __ballot(mine);
                if (mine) {
                    const long long place = at + __popcll(mask & ((1ull << lane) - 1ull));
                    const double w = inv_var(a.dy, i) / W;
                    const double yc = a.y[i] - ybar;
                    const double wy = w * yc;
                    yy += wy * yc;
                    y1 += wy;
                    put_record(a.rec + place * 6, wy, w, a.delta, a.t[i] - tmin);
                }
                at += __popcll(mask);
            }
        }
        yy = wave_sum(yy);
        y1 = wave_sum(y1);
        if (lane == 0) {
            s_p[b][wave] = yy;
            s_q[b][wave] = y1;
        }
    }
    put_spare_records(a.rec, n, tid);
    __syncthreads();
    if (tid < B) {
        double yy = 0.0, y1 = 0.0;
        for (int s = 0; s < kPrepWaves; ++s) {
            yy += s_p[tid][s];
            y1 += s_q[tid][s];
        }
        s_yy[tid] = yy;
        a.scal[kScalWb + tid] = s_wb[tid];
        a.scal[kScalYb + tid] = y1;
    }
    if (tid <= B) reinterpret_cast<long long *>(a.scal + kScalStart)[tid] = s_start[tid];
    __syncthreads();
    if (tid == 0) {
        double yy = 0.0, wsum = 0.0;
        for (int b = 0; b < B; ++b) {   // bands in order: the same bits at every call
            yy += s_yy[b];
            wsum += s_wb[b];
        }
        a.scal[kScalYY] = yy;
        a.scal[kScalWsum] = wsum;
        a.scal[kScalWerr] = W;
        a.scal[kScalBad] = s_bad ? 1.0 : 0.0;
    }
}

// ---- the scan -------------------------------------------------------------------------------------------------------
// The scalar block is read as wave-uniform values through the scalar cache (as the records are): the band loop's
// bounds, and with them the barriers and the record addresses inside it, are uniform to the compiler too.
using ci64 = __attribute__((address_space(4))) const long long;
__device__ __forceinline__ double scal_at(const double *scal, int i) {
    return reinterpret_cast<const cdbl *>(reinterpret_cast<uintptr_t>(scal))[i];
}
__device__ __forceinline__ int64_t start_at(const double *scal, int b) {
    return reinterpret_cast<const ci64 *>(reinterpret_cast<uintptr_t>(scal + kScalStart))[b];
}

// H = harmonics, K = trial frequencies per thread: (6 H + 2 H + H (2H + 1)) K doubles of sums, snapshots and rank-one
// terms, whatever the number of bands.
// Epilogue: basis order (cos th, sin th, ..., cos H th, sin H th); entry (r, c), r >= c, of M' is that of M_hh minus the
// bands' rank-one terms in corr[r (r + 1) / 2 + c].
template <int H, int K>
__global__ __launch_bounds__(kBlock) void mbgls_scan_kernel(MbArgs a) {
    constexpr int COLS = kBlock / 64;   // 64-lane columns of the tile
    constexpr int NC = H * (2 * H + 1);
    // per sample: {sin, cos} of theta_tile + 8 q Theta, q < 8 COLS | {sin, cos}(b Theta), b < 8 (fill_rotation_tables)
    __shared__ double2 tab[kChunk + 1][COLS * 8 + 8 + 1];   // + 1: rows start 16 B apart modulo 128 B (bank spread)

    const int64_t tile = xcd_tile(blockIdx.x, a.tiles);
    if (tile >= a.tiles) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int col = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t n = a.n;
    // first local frequency of the tile and of this thread
    const int64_t jt = tile * kBlock * (int64_t)K;
    const int64_t jl = jt + (int64_t)tid * K;

    if (scal_at(a.scal, kScalBad) != 0.0) {   // a label out of range: the prologue placed no such sample - every bin NaN
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (jl + k < a.nf) a.power[jl + k] = __builtin_nan("");
        return;
    }

    // numpy's arange fill rule: start + i*delta, two roundings (no fma)
    const double f_tile = __dadd_rn(a.f0, __dmul_rn((double)(a.j_begin + jt), a.delta));
    const double kdelta = (double)K * a.delta;   // spacing of the threads' first frequencies (exact)

    double Cm[2 * H][K], Sm[2 * H][K], YC[H][K], YS[H][K];
    double snapC[H][K], snapS[H][K], corr[NC][K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int m = 0; m < 2 * H; ++m) Cm[m][k] = Sm[m][k] = 0.0;
#pragma unroll
        for (int h = 0; h < H; ++h) YC[h][k] = YS[h][k] = snapC[h][k] = snapS[h][k] = 0.0;
#pragma unroll
        for (int e = 0; e < NC; ++e) corr[e][k] = 0.0;
    }
    double q0 = 0.0;

    const int slot_a = col * 8 + (lane >> 3), slot_b = COLS * 8 + (lane & 7);
    int64_t beg = start_at(a.scal, 0);
    for (int b = 0; b < a.n_bands; ++b) {
        const int64_t end = start_at(a.scal, b + 1);
        if (end <= beg) continue;   // an empty band
        // one stretch per band (a band that ends mid-chunk ends its stretch: the read-ahead sees the next band's records)
        scan_stretch<kChunk, K>(
            tab, a.rec, n, beg, end, tid, slot_a, slot_b,
            [&](double2 *row, const int64_t i, const bool real) {   // (sin, cos) unscaled
                fill_rotation_tables<COLS>(row, tid & 1, real ? a.rec[i * 6 + 5] : 0.0, kdelta, f_tile, 1.0);
            },
            [&](const Ahead &h, const int k, const double s, const double c) {
                const double wy = h.r[0], w = h.r[1];
                const double c2 = c + c;
                double sm = s, cm = c, sl = 0.0, cl = 1.0;   // harmonic m and m - 1
#pragma unroll
                for (int m = 1; m <= 2 * H; ++m) {
                    Cm[m - 1][k] = __builtin_fma(w, cm, Cm[m - 1][k]);
                    Sm[m - 1][k] = __builtin_fma(w, sm, Sm[m - 1][k]);
                    if (m <= H) {
                        YC[m - 1][k] = __builtin_fma(wy, cm, YC[m - 1][k]);
                        YS[m - 1][k] = __builtin_fma(wy, sm, YS[m - 1][k]);
                    }
                    if (m < 2 * H) {
                        const double cn = __builtin_fma(c2, cm, -cl), sn = __builtin_fma(c2, sm, -sl);
                        cl = cm;
                        sl = sm;
                        cm = cn;
                        sm = sn;
                    }
                }
            });
        if (a.fit_mean) {   // the band's offset leaves the normal equations
            const double iw = 1.0 / scal_at(a.scal, kScalWb + b), Yb = scal_at(a.scal, kScalYb + b);
            const double yw = Yb * iw;
            q0 = __builtin_fma(Yb, yw, q0);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double v[2 * H];
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    v[2 * h] = Cm[h][k] - snapC[h][k];
                    v[2 * h + 1] = Sm[h][k] - snapS[h][k];
                    snapC[h][k] = Cm[h][k];
                    snapS[h][k] = Sm[h][k];
                    YC[h][k] = __builtin_fma(-yw, v[2 * h], YC[h][k]);
                    YS[h][k] = __builtin_fma(-yw, v[2 * h + 1], YS[h][k]);
                }
#pragma unroll
                for (int r = 0; r < 2 * H; ++r) {
                    const double vr = v[r] * iw;
#pragma unroll
                    for (int c = 0; c <= r; ++c) corr[r * (r + 1) / 2 + c][k] = __builtin_fma(vr, v[c], corr[r * (r + 1) / 2 + c][k]);
                }
            }
        }
        beg = end;
    }

    const double YY = scal_at(a.scal, kScalYY), Wsum = scal_at(a.scal, kScalWsum), Werr = scal_at(a.scal, kScalWerr);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t j = jl + k;
        if (j < a.nf) {
            double Cs[2 * H + 1], Ss[2 * H + 1], bv[2 * H];
            gather_fourier_sums<H, K>(Cm, Sm, YC, YS, k, Wsum, Cs, Ss, bv);
            const double quad = cholesky_quadratic<2 * H>(
                [&](const int r, const int c) { return fourier_entry<H>(Cs, Ss, r, c) - corr[r * (r + 1) / 2 + c][k]; }, bv,
                2 * H);
            a.power[j] = normalised_power(q0 + quad, a.psd, Werr, YY);
        }
    }
}

// Frequencies per thread: the doubles above are 11 K at H = 1, 26 K at H = 2 and 45 K at H = 3, so K = 4 / 2 / 2 keeps
// every instance in registers (88 / 104 / 180 VGPRs of state); a tile is 1024 / 512 / 512 frequencies.
constexpr int freqs_of(int nterms) { return nterms == 1 ? 4 : 2; }

int64_t mb_work_bytes(int64_t n) { return up256((n + 2) * 48) + up256(kScalCount * 8); }

int mb_validate(const char *what, int64_t n, int n_bands, double delta, int64_t j_begin, int64_t nf, int nterms,
                int fit_mean) {
    PDC_REQUIRE(n >= 0 && nf >= 0 && j_begin >= 0, "%s: negative size", what);
    PDC_REQUIRE(nterms >= 1 && nterms <= kMaxTerms, "%s: nterms must be 1 .. %d (got %d)", what, kMaxTerms, nterms);
    PDC_REQUIRE(n_bands >= 1 && n_bands <= kMaxBands, "%s: n_bands must be 1 .. %d (got %d)", what, kMaxBands, n_bands);
    PDC_REQUIRE(std::isfinite(delta) && delta > 0.0, "%s: the grid step must be finite and positive", what);
    const int cols = 2 * nterms + (fit_mean ? n_bands : 0);
    PDC_REQUIRE(n >= cols + 1, "%s: %d parameters are fitted, at least %d samples are needed (got %lld)", what, cols,
                cols + 1, (long long)n);
    const int64_t tile = kBlock * freqs_of(nterms);
    PDC_REQUIRE((nf + tile - 1) / tile < ((int64_t)1 << 31) - 8, "%s: grid too large", what);
    return PDC_OK;
}

int mb_enqueue(hipStream_t st, const double *d_t, const double *d_y, const double *d_dy, const int32_t *d_band, int64_t n,
               int n_bands, double f0, double delta, int64_t j_begin, int64_t nf, int nterms, int fit_mean, int psd,
               double *d_power, void *work) {
    MbPrepArgs p;
    p.t = d_t;
    p.y = d_y;
    p.dy = d_dy;
    p.band = fit_mean ? d_band : nullptr;   // without offsets the bands do not enter: one stretch, no label read
    p.n = n;
    p.n_bands = fit_mean ? n_bands : 1;
    p.fit_mean = fit_mean;
    p.delta = delta;
    p.rec = static_cast<double *>(work);
    p.scal = reinterpret_cast<double *>(static_cast<char *>(work) + up256((n + 2) * 48));
    hipLaunchKernelGGL(mbgls_prep_kernel, dim3(1), dim3(kPrepBlock), 0, st, p);
    PDC_HIP(hipGetLastError());
    const int64_t tile = kBlock * freqs_of(nterms);
    MbArgs a;
    a.rec = p.rec;
    a.scal = p.scal;
    a.n = n;
    a.tiles = (nf + tile - 1) / tile;
    a.f0 = f0;
    a.delta = delta;
    a.j_begin = j_begin;
    a.nf = nf;
    a.n_bands = p.n_bands;
    a.fit_mean = fit_mean;
    a.psd = psd;
    a.power = d_power;
    const dim3 grid((unsigned)((a.tiles + 7) / 8 * 8));
    switch (nterms) {
        case 1: hipLaunchKernelGGL((mbgls_scan_kernel<1, freqs_of(1)>), grid, dim3(kBlock), 0, st, a); break;
        case 2: hipLaunchKernelGGL((mbgls_scan_kernel<2, freqs_of(2)>), grid, dim3(kBlock), 0, st, a); break;
        default: hipLaunchKernelGGL((mbgls_scan_kernel<3, freqs_of(3)>), grid, dim3(kBlock), 0, st, a); break;
    }
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

}  // namespace

extern "C" {

int pdc_mbgls_tile_bins(int nterms) {
    return nterms >= 1 && nterms <= kMaxTerms ? kBlock * freqs_of(nterms) : -1;
}

int pdc_mbgls_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy,
                       const int32_t *d_band, int64_t n, int n_bands, double f0, double delta, int64_t j_begin, int64_t nf,
                       int nterms, int fit_mean, int psd, double *d_power) {
    PDC_REQUIRE(d_t && d_y && d_band && (d_power || nf == 0), "mbgls: NULL argument");
    PDC_TRY(mb_validate("mbgls", n, n_bands, delta, j_begin, nf, nterms, fit_mean));
    if (nf == 0) return PDC_OK;
    PDC_TRY(use_device(device));
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, mb_work_bytes(n), &work));
    return mb_enqueue(st, d_t, d_y, d_dy, d_band, n, n_bands, f0, delta, j_begin, nf, nterms, fit_mean, psd, d_power, work);
}

int pdc_mbgls_scan(const double *t, const double *y, const double *dy, const int32_t *band, int64_t n, int n_bands,
                   double f0, double delta, int64_t j_begin, int64_t nf, int nterms, int fit_mean, int psd,
                   double *power_out, int device) {
    PDC_REQUIRE(t && y && band && (power_out || nf == 0), "mbgls: NULL argument");
    PDC_TRY(mb_validate("mbgls", n, n_bands, delta, j_begin, nf, nterms, fit_mean));
    int64_t held[kMaxBands] = {0};
    for (int64_t i = 0; i < n; ++i) {
        PDC_REQUIRE(band[i] >= 0 && band[i] < n_bands, "mbgls: band[%lld] = %d is not a label in 0 .. %d", (long long)i,
                    (int)band[i], n_bands - 1);
        ++held[band[i]];
    }
    for (int b = 0; b < n_bands; ++b) PDC_REQUIRE(held[b] > 0, "mbgls: band %d has no samples", b);
    if (nf == 0) return PDC_OK;
    HostCall hc(device);
    double *d_t = hc.in(SLOT_IN0, t, n * 8), *d_y = hc.in(SLOT_IN1, y, n * 8), *d_dy = hc.in(SLOT_IN2, dy, n * 8);
    int32_t *d_band = hc.in(SLOT_IN3, band, n * 4);
    double *d_out = hc.out<double>(SLOT_OUT0, nf * 8);
    void *d_work = hc.reserve(SLOT_WORK, mb_work_bytes(n));
    PDC_TRY(hc.status);
    PDC_TRY(mb_enqueue(hc.stream(), d_t, d_y, d_dy, d_band, n, n_bands, f0, delta, j_begin, nf, nterms, fit_mean, psd, d_out,
                       d_work));
    hc.back(power_out, d_out, nf * 8);
    return hc.finish();
}

}  // extern "C"
