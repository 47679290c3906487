// Multi-harmonic generalised Lomb-Scargle (Schwarzenberg-Czerny 1996; Palmer 2009; the `nterms` of other packages) as
// an exact direct summation on gfx950: per trial frequency the weighted least-squares fit of a Fourier series of H
// harmonics (plus a floating mean), power = b^T M^-1 b / YY.
//
// The reference (/root/reference/src/periodicity/spectral.py) has no such class: PARITY UNPINNED BY THE REFERENCE.
// The weights, the centring and the two normalisations are those of GLS (spectral.py:99-108, 129-132).
//
// Decomposition
//   mhgls_prep_kernel   one workgroup: weights, weighted mean, YY, and one 48-byte record per sample
//                       {w y, w, cos(2 pi delta t'), sin(2 pi delta t'), 2 cos(2 pi delta t'), t' = t - t0}.
//   mhgls_scan_kernel   one stretch [0, n) of scan_stretch (gls_sums.h): each thread owns K consecutive frequencies,
//                       the records come through the scalar cache, the seed of a (sample, thread) is one
//                       plane rotation of two LDS table entries built per 64-sample chunk from exact cycle reductions,
//                       and a rotation plus the three-term recurrence walk the K frequencies.  (sin, cos) are carried
//                       UNscaled here: harmonics 2 .. 2H of every (sample, frequency) follow from them by
//                       harmonic_ladder, and add_fourier_sums keeps the 6H running sums per frequency, one fma each
//                       (harmonic_sums.h).  Epilogue, from the same header: fourier_entry turns the sums into M by the
//                       product-to-sum rules and cholesky_quadratic, unrolled in registers, into b^T M^-1 b: only
//                       power[nf] is written.
//
// One workgroup per tile of 256 K frequencies streams the whole curve (as the MODE_TREND instances of gls.hip do); no
// sample parts, no balanced pieces, one device.
#include "pdc_internal.h"
#include "harmonic_sums.h"

#include <cmath>

using namespace pdc;

namespace {

constexpr int kBlock = 256;
constexpr int kPrepBlock = 1024;
constexpr int kChunk = 64;   // samples per rotation-table chunk
constexpr int kMaxTerms = 4;

struct MhPrepArgs {
    const double *t, *y, *dy;
    int64_t n;
    int fit_mean;
    double delta;
    double *rec;    // [n + 2][6] (the scan reads one record ahead)
    double *scal;   // {YY, sum w, sum err^-2, sum w y}
};

struct MhArgs {
    const double *rec, *scal;
    int64_t n, tiles;
    double f0, delta;
    int64_t j_begin, nf;
    int fit_mean, psd;
    double *power;
};

// ---- prologue: weights, centring and YY as GLS takes them (spectral.py:99-108, 120) ---------------------------------
__global__ __launch_bounds__(kPrepBlock) void mhgls_prep_kernel(MhPrepArgs a) {
    __shared__ double red[kPrepBlock / 64];
    const int tid = threadIdx.x;
    const double t0 = a.n > 0 ? a.t[0] : 0.0;
    double W, ybar;
    weights_and_mean<kPrepBlock>(a.y, a.dy, a.n, a.fit_mean, red, W, ybar);
    double yy = 0.0, wsum = 0.0, y1 = 0.0;
    for (int64_t i = tid; i < a.n; i += kPrepBlock) {
        const double tp = a.t[i] - t0;
        const double w = inv_var(a.dy, i) / W;
        const double yc = a.y[i] - ybar;
        const double wy = w * yc;
        yy += wy * yc;
        wsum += w;
        y1 += wy;
        put_record(a.rec + i * 6, wy, w, a.delta, tp);
    }
    put_spare_records(a.rec, a.n, tid);
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

// ---- the scan -----------------------------------------------------------------------------------------------------
// H = harmonics, K = trial frequencies per thread: 6 H K accumulators (12 H K VGPRs).
// Epilogue: basis order (cos th, sin th, ..., cos H th, sin H th, 1).  The constant comes LAST, so the model without a
// floating mean is the same factorisation stopped one column early; b = {YC_1, YS_1, ..., YC_H, YS_H, sum w y}.
template <int H, int K>
__global__ __launch_bounds__(kBlock) void mhgls_scan_kernel(MhArgs a) {
    constexpr int COLS = kBlock / 64;   // 64-lane columns of the tile
    // per sample: {sin, cos} of theta_tile + 8 q Theta, q < 8 COLS (the seed of lanes 8q .. 8q+7 before their own
    // offset) | {sin, cos}(b Theta), b < 8
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
    // numpy's arange fill rule: start + i*delta, two roundings (no fma)
    const double f_tile = __dadd_rn(a.f0, __dmul_rn((double)(a.j_begin + jt), a.delta));
    const double kdelta = (double)K * a.delta;   // spacing of the threads' first frequencies (exact)

    double Cm[2 * H][K], Sm[2 * H][K], YC[H][K], YS[H][K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int m = 0; m < 2 * H; ++m) Cm[m][k] = Sm[m][k] = 0.0;
#pragma unroll
        for (int h = 0; h < H; ++h) YC[h][k] = YS[h][k] = 0.0;
    }

    const int slot_a = col * 8 + (lane >> 3), slot_b = COLS * 8 + (lane & 7);
    scan_stretch<kChunk, K>(
        tab, a.rec, n, 0, n, tid, slot_a, slot_b,
        [&](double2 *row, const int64_t i, const bool real) {   // (sin, cos) unscaled
            fill_rotation_tables<COLS>(row, tid & 1, real ? a.rec[i * 6 + 5] : 0.0, kdelta, f_tile, 1.0);
        },
        [&](const Ahead &h, const int k, const double s, const double c) {
            add_fourier_sums<H, K>(Cm, Sm, YC, YS, k, h.r[1], h.r[0], s, c);
        });

    const double YY = a.scal[0], Wsum = a.scal[1], Werr = a.scal[2], Y1 = a.scal[3];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t j = jl + k;
        if (j < a.nf) {
            constexpr int D = 2 * H + 1;
            double Cs[D], Ss[D], b[D];
            gather_fourier_sums<H, K>(Cm, Sm, YC, YS, k, Wsum, Cs, Ss, b);
            b[2 * H] = Y1;
            const double quad = cholesky_quadratic<D>(
                [&](const int r, const int c) {   // the constant's row: sum w cos / sin (h th), then sum w
                    if (r < 2 * H) return fourier_entry<H>(Cs, Ss, r, c);
                    return c == 2 * H ? Cs[0] : ((c & 1) ? Ss[c / 2 + 1] : Cs[c / 2 + 1]);
                },
                b, a.fit_mean ? D : D - 1);
            a.power[j] = normalised_power(quad, a.psd, Werr, YY);
        }
    }
}

// Frequencies per thread, for every H: the 6 H K running sums are 12 H K registers - 192 at H = 4, the budget of the
// headline kernel - and a tile is 1024 frequencies whatever H is.
constexpr int kFreqs = 4;

int64_t mh_work_bytes(int64_t n) { return up256((n + 2) * 48) + 256; }

int mh_validate(const char *what, int64_t n, double delta, int64_t j_begin, int64_t nf, int nterms, int fit_mean) {
    PDC_REQUIRE(n >= 0 && nf >= 0 && j_begin >= 0, "%s: negative size", what);
    PDC_REQUIRE(nterms >= 1 && nterms <= kMaxTerms, "%s: nterms must be 1 .. %d (got %d)", what, kMaxTerms, nterms);
    PDC_REQUIRE(std::isfinite(delta) && delta > 0.0, "%s: the grid step must be finite and positive", what);
    const int cols = 2 * nterms + (fit_mean ? 1 : 0);
    PDC_REQUIRE(n >= cols + 1, "%s: %d parameters are fitted, at least %d samples are needed (got %lld)", what, cols,
                cols + 1, (long long)n);
    PDC_REQUIRE((nf + kBlock * kFreqs - 1) / (kBlock * kFreqs) < ((int64_t)1 << 31) - 8, "%s: grid too large", what);
    return PDC_OK;
}

int mh_enqueue(hipStream_t st, const double *d_t, const double *d_y, const double *d_dy, int64_t n, double f0, double delta,
               int64_t j_begin, int64_t nf, int nterms, int fit_mean, int psd, double *d_power, void *work) {
    MhPrepArgs p;
    p.t = d_t;
    p.y = d_y;
    p.dy = d_dy;
    p.n = n;
    p.fit_mean = fit_mean;
    p.delta = delta;
    p.rec = static_cast<double *>(work);
    p.scal = reinterpret_cast<double *>(static_cast<char *>(work) + up256((n + 2) * 48));
    hipLaunchKernelGGL(mhgls_prep_kernel, dim3(1), dim3(kPrepBlock), 0, st, p);
    PDC_HIP(hipGetLastError());
    MhArgs a;
    a.rec = p.rec;
    a.scal = p.scal;
    a.n = n;
    a.tiles = (nf + kBlock * kFreqs - 1) / (kBlock * kFreqs);
    a.f0 = f0;
    a.delta = delta;
    a.j_begin = j_begin;
    a.nf = nf;
    a.fit_mean = fit_mean;
    a.psd = psd;
    a.power = d_power;
    const dim3 grid((unsigned)((a.tiles + 7) / 8 * 8));
    switch (nterms) {
        case 1: hipLaunchKernelGGL((mhgls_scan_kernel<1, kFreqs>), grid, dim3(kBlock), 0, st, a); break;
        case 2: hipLaunchKernelGGL((mhgls_scan_kernel<2, kFreqs>), grid, dim3(kBlock), 0, st, a); break;
        case 3: hipLaunchKernelGGL((mhgls_scan_kernel<3, kFreqs>), grid, dim3(kBlock), 0, st, a); break;
        default: hipLaunchKernelGGL((mhgls_scan_kernel<4, kFreqs>), grid, dim3(kBlock), 0, st, a); break;
    }
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

}  // namespace

extern "C" {

int pdc_mhgls_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                       double f0, double delta, int64_t j_begin, int64_t nf, int nterms, int fit_mean, int psd,
                       double *d_power) {
    PDC_REQUIRE(d_t && d_y && (d_power || nf == 0), "mhgls: NULL argument");
    PDC_TRY(mh_validate("mhgls", n, delta, j_begin, nf, nterms, fit_mean));
    if (nf == 0) return PDC_OK;
    PDC_TRY(use_device(device));
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, mh_work_bytes(n), &work));
    return mh_enqueue(st, d_t, d_y, d_dy, n, f0, delta, j_begin, nf, nterms, fit_mean, psd, d_power, work);
}

int pdc_mhgls_scan(const double *t, const double *y, const double *dy, int64_t n, double f0, double delta, int64_t j_begin,
                   int64_t nf, int nterms, int fit_mean, int psd, double *power_out, int device) {
    PDC_REQUIRE(t && y && (power_out || nf == 0), "mhgls: NULL argument");
    PDC_TRY(mh_validate("mhgls", n, delta, j_begin, nf, nterms, fit_mean));
    if (nf == 0) return PDC_OK;
    HostCall hc(device);
    double *d_t = hc.in(SLOT_IN0, t, n * 8), *d_y = hc.in(SLOT_IN1, y, n * 8), *d_dy = hc.in(SLOT_IN2, dy, n * 8);
    double *d_out = hc.out<double>(SLOT_OUT0, nf * 8);
    void *d_work = hc.reserve(SLOT_WORK, mh_work_bytes(n));
    PDC_TRY(hc.status);
    PDC_TRY(mh_enqueue(hc.stream(), d_t, d_y, d_dy, n, f0, delta, j_begin, nf, nterms, fit_mean, psd, d_out, d_work));
    hc.back(power_out, d_out, nf * 8);
    return hc.finish();
}

}  // extern "C"
