// Z^2_m (Rayleigh for m = 1; Buccheri et al. 1983, A&A 128, 245) and the H-test (de Jager, Raubenheimer & Swanepoel
// 1989, A&A 221, 180) of an event list as an exact direct summation on gfx950.  Events t_i, photon weights w_i (1 where
// none are given; Kerr 2011, ApJ 732, 38 for the weighted form), theta_i = 2 pi f (t_i - t_0), t_0 = t[0]:
//     C_k(f) = sum w_i cos(k theta_i),  S_k(f) = sum w_i sin(k theta_i),
//     Z^2_m(f) = (2 / sum w_i^2) sum_{k <= m} (C_k^2 + S_k^2),
//     H(f) = max_{1 <= m <= nharm} (Z^2_m - 4 m + 4), with the lowest m that reaches the maximum.
//
// The reference (periodicity.spectral) has no such class: PARITY UNPINNED BY THE REFERENCE.
//
// Decomposition (records, prep kernel, part runs, partial sums, epilogue, ladder and sizes are in htest_common.h, shared
// with htest_fdot.hip)
//   htest_prep_kernel    one workgroup: sum w^2 (block_sum, fixed order) and one 48-byte record per event
//                        {w, w, cos(2 pi delta t'), sin(2 pi delta t'), 2 cos(2 pi delta t'), t' = t - t0}, plus the
//                        two spare records the pipeline reads ahead.
//   htest_scan_kernel    scan_stretch of gls_sums.h (rotation tables per 64-event chunk, two-set scalar pipeline,
//                        grid walk) over the part's run, (sin, cos) carried unscaled; harmonics 2 .. HT of every (event,
//                        frequency) by harmonic_ladder (harmonic_sums.h), 2 HT running sums per frequency, one fma
//                        each with w as the SGPR operand: 4 HT - 2 fma per pair plus the walk.  Workgroup (tile, part)
//                        streams the part's run of whole chunks.  parts == 1: the epilogue is fused, only the outputs are
//                        written.  parts > 1: the workgroup writes its sums to partial[part][2 HT][nf] (rows k < nharm
//                        of C, then of S), and
//   htest_finish_kernel  one thread per bin adds the parts in ascending order (reads coalesced over bins) and runs the
//                        same epilogue.  No atomics: for a given `parts` the bits are the same from call to call.
//
// Instantiations <HT, K, BLOCK>: a call with nharm runs the smallest HT >= nharm and its epilogue takes the first nharm
// harmonics.  The running sums are 4 HT K VGPRs; every tile is K BLOCK = 1024 frequencies, so a grid cuts into the
// same tiles whatever nharm is.
//     HT =  2  4  8 12 : K = 4, BLOCK = 256    32 .. 192 VGPRs of sums (192: the budget of mhgls_scan_kernel<4, 4>)
//     HT = 16 20       : K = 2, BLOCK = 512   128, 160 VGPRs of sums; 512 threads bound the kernel to 256 VGPRs
// A larger K at small HT would save half an fma per pair of the walk (3 per pair at K = 4, 2.5 at K = 8) against the
// 4 HT - 2 of the harmonics; it is not worth another launch shape.
//
// The parts rule (parts == 0), a function of (n, nf, nharm, CU count) only:
//     tiles = ceil(nf / 1024), chunks = ceil(n / 64)
//     parts = min(ceil(2 CUs / tiles), max(1, chunks / 8))
// two workgroups per CU where the grid alone does not give them, while a part keeps at least 8 chunks (512 events):
// a part pays one write of 2 nharm K BLOCK sums and its share of the finish kernel, about what a sixteenth of a chunk
// costs.  Under PDC_WORK_BUDGET_GB the records and the partial sums together stay within the budget: fewer parts (the
// explicit count too), never an error.  An explicit count above 65535 (the launch grid's second dimension) is 65535.
#include "htest_common.h"

namespace {

struct HtArgs {
    const double *rec, *scal;
    int64_t n;
    double f0, delta;
    int64_t j_begin, nf;
    int nharm, parts;
    double *partial;   // [parts][2 HT][nf], parts > 1
    double *h;
    int32_t *m;
    double *z2;
};

// ---- the scan --------------------------------------------------------------------------------------------------------
// blockIdx.x = tile, blockIdx.y = part.  Dynamic LDS: the table of BLOCK = 512 is 76 KB.
template <int HT, int K, int BLOCK>
__global__ __launch_bounds__(BLOCK) void htest_scan_kernel(HtArgs a) {
    static_assert(K * BLOCK == kTile, "every tile is kTile frequencies");
    constexpr int COLS = BLOCK / 64;      // 64-lane columns of the tile
    constexpr int ROW = COLS * 8 + 8 + 1;   // + 1: rows start 16 B apart modulo 128 B (bank spread)
    // per event: {sin, cos} of theta_tile + 8 q Theta, q < 8 COLS | {sin, cos}(b Theta), b < 8 (fill_rotation_tables)
    extern __shared__ double2 htest_lds[];
    double2(*tab)[ROW] = reinterpret_cast<double2(*)[ROW]>(htest_lds);   // [kChunk + 1][ROW]

    const int64_t tile = blockIdx.x;
    const int part = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int col = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t jt = tile * kTile;
    const int64_t jl = jt + (int64_t)tid * K;
    // numpy's arange fill rule: start + i*delta, two roundings (no fma)
    const double f_tile = __dadd_rn(a.f0, __dmul_rn((double)(a.j_begin + jt), a.delta));
    const double kdelta = (double)K * a.delta;   // spacing of the threads' first frequencies (exact)
    int64_t s_beg, s_end;
    part_run(part, a.parts, a.n, s_beg, s_end);

    double Ck[HT][K], Sk[HT][K];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int m = 0; m < HT; ++m) Ck[m][k] = Sk[m][k] = 0.0;

    const int slot_a = col * 8 + (lane >> 3), slot_b = COLS * 8 + (lane & 7);
    scan_stretch<kChunk, K>(
        tab, a.rec, a.n, s_beg, s_end, tid, slot_a, slot_b,
        [&](double2 *row, const int64_t i, const bool real) {   // (sin, cos) unscaled
            fill_rotation_tables<COLS>(row, tid & 1, real ? a.rec[i * 6 + 5] : 0.0, kdelta, f_tile, 1.0);
        },
        [&](const Ahead &h, const int k, const double s, const double c) { add_harmonics<HT, K>(Ck, Sk, k, h.r[1], s, c); });

    if (a.parts == 1) {
        const double scale = 2.0 / a.scal[0];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t j = jl + k;
            if (j < a.nf)
                htest_epilogue<HT>(
                    a.nharm, scale, [&](const int m) { return make_double2(Ck[m][k], Sk[m][k]); }, j, a.h, a.m, a.z2);
        }
        return;
    }
    store_partial<HT, K>(a.partial + (int64_t)part * (2 * HT) * a.nf, a.nf, a.nharm, jl, Ck, Sk);
}

// One thread per bin; `ht` is the scan's HT (the row count of a part's block).
__global__ __launch_bounds__(kFinishBlock) void htest_finish_kernel(HtArgs a, int ht) {
    const int64_t j = (int64_t)blockIdx.x * kFinishBlock + threadIdx.x;
    if (j >= a.nf) return;
    htest_epilogue<kMaxHarm>(
        a.nharm, 2.0 / a.scal[0], [&](const int m) { return sum_parts(a.partial, ht, a.nf, a.parts, j, m); }, j, a.h, a.m,
        a.z2);
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct HtDispatch {
    int ht, k, parts;
};
thread_local HtDispatch g_last = {};

// The parts a call runs: the automatic rule for asked == 0, then the launch limit and the budget.
int parts_of(int asked, int64_t n, int64_t nf, int ht, int cus) {
    int64_t parts = asked;
    if (asked == 0) parts = auto_parts(n, (nf + kTile - 1) / kTile, cus);
    if (parts > kMaxParts) parts = kMaxParts;
    const int64_t budget = work_budget();
    if (budget > 0 && parts > 1 && rec_bytes(n) + partial_bytes(nf, ht, (int)parts) > budget)
        parts = (budget - rec_bytes(n)) / ((int64_t)2 * ht * nf * 8);
    return parts < 2 ? 1 : (int)parts;
}

template <int HT, int K, int BLOCK>
int launch_scan(hipStream_t st, const HtArgs &a) {
    const int lds = scan_lds_bytes(BLOCK);
    PDC_TRY(allow_dynamic_lds((const void *)htest_scan_kernel<HT, K, BLOCK>, lds));
    const dim3 grid((unsigned)((a.nf + kTile - 1) / kTile), (unsigned)a.parts);
    hipLaunchKernelGGL((htest_scan_kernel<HT, K, BLOCK>), grid, dim3(BLOCK), lds, st, a);
    return PDC_OK;
}

// `work`: rec_bytes(n) of records and scalars, then partial_bytes(nf, rung.ht, parts)
int ht_enqueue(hipStream_t st, const double *d_t, const double *d_w, int64_t n, double f0, double delta, int64_t j_begin,
               int64_t nf, int nharm, const Rung &rung, int parts, double *d_h, int32_t *d_m, double *d_z2, void *work) {
    HtPrepArgs p;
    PDC_TRY(ht_enqueue_prep(st, d_t, d_w, n, delta, work, p));
    HtArgs a;
    a.rec = p.rec;
    a.scal = p.scal;
    a.n = n;
    a.f0 = f0;
    a.delta = delta;
    a.j_begin = j_begin;
    a.nf = nf;
    a.nharm = nharm;
    a.parts = parts;
    a.partial = reinterpret_cast<double *>(static_cast<char *>(work) + rec_bytes(n));
    a.h = d_h;
    a.m = d_m;
    a.z2 = d_z2;
    g_last = {rung.ht, rung.k, parts};
    PDC_TRY(with_rung(rung, [&](auto r) { return launch_scan<decltype(r)::ht, decltype(r)::k, decltype(r)::block>(st, a); }));
    PDC_HIP(hipGetLastError());
    if (parts > 1) {
        hipLaunchKernelGGL(htest_finish_kernel, dim3((unsigned)((nf + kFinishBlock - 1) / kFinishBlock)), dim3(kFinishBlock),
                           0, st, a, rung.ht);
        PDC_HIP(hipGetLastError());
    }
    return PDC_OK;
}

}  // namespace

extern "C" {

int64_t pdc_htest_tile_bins(int nharm) {
    const Rung *r = rung_of(nharm);
    return r ? (int64_t)r->k * r->block : -1;
}

int pdc_htest_last_dispatch(int *ht, int *k, int *parts) {
    if (ht) *ht = g_last.ht;
    if (k) *k = g_last.k;
    if (parts) *parts = g_last.parts;
    return PDC_OK;
}

int pdc_htest_scan_dev(int device, void *stream, const double *d_t, const double *d_w, int64_t n, double f0, double delta,
                       int64_t j_begin, int64_t nf, int nharm, int parts, double *d_h, int32_t *d_m, double *d_z2) {
    PDC_TRY(ht_validate(n, delta, j_begin, nf, nharm, parts, d_h || d_m || d_z2));
    PDC_REQUIRE(d_t, "htest: NULL argument");
    if (nf == 0) return PDC_OK;
    PDC_TRY(use_device(device));
    const Rung &rung = *rung_of(nharm);
    parts = parts_of(parts, n, nf, rung.ht, cu_count(device));
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, rec_bytes(n) + partial_bytes(nf, rung.ht, parts), &work));
    return ht_enqueue(st, d_t, d_w, n, f0, delta, j_begin, nf, nharm, rung, parts, d_h, d_m, d_z2, work);
}

int pdc_htest_scan(const double *t, const double *w, int64_t n, double f0, double delta, int64_t j_begin, int64_t nf,
                   int nharm, int parts, double *h_out, int32_t *m_out, double *z2_out, int device) {
    PDC_TRY(ht_validate(n, delta, j_begin, nf, nharm, parts, h_out || m_out || z2_out));
    PDC_REQUIRE(t, "htest: NULL argument");
    if (nf == 0) return PDC_OK;
    HostCall hc(device);
    PDC_TRY(hc.status);
    const Rung &rung = *rung_of(nharm);
    parts = parts_of(parts, n, nf, rung.ht, cu_count(device));
    double *d_t = hc.in(SLOT_IN0, t, n * 8), *d_w = hc.in(SLOT_IN1, w, n * 8);
    double *d_h = h_out ? hc.out<double>(SLOT_OUT0, nf * 8) : nullptr;
    int32_t *d_m = m_out ? hc.out<int32_t>(SLOT_OUT1, nf * 4) : nullptr;
    double *d_z2 = z2_out ? hc.out<double>(SLOT_OUT2, nf * 8) : nullptr;
    void *d_work = hc.reserve(SLOT_WORK, rec_bytes(n) + partial_bytes(nf, rung.ht, parts));
    PDC_TRY(hc.status);
    PDC_TRY(ht_enqueue(hc.stream(), d_t, d_w, n, f0, delta, j_begin, nf, nharm, rung, parts, d_h, d_m, d_z2, d_work));
    hc.back(h_out, d_h, nf * 8);
    hc.back(m_out, d_m, nf * 4);
    hc.back(z2_out, d_z2, nf * 8);
    return hc.finish();
}

}  // extern "C"
