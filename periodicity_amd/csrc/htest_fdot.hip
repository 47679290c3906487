// The H-test and Z^2_m of an event list over the (frequency, spin-down) plane: htest.hip's statistic with the phase
//     phase_i(f, fdot) = f tau_i + fdot tau_i^2 / 2 cycles,   tau_i = t_i - epoch,
// for every trial frequency of the grid and every fdot of a list, reduced on the device to the ridge (per frequency
// the best fdot) and the best cell.  f (t_0 - epoch) is common to all events and drops out of every C_k^2 + S_k^2, so
// the scan keeps f t' with t' = t - t[0] from htest.hip's records and adds only the offset
//     phi_i = frac(fdot tau_i^2 / 2)
// to an event's tile base phase, in cycles, before the one sincos of the table fill (its `offset`).  phi is
// reduced exactly: tau^2 as the pair (hi, lo) of a product and its fma error, frac_product(fdot / 2, hi) + fdot / 2 lo.
// A handful of flops per (event, tile, row): no further sincos, no [nfd][n] table in memory, and the 1024 frequencies
// of the tile walk from the base as before at 4 HT - 2 fma per pair.  fdot = 0 gives phi = 0 and the bits of
// pdc_htest_scan at the same `parts`.
//
// Decomposition (records, part runs, partial sums, ladder, epilogue, sizes: htest_common.h)
//   htest_prep_kernel        as htest.hip.
//   htest_fdot_scan_kernel   scan_stretch of gls_sums.h over the part's run, with phi in the fill; blockIdx = (tile, part,
//                            row) and `row` indexes the fdot values of this
//                            launch; the row is an SGPR, fdot / 2 and the epoch wait in LDS for the table fills (in
//                            SGPRs across the hot loop they cost two VGPRs).  parts == 1: the epilogue is fused and
//                            writes the row's values (H, or Z^2 at nharm) and m to the plane, or to a [rows][nf] slab
//                            of the workspace where the caller asked for no plane.  parts > 1: the sums go to
//                            partial[row][part][2 HT][nf].
//   htest_fdot_fold_kernel   one thread per bin, the launch's rows in ascending order: parts > 1 adds the parts in
//                            ascending order, runs the epilogue and writes the plane row where one is asked for;
//                            parts == 1 reads what the scan wrote.  Either way the row is folded into the running
//                            ridge (ArgMax: NaN never wins, the lowest row of equal maxima wins, value NaN and row -1
//                            where nothing is finite), which carries from launch to launch in ascending row order.
//   htest_fdot_best_kernel   one workgroup: ArgMax over the ridge in ascending bin order (lowest bin of equal maxima).
// No atomics: for a given (parts, rows per launch) the bits are the same from call to call; the ridge and the best
// cell do not depend on the rows per launch at all (they are maxima of the same values in the same order).
//
// Rows per launch and parts.  rows = min(nfd, 65535) (the launch grid's third dimension).  parts == 0: htest.hip's rule
// with tiles x rows workgroups per part, parts = min(ceil(2 CUs / (tiles rows)), max(1, chunks / 8)): rows fill the
// device where parts had to.  Workspace: the records, the ridge state (16 B per bin), and per row of a launch either
// the partial sums (parts > 1) or the slabs of what the caller does not take (parts == 1: 8 B per bin of values without
// a plane, 4 B per bin of m for the H-test without an m plane).  Under PDC_WORK_BUDGET_GB: fewer rows per launch first
// (where a row costs workspace at all), then, at one row, fewer parts; never an error.  The automatic parts are chosen
// from min(nfd, 65535) rows BEFORE the budget cuts the rows of a launch and are not raised again afterwards (parts cost
// workspace of their own, so raising them would argue with the same budget): a budget that leaves one or two rows per
// launch runs a short grid with tiles x rows workgroups and underfills the device.  An explicit `parts` is the way out.
#include "htest_common.h"

namespace {

struct FdArgs {
    const double *rec, *scal, *t, *fdot;   // fdot: [nfd] on the device
    int64_t n;
    double f0, delta, epoch;
    int64_t j_begin, nf;
    int nharm, parts, stat;   // stat 0: H (and m), 1: Z^2 at nharm
    int64_t row0;             // first row of this launch
    int rows;                 // rows of this launch
    double *partial;          // [rows][parts][2 HT][nf], parts > 1
    double *val;              // [rows][nf]: the plane from row0 on, or the slab; NULL: parts > 1 and no plane
    int32_t *m;               // likewise for m (NULL with stat 1)
    double *ridge;            // [nf] running ridge: value (NaN where row is -1), row, m (NULL with stat 1)
    int32_t *ridge_row, *ridge_m;
    double *best;             // [1] | NULL
    int64_t *best_at;         // [3] (bin, row, m) | NULL
};

// frac(hfd tau^2), hfd = fdot / 2, with tau^2 carried exactly
__device__ __forceinline__ double spin_down_cycles(double hfd, double tau) {
    const double hi = tau * tau;
    const double lo = __builtin_fma(tau, tau, -hi);
    return frac_product(hfd, hi) + hfd * lo;
}

// blockIdx.x = tile, blockIdx.y = part, blockIdx.z = row of the launch.  Dynamic LDS as htest_scan_kernel.
template <int HT, int K, int BLOCK>
__global__ __launch_bounds__(BLOCK) void htest_fdot_scan_kernel(FdArgs a) {
    static_assert(K * BLOCK == kTile, "every tile is kTile frequencies");
    constexpr int COLS = BLOCK / 64;
    constexpr int ROW = COLS * 8 + 8 + 1;
    extern __shared__ double2 htest_fdot_lds[];
    double2(*tab)[ROW] = reinterpret_cast<double2(*)[ROW]>(htest_fdot_lds);   // [kChunk + 1][ROW]

    const int64_t tile = blockIdx.x;
    const int part = blockIdx.y;
    const int row = blockIdx.z;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int col = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t jt = tile * kTile;
    const int64_t jl = jt + (int64_t)tid * K;
    // numpy's arange fill rule: start + i*delta, two roundings (no fma)
    const double f_tile = __dadd_rn(a.f0, __dmul_rn((double)(a.j_begin + jt), a.delta));
    const double kdelta = (double)K * a.delta;   // spacing of the threads' first frequencies (exact)
    // The row's two constants, fdot / 2 and the epoch, wait in LDS for the table fills (the first read is behind the
    // stretch's first barrier).  Held in scalar registers across the hot loop they cost every instance two VGPRs at its
    // peak, and <12, 4, 256>, which sits at 256, its second wave per SIMD.
    __shared__ double fd_const[2];
    if (tid == 0) {
        fd_const[0] = 0.5 * a.fdot[a.row0 + row];
        fd_const[1] = a.epoch;
    }
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
        [&](double2 *trow, const int64_t i, const bool real) {   // (sin, cos) unscaled, the base moved by phi_i
            fill_rotation_tables<COLS>(trow, tid & 1, real ? a.rec[i * 6 + 5] : 0.0, kdelta, f_tile, 1.0, [&] {
                return spin_down_cycles(fd_const[0], real ? a.t[i] - fd_const[1] : 0.0);
            });
        },
        [&](const Ahead &h, const int k, const double s, const double c) { add_harmonics<HT, K>(Ck, Sk, k, h.r[1], s, c); });

    if (a.parts == 1) {
        const double scale = 2.0 / a.scal[0];
        double *val = a.val + (int64_t)row * a.nf;
        int32_t *m_out = a.m ? a.m + (int64_t)row * a.nf : nullptr;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t j = jl + k;
            if (j < a.nf)
                htest_epilogue<HT>(
                    a.nharm, scale, [&](const int m) { return make_double2(Ck[m][k], Sk[m][k]); }, j,
                    a.stat == 0 ? val : nullptr, m_out, a.stat == 0 ? nullptr : val);
        }
        return;
    }
    store_partial<HT, K>(a.partial + ((int64_t)row * a.parts + part) * (2 * HT) * a.nf, a.nf, a.nharm, jl, Ck, Sk);
}

// One thread per bin; `ht` is the scan's HT (the row count of a part's block).
__global__ __launch_bounds__(kFinishBlock) void htest_fdot_fold_kernel(FdArgs a, int ht) {
    const int64_t j = (int64_t)blockIdx.x * kFinishBlock + threadIdx.x;
    if (j >= a.nf) return;
    ArgMax am;
    int32_t am_m = -1;
    if (a.row0 > 0) {   // the ridge so far (a row of -1: nothing finite yet, whatever the value says)
        am.v = a.ridge[j];
        am.j = a.ridge_row[j];
        if (a.ridge_m) am_m = a.ridge_m[j];
    }
    const int64_t part_stride = (int64_t)2 * ht * a.nf;
    const double scale = 2.0 / a.scal[0];
    for (int row = 0; row < a.rows; ++row) {
        double v;
        int32_t mv = -1;
        if (a.parts > 1) {
            double h, z2;
            const double *p0 = a.partial + (int64_t)row * a.parts * part_stride;
            htest_epilogue<kMaxHarm>(
                a.nharm, scale,
                [&](const int m) { return sum_parts(p0, ht, a.nf, a.parts, j, m); },
                0, &h, &mv, &z2);
            v = a.stat == 0 ? h : z2;
            if (a.val) a.val[(int64_t)row * a.nf + j] = v;
            if (a.m) a.m[(int64_t)row * a.nf + j] = mv;
        } else {
            v = a.val[(int64_t)row * a.nf + j];
            if (a.m) mv = a.m[(int64_t)row * a.nf + j];
        }
        const long long before = am.j;
        am.take(v, a.row0 + row);
        if (am.j != before) am_m = mv;
    }
    a.ridge[j] = am.j < 0 ? __longlong_as_double(0x7ff8000000000000ll) : am.v;
    a.ridge_row[j] = (int32_t)am.j;
    if (a.ridge_m) a.ridge_m[j] = am.j < 0 ? -1 : am_m;
}

// One workgroup.  Wave w takes the w-th run of bins, its lanes interleaved (coalesced reads): a lane sees ascending
// bins, wave_fold compares the indices of equal maxima, the waves fold in order.
__global__ __launch_bounds__(kPrepBlock) void htest_fdot_best_kernel(FdArgs a) {
    constexpr int WAVES = kPrepBlock / 64;
    __shared__ double red_v[WAVES];
    __shared__ long long red_i[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t run = (a.nf + WAVES - 1) / WAVES;
    const int64_t beg = wave * run, end = beg + run < a.nf ? beg + run : a.nf;
    ArgMax am;
    for (int64_t j = beg + lane; j < end; j += 64)
        if (a.ridge_row[j] >= 0) am.take(a.ridge[j], j);
    if (!am.block_fold<WAVES>(red_v, red_i, lane, wave)) return;
    if (a.best) a.best[0] = am.j < 0 ? __longlong_as_double(0x7ff8000000000000ll) : am.v;
    if (a.best_at) {
        a.best_at[0] = am.j;
        a.best_at[1] = am.j < 0 ? -1 : a.ridge_row[am.j];
        a.best_at[2] = am.j < 0 ? -1 : (a.ridge_m ? a.ridge_m[am.j] : a.nharm);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct FdDispatch {
    int ht, k, parts, rows;
    int64_t launches;
};
thread_local FdDispatch g_last = {};

// What a call runs and where its workspace parts lie: records | ridge value, row, m | per launch row: partial sums, or
// the value and m slabs.
struct FdPlan {
    const Rung *rung;
    int parts, rows;
    bool slab_v, slab_m;
    int64_t at_ridge, at_ridge_row, at_ridge_m, at_rows, row_bytes, total;
};

int64_t fd_row_bytes(int64_t nf, int ht, int parts, bool slab_v, bool slab_m) {
    if (parts > 1) return up256(partial_bytes(nf, ht, parts));
    return (slab_v ? up256(nf * 8) : 0) + (slab_m ? up256(nf * 4) : 0);
}

FdPlan fd_plan(int64_t n, int64_t nf, int64_t nfd, int nharm, int stat, int asked, int cus, bool have_plane,
               bool have_m_plane) {
    FdPlan p;
    p.rung = rung_of(nharm);
    const int ht = p.rung->ht;
    p.slab_v = !have_plane;
    p.slab_m = stat == 0 && !have_m_plane;
    Carve c;
    c.take(rec_bytes(n));
    p.at_ridge = c.take(nf * 8);
    p.at_ridge_row = c.take(nf * 4);
    p.at_ridge_m = c.take(nf * 4);
    p.at_rows = c.at;
    int64_t rows = nfd < kMaxParts ? nfd : kMaxParts;   // (the grid's third dimension has the second's limit)
    int64_t parts = asked;
    if (asked == 0) parts = auto_parts(n, (nf + kTile - 1) / kTile * rows, cus);
    if (parts > kMaxParts) parts = kMaxParts;
    if (parts < 2) parts = 1;
    const int64_t budget = work_budget();
    if (budget > 0) {
        const int64_t room = budget - p.at_rows;
        int64_t per = fd_row_bytes(nf, ht, (int)parts, p.slab_v, p.slab_m);
        if (per > 0 && rows * per > room) rows = room / per < 1 ? 1 : room / per;
        if (parts > 1 && per > room) {   // one row and still too much: fewer parts
            parts = room / ((int64_t)2 * ht * nf * 8);
            if (parts < 2) parts = 1;
            per = fd_row_bytes(nf, ht, (int)parts, p.slab_v, p.slab_m);
            rows = nfd < kMaxParts ? nfd : kMaxParts;
            if (per > 0 && rows * per > room) rows = room / per < 1 ? 1 : room / per;
        }
    }
    p.parts = (int)parts;
    p.rows = (int)rows;
    p.row_bytes = fd_row_bytes(nf, ht, p.parts, p.slab_v, p.slab_m);
    p.total = p.at_rows + p.rows * p.row_bytes;
    return p;
}

int fd_validate(int64_t n, double delta, int64_t j_begin, int64_t nf, int64_t nfd, double epoch, int nharm, int stat,
                int parts, const void *m_plane, const void *ridge_m, bool any_output) {
    PDC_TRY(ht_validate(n, delta, j_begin, nf, nharm, parts, any_output));
    PDC_REQUIRE(nfd >= 1, "htest fdot: at least one fdot is needed (got %lld)", (long long)nfd);
    PDC_REQUIRE(std::isfinite(epoch), "htest fdot: the epoch must be finite");
    PDC_REQUIRE(stat == 0 || stat == 1, "htest fdot: stat must be 0 (H) or 1 (Z^2) (got %d)", stat);
    PDC_REQUIRE(stat == 0 || (!m_plane && !ridge_m), "htest fdot: Z^2 (stat 1) has no harmonics outputs");
    return PDC_OK;
}

template <int HT, int K, int BLOCK>
int launch_scan(hipStream_t st, const FdArgs &a) {
    const int lds = scan_lds_bytes(BLOCK);
    PDC_TRY(allow_dynamic_lds((const void *)htest_fdot_scan_kernel<HT, K, BLOCK>, lds));
    const dim3 grid((unsigned)((a.nf + kTile - 1) / kTile), (unsigned)a.parts, (unsigned)a.rows);
    hipLaunchKernelGGL((htest_fdot_scan_kernel<HT, K, BLOCK>), grid, dim3(BLOCK), lds, st, a);
    return PDC_OK;
}

// `work`: plan.total bytes.  Outputs are device pointers, any of them NULL.
int fd_enqueue(hipStream_t st, const double *d_t, const double *d_w, int64_t n, double f0, double delta, int64_t j_begin,
               int64_t nf, const double *d_fdot, int64_t nfd, double epoch, int nharm, int stat, const FdPlan &plan,
               double *d_plane, int32_t *d_m_plane, double *d_ridge, int32_t *d_ridge_row, int32_t *d_ridge_m,
               double *d_best, int64_t *d_best_at, void *work) {
    HtPrepArgs p;
    PDC_TRY(ht_enqueue_prep(st, d_t, d_w, n, delta, work, p));
    char *base = static_cast<char *>(work);
    FdArgs a;
    a.rec = p.rec;
    a.scal = p.scal;
    a.t = d_t;
    a.fdot = d_fdot;
    a.n = n;
    a.f0 = f0;
    a.delta = delta;
    a.epoch = epoch;
    a.j_begin = j_begin;
    a.nf = nf;
    a.nharm = nharm;
    a.parts = plan.parts;
    a.stat = stat;
    a.ridge = d_ridge ? d_ridge : reinterpret_cast<double *>(base + plan.at_ridge);
    a.ridge_row = d_ridge_row ? d_ridge_row : reinterpret_cast<int32_t *>(base + plan.at_ridge_row);
    a.ridge_m = stat != 0 ? nullptr : d_ridge_m ? d_ridge_m : reinterpret_cast<int32_t *>(base + plan.at_ridge_m);
    a.best = d_best;
    a.best_at = d_best_at;
    char *rows_at = base + plan.at_rows;
    const int ht = plan.rung->ht;
    g_last = {ht, plan.rung->k, plan.parts, plan.rows, (nfd + plan.rows - 1) / plan.rows};
    for (int64_t row0 = 0; row0 < nfd; row0 += plan.rows) {
        a.row0 = row0;
        a.rows = (int)(nfd - row0 < plan.rows ? nfd - row0 : plan.rows);
        a.partial = reinterpret_cast<double *>(rows_at);
        a.val = d_plane ? d_plane + row0 * nf : nullptr;
        a.m = d_m_plane ? d_m_plane + row0 * nf : nullptr;
        if (plan.parts == 1) {   // the slabs of what the caller does not take: the fold reads them
            char *slab = rows_at;
            if (plan.slab_v) {
                a.val = reinterpret_cast<double *>(slab);
                slab += up256(nf * 8) * plan.rows;
            }
            if (plan.slab_m) a.m = reinterpret_cast<int32_t *>(slab);
        }
        PDC_TRY(with_rung(*plan.rung,
                          [&](auto r) { return launch_scan<decltype(r)::ht, decltype(r)::k, decltype(r)::block>(st, a); }));
        PDC_HIP(hipGetLastError());
        hipLaunchKernelGGL(htest_fdot_fold_kernel, dim3((unsigned)((nf + kFinishBlock - 1) / kFinishBlock)),
                           dim3(kFinishBlock), 0, st, a, ht);
        PDC_HIP(hipGetLastError());
    }
    if (d_best || d_best_at) {
        hipLaunchKernelGGL(htest_fdot_best_kernel, dim3(1), dim3(kPrepBlock), 0, st, a);
        PDC_HIP(hipGetLastError());
    }
    return PDC_OK;
}

}  // namespace

extern "C" {

int pdc_htest_fdot_last_dispatch(int *ht, int *k, int *parts, int *rows_per_launch, int64_t *launches) {
    if (ht) *ht = g_last.ht;
    if (k) *k = g_last.k;
    if (parts) *parts = g_last.parts;
    if (rows_per_launch) *rows_per_launch = g_last.rows;
    if (launches) *launches = g_last.launches;
    return PDC_OK;
}

int64_t pdc_htest_fdot_work_bytes(int64_t n, int64_t nf, int64_t nfd, int nharm, int parts, int want_plane) {
    if (n < 1 || nf < 0 || nfd < 1 || parts < 0 || !rung_of(nharm)) return -1;
    if (nf == 0) return rec_bytes(n);   // nothing to scan: the scan entries return before they plan, so does the size
    return fd_plan(n, nf, nfd, nharm, 0, parts, cu_count(-1), want_plane != 0, want_plane != 0).total;
}

int pdc_htest_fdot_scan_dev(int device, void *stream, const double *d_t, const double *d_w, int64_t n, double f0,
                            double delta, int64_t j_begin, int64_t nf, const double *d_fdot, int64_t nfd, double epoch,
                            int nharm, int stat, int parts, double *d_plane, int32_t *d_m_plane, double *d_ridge,
                            int32_t *d_ridge_row, int32_t *d_ridge_m, double *d_best, int64_t *d_best_at) {
    PDC_TRY(fd_validate(n, delta, j_begin, nf, nfd, epoch, nharm, stat, parts, d_m_plane, d_ridge_m,
                        d_plane || d_m_plane || d_ridge || d_ridge_row || d_ridge_m || d_best || d_best_at));
    PDC_REQUIRE(d_t && d_fdot, "htest fdot: NULL argument");
    if (nf == 0) return PDC_OK;
    PDC_TRY(use_device(device));
    const FdPlan plan = fd_plan(n, nf, nfd, nharm, stat, parts, cu_count(device), d_plane != nullptr, d_m_plane != nullptr);
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, plan.total, &work));
    return fd_enqueue(st, d_t, d_w, n, f0, delta, j_begin, nf, d_fdot, nfd, epoch, nharm, stat, plan, d_plane, d_m_plane,
                      d_ridge, d_ridge_row, d_ridge_m, d_best, d_best_at, work);
}

int pdc_htest_fdot_scan(const double *t, const double *w, int64_t n, double f0, double delta, int64_t j_begin, int64_t nf,
                        const double *fdot, int64_t nfd, double epoch, int nharm, int stat, int parts, double *plane_out,
                        int32_t *m_plane_out, double *ridge_out, int32_t *ridge_row_out, int32_t *ridge_m_out,
                        double *best_out, int64_t *best_at_out, int device) {
    PDC_TRY(fd_validate(n, delta, j_begin, nf, nfd, epoch, nharm, stat, parts, m_plane_out, ridge_m_out,
                        plane_out || m_plane_out || ridge_out || ridge_row_out || ridge_m_out || best_out || best_at_out));
    PDC_REQUIRE(t && fdot, "htest fdot: NULL argument");
    for (int64_t r = 0; r < nfd; ++r)
        PDC_REQUIRE(std::isfinite(fdot[r]), "htest fdot: fdot[%lld] is not finite", (long long)r);
    PDC_REQUIRE(nf == 0 || nfd <= (((int64_t)1 << 62) / 8) / nf, "htest fdot: plane too large");
    if (nf == 0) return PDC_OK;
    HostCall hc(device);
    PDC_TRY(hc.status);
    const FdPlan plan = fd_plan(n, nf, nfd, nharm, stat, parts, cu_count(device), plane_out != nullptr, m_plane_out != nullptr);
    double *d_t = hc.in(SLOT_IN0, t, n * 8), *d_w = hc.in(SLOT_IN1, w, n * 8), *d_fdot = hc.in(SLOT_IN2, fdot, nfd * 8);
    double *d_plane = plane_out ? hc.out<double>(SLOT_OUT0, nfd * nf * 8) : nullptr;
    int32_t *d_m_plane = m_plane_out ? hc.out<int32_t>(SLOT_OUT1, nfd * nf * 4) : nullptr;
    // the small outputs share one block: ridge | ridge_row | ridge_m | best | best_at
    Carve c;
    const int64_t at_ridge = c.take(nf * 8), at_row = c.take(nf * 4), at_m = c.take(nf * 4), at_best = c.take(8),
                  at_best_at = c.take(24);
    char *d_small = hc.out<char>(SLOT_OUT2, c.at);
    void *d_work = hc.reserve(SLOT_WORK, plan.total);
    PDC_TRY(hc.status);
    double *d_ridge = ridge_out ? reinterpret_cast<double *>(d_small + at_ridge) : nullptr;
    int32_t *d_row = ridge_row_out ? reinterpret_cast<int32_t *>(d_small + at_row) : nullptr;
    int32_t *d_rm = ridge_m_out ? reinterpret_cast<int32_t *>(d_small + at_m) : nullptr;
    double *d_best = best_out ? reinterpret_cast<double *>(d_small + at_best) : nullptr;
    int64_t *d_best_at = best_at_out ? reinterpret_cast<int64_t *>(d_small + at_best_at) : nullptr;
    PDC_TRY(fd_enqueue(hc.stream(), d_t, d_w, n, f0, delta, j_begin, nf, d_fdot, nfd, epoch, nharm, stat, plan, d_plane,
                       d_m_plane, d_ridge, d_row, d_rm, d_best, d_best_at, d_work));
    hc.back(plane_out, d_plane, nfd * nf * 8);
    hc.back(m_plane_out, d_m_plane, nfd * nf * 4);
    hc.back(ridge_out, d_ridge, nf * 8);
    hc.back(ridge_row_out, d_row, nf * 4);
    hc.back(ridge_m_out, d_rm, nf * 4);
    hc.back(best_out, d_best, 8);
    hc.back(best_at_out, d_best_at, 24);
    return hc.finish();
}

}  // extern "C"
