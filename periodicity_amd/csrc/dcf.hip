// The discrete correlation function (Edelson & Krolik 1988, ApJ 333, 646) of two unevenly sampled curves on gfx950:
// every ordered pair (i, j) of samples is binned by its lag tb[j] - ta[i]; per bin the pair count and six sums, from
// which the host forms the globally normalised DCF (Edelson & Krolik) or the locally normalised one (Lehar et al. 1992;
// White & Peterson 1994).  With both curves the same and the diagonal left out it is the autocorrelation function of a
// curve that need not be evenly sampled.
//
// The reference has an ACF for evenly sampled series only (core.py:578-608) and no cross-correlation: PARITY UNPINNED BY
// THE REFERENCE.
//
// The predicate.  Pair (i, j) has lag d = fl(tb[j] - ta[i]), one IEEE subtraction, and is in bin k iff
// edges[k] <= d < edges[k+1].  Nothing else is ever compared: `below(i, j, e)` = (d < e) is the only test the kernel
// makes.  A rounded subtraction is monotone, and both time tables never decrease, so for a fixed i the j with d < e are
// a prefix of tb, and that prefix never shrinks as i advances.  first(i, e) = the first j with not d < e.  Bin k's pairs
// of sample i are the run [first(i, edges[k]), first(i, edges[k+1])): the run of bin k ends where the run of bin k + 1
// begins, by the same comparison of the same two doubles, so a pair with edges[0] <= d < edges[nlag] is in exactly one bin.
//
// Decomposition
//   dcf_scan_kernel    a workgroup owns one chunk of consecutive i and a tile of 256 bins, a thread one bin.  It finds
//                      first(i0, lo) and first(i0, hi) by bisection, then carries both forward from i to i + 1 (a step
//                      each on average).  Per i the count is the run's length, and sum b and sum b^2 over the run are
//                      folded in with a_i:
//                          Sa += a n,  Saa += a^2 n,  Sb += sum b,  Sbb += sum b^2,  Sab += a sum b,  Sabab += a^2 sum b^2.
//                      The runs of consecutive i overlap almost entirely, and the walk is bound by its per-lane gathers
//                      (about one 8-byte access per clock and CU, measured), not by arithmetic: so kRows = 8 consecutive
//                      i share ONE walk of [their first run's start, their last run's end).  Every b[j] is loaded once
//                      and added, in ascending j, to each of the eight (sum b, sum b^2) whose run holds j; the others
//                      get + 0.0, which changes no bit and keeps a NaN out of the runs it is not in.  (One i per walk:
//                      6.6 ms at 1e5 samples x 1000 lags; 2 / 4 / 8 / 16: 6.3 / 4.0 / 3.0 / 3.0 ms, 16 at 249 VGPRs.)
//                      An empty run folds nothing (a NaN in a_i stays out of the bins it has no pair in).  The chunk's
//                      seven values per bin go to its slab of the workspace.
//   dcf_fold_kernel    a thread per (sum, bin): the chunks' slabs in ascending chunk order.
// No atomics, no LDS; every sum in one fixed order that depends on the shapes and the chunk alone: the same bits from
// call to call.
#include "pdc_internal.h"

#include <cmath>

using namespace pdc;

namespace {

constexpr int kBlock = 256;                        // bins per tile, one per thread
constexpr int64_t kMaxLags = (int64_t)1 << 22;     // 16 384 tiles; one chunk's slab: 224 MiB
constexpr int64_t kMaxSamples = ((int64_t)1 << 31) - 64;   // sample indices are 32-bit in the scan
constexpr int64_t kMaxChunks = (int64_t)1 << 24;  // the grid's x: chunks x kBlock threads stay below 2^32
constexpr int64_t kMinChunk = 64;                  // the library's own choice is a multiple of this
constexpr int64_t kWantGroups = 4096;              // workgroups to aim for: 256 CUs x 8 resident x 2
constexpr int64_t kSlabCap = (int64_t)1 << 31;     // bytes of slabs the library's own choice stays under
constexpr int kSums = 6;                           // Sa, Sb, Saa, Sbb, Sab, Sabab
constexpr int kRows = 8;                           // consecutive i a thread takes through one walk of b

struct DcfArgs {
    const double *ta, *a, *tb, *b, *edges;
    int64_t na, nb, nlag, chunk, chunks;
    double *slab;      // [chunks][6][nlag]
    int64_t *count;    // [chunks][nlag]
    int64_t *pairs_out;
    double *sums_out;  // [6][nlag]
};

// THE predicate: is the lag of (ti, tb[j]) below the edge e?
__device__ __forceinline__ bool below(const double *tb, int j, double ti, double e) {
    return __dsub_rn(tb[j], ti) < e;
}

// The first j in [0, nb] that is not below e, by bisection.
__device__ __forceinline__ int first_not_below(const double *tb, int nb, double ti, double e) {
    int lo = 0, hi = nb;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (below(tb, mid, ti, e))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Sample indices are 32-bit (a curve has fewer than 2^31 samples); the counts and the slab offsets are 64-bit.
template <bool SKIP>
__global__ __launch_bounds__(kBlock) void dcf_scan_kernel(DcfArgs p) {
    const int64_t k = (int64_t)blockIdx.y * kBlock + threadIdx.x;
    if (k >= p.nlag) return;
    const int64_t c = blockIdx.x;
    const int i0 = (int)(c * p.chunk);
    const int i1 = (int)(c * p.chunk + p.chunk < p.na ? c * p.chunk + p.chunk : p.na);
    const double lo = p.edges[k], hi = p.edges[k + 1];
    const double *__restrict__ ta = p.ta;   // (read only, as a: they may be tb and b)
    const double *__restrict__ a = p.a;
    const double *__restrict__ tb = p.tb;
    const double *__restrict__ b = p.b;
    const int nb = (int)p.nb;

    int jlo = first_not_below(tb, nb, ta[i0], lo);
    int jhi = first_not_below(tb, nb, ta[i0], hi);
    int64_t n = 0;
    double Sa = 0.0, Sb = 0.0, Saa = 0.0, Sbb = 0.0, Sab = 0.0, Sabab = 0.0;
    for (int i = i0; i < i1; i += kRows) {   // (i1 - i <= chunk: no overflow before the test)
        // the runs of the group's samples, [r0, r0 + len): both ends never move back, so the group's pairs lie in
        // [r0[0], jhi)
        int r0[kRows], len[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (r < i1 - i) {
                const double ti = ta[i + r];
                while (jlo < nb && below(tb, jlo, ti, lo)) ++jlo;
                while (jhi < nb && below(tb, jhi, ti, hi)) ++jhi;   // (jhi >= jlo: lo < hi)
                r0[r] = jlo;
                len[r] = jhi - jlo;
            } else {   // past the chunk: an empty run
                r0[r] = jhi;
                len[r] = 0;
            }
        }
        // one walk for the group: every b[j] loaded once, added to the samples whose run holds j (0.0 to the others:
        // exact, and a NaN stays out of the runs it is not in)
        double s[kRows], q[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) s[r] = q[r] = 0.0;
        auto take = [&](const int j, const double bj) {
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                bool in = (unsigned)(j - r0[r]) < (unsigned)len[r];
                if (SKIP) in = in && j != i + r;
                const double v = in ? bj : 0.0;
                s[r] += v;
                q[r] = __builtin_fma(v, v, q[r]);
            }
        };
        int j = r0[0];
        for (; j < jhi - 1; j += 2) {
            const double b0 = b[j], b1 = b[j + 1];
            take(j, b0);
            take(j + 1, b1);
        }
        if (j < jhi) take(j, b[j]);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const bool self = SKIP && (unsigned)(i + r - r0[r]) < (unsigned)len[r];
            const int m = len[r] - (self ? 1 : 0);
            if (m <= 0) continue;   // (a_i stays out of a bin it has no pair in; past the chunk it is not even read)
            const double ai = a[i + r], a2 = ai * ai, fm = (double)m;
            n += m;
            Sa = __builtin_fma(ai, fm, Sa);
            Saa = __builtin_fma(a2, fm, Saa);
            Sb += s[r];
            Sbb += q[r];
            Sab = __builtin_fma(ai, s[r], Sab);
            Sabab = __builtin_fma(a2, q[r], Sabab);
        }
    }
    double *slab = p.slab + c * kSums * p.nlag + k;
    slab[0] = Sa;
    slab[p.nlag] = Sb;
    slab[2 * p.nlag] = Saa;
    slab[3 * p.nlag] = Sbb;
    slab[4 * p.nlag] = Sab;
    slab[5 * p.nlag] = Sabab;
    p.count[c * p.nlag + k] = n;
}

// A thread per (row, bin), row 6 the counts: the chunks in ascending order.  Also what writes the zeros of a call
// without pairs (chunks == 0).
__global__ __launch_bounds__(kBlock) void dcf_fold_kernel(DcfArgs p) {
    const int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (at >= (kSums + 1) * p.nlag) return;
    const int64_t row = at / p.nlag, k = at - row * p.nlag;
    if (row == kSums) {
        int64_t n = 0;
        for (int64_t c = 0; c < p.chunks; ++c) n += p.count[c * p.nlag + k];
        p.pairs_out[k] = n;
    } else {
        double s = 0.0;
        for (int64_t c = 0; c < p.chunks; ++c) s += p.slab[(c * kSums + row) * p.nlag + k];
        p.sums_out[at] = s;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct DcfDispatch {
    int64_t chunks, chunk;
};
thread_local DcfDispatch g_last = {};

int dcf_validate(int64_t na, int64_t nb, int64_t nlag, int skip_same, int64_t chunk, bool outputs) {
    PDC_REQUIRE(na >= 0 && nb >= 0, "dcf: the sample counts must not be negative (got %lld and %lld)", (long long)na,
                (long long)nb);
    PDC_REQUIRE(na <= kMaxSamples && nb <= kMaxSamples, "dcf: at most 2^31 - 64 samples a curve");
    PDC_REQUIRE(nlag >= 1 && nlag <= kMaxLags, "dcf: 1 <= nlag <= %lld is needed (got %lld)", (long long)kMaxLags,
                (long long)nlag);
    PDC_REQUIRE(chunk >= 0, "dcf: chunk must be 0 (the library chooses) or positive (got %lld)", (long long)chunk);
    PDC_REQUIRE(!skip_same || na == nb, "dcf: skip_same_index needs curves of one length (got %lld and %lld)",
                (long long)na, (long long)nb);
    PDC_REQUIRE(outputs, "dcf: NULL output");
    return PDC_OK;
}

// The size functions refuse what the scan refuses: the same checks, no output asked for.
bool dcf_sizes_ok(int64_t na, int64_t nb, int64_t nlag, int64_t chunk) {
    return dcf_validate(na, nb, nlag, 0, chunk, true) == PDC_OK;
}

constexpr int64_t slab_bytes(int64_t nlag) { return (kSums + 1) * 8 * nlag + 2 * 256; }   // (the two parts' roundings)

// The i per chunk: the caller's, or enough chunks for kWantGroups workgroups in multiples of kMinChunk, and no more
// slabs than kSlabCap holds.  PDC_WORK_BUDGET_GB enlarges either until the slabs fit it, up to one chunk of all i.
int64_t dcf_chunk_for(int64_t na, int64_t nlag, int64_t forced) {
    if (na == 0) return forced > 0 ? forced : kMinChunk;
    int64_t chunk = forced;
    int64_t cap = work_budget();
    if (forced <= 0) {
        const int64_t tiles = (nlag + kBlock - 1) / kBlock;
        const int64_t want = (kWantGroups + tiles - 1) / tiles;
        chunk = ((na + want - 1) / want + kMinChunk - 1) / kMinChunk * kMinChunk;
        if (cap <= 0 || cap > kSlabCap) cap = kSlabCap;
    }
    if (cap > 0) {
        const int64_t fit = cap / slab_bytes(nlag);   // chunks whose slabs the budget holds
        const int64_t least = fit < 1 ? na : (na + fit - 1) / fit;
        if (chunk < least) chunk = least;
    }
    return chunk;
}

struct DcfPlan {
    int64_t chunk, chunks, at_count, total;
};

DcfPlan dcf_plan(int64_t na, int64_t nb, int64_t nlag, int64_t forced) {
    DcfPlan p;
    p.chunk = dcf_chunk_for(na, nlag, forced);
    p.chunks = (na == 0 || nb == 0) ? 0 : (na + p.chunk - 1) / p.chunk;
    const int64_t slabs = p.chunks < 1 ? 1 : p.chunks;
    Carve c;
    c.take(slabs * kSums * nlag * 8);
    p.at_count = c.take(slabs * nlag * 8);
    p.total = c.at;
    return p;
}

int dcf_check_times(const char *name, const double *t, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        PDC_REQUIRE(std::isfinite(t[i]), "dcf: %s[%lld] is not finite", name, (long long)i);
        PDC_REQUIRE(i == 0 || t[i] >= t[i - 1], "dcf: %s must never decrease (at %lld)", name, (long long)i);
    }
    return PDC_OK;
}

// `work`: plan.total bytes.  Inputs and outputs are device pointers.
int dcf_enqueue(hipStream_t st, const double *d_ta, const double *d_a, int64_t na, const double *d_tb, const double *d_b,
                int64_t nb, const double *d_edges, int64_t nlag, int skip_same, const DcfPlan &plan, int64_t *d_pairs,
                double *d_sums, void *work) {
    DcfArgs p;
    p.ta = d_ta;
    p.a = d_a;
    p.tb = d_tb;
    p.b = d_b;
    p.edges = d_edges;
    p.na = na;
    p.nb = nb;
    p.nlag = nlag;
    p.chunk = plan.chunk;
    p.chunks = plan.chunks;
    p.slab = reinterpret_cast<double *>(work);
    p.count = reinterpret_cast<int64_t *>(static_cast<char *>(work) + plan.at_count);
    p.pairs_out = d_pairs;
    p.sums_out = d_sums;
    g_last = {plan.chunks, plan.chunk};
    const int64_t tiles = (nlag + kBlock - 1) / kBlock;
    if (plan.chunks > 0) {
        const dim3 grid((unsigned)plan.chunks, (unsigned)tiles);
        if (skip_same)
            hipLaunchKernelGGL(dcf_scan_kernel<true>, grid, dim3(kBlock), 0, st, p);
        else
            hipLaunchKernelGGL(dcf_scan_kernel<false>, grid, dim3(kBlock), 0, st, p);
        PDC_HIP(hipGetLastError());
    }
    const int64_t fold_blocks = ((kSums + 1) * nlag + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(dcf_fold_kernel, dim3((unsigned)fold_blocks), dim3(kBlock), 0, st, p);
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

// What a plan must meet before a device is looked for: the chunks are the grid's x (chunks x 256 threads < 2^32), and
// the slabs fit the budget.
int dcf_fits(const DcfPlan &plan) {
    PDC_REQUIRE(plan.chunks < kMaxChunks, "dcf: a chunk of %lld samples makes %lld chunks, a launch takes fewer than %lld",
                (long long)plan.chunk, (long long)plan.chunks, (long long)kMaxChunks);
    const int64_t budget = work_budget();
    PDC_REQUIRE(budget <= 0 || plan.total <= budget,
                "dcf: even one chunk of all samples needs %lld bytes of workspace, over the budget of %.3f GB "
                "(PDC_WORK_BUDGET_GB)", (long long)plan.total, (double)budget / (double)(1 << 30));
    return PDC_OK;
}

}  // namespace

extern "C" {

int64_t pdc_dcf_chunk(int64_t na, int64_t nb, int64_t nlag) {
    if (!dcf_sizes_ok(na, nb, nlag, 0)) return -1;
    return dcf_chunk_for(na, nlag, 0);
}

int64_t pdc_dcf_work_bytes(int64_t na, int64_t nb, int64_t nlag, int64_t chunk) {
    if (!dcf_sizes_ok(na, nb, nlag, chunk)) return -1;
    const DcfPlan plan = dcf_plan(na, nb, nlag, chunk);
    return plan.chunks < kMaxChunks ? plan.total : -1;   // (a forced chunk so small that the scan refuses it)
}

int pdc_dcf_last_dispatch(int64_t *chunks, int64_t *chunk) {
    if (chunks) *chunks = g_last.chunks;
    if (chunk) *chunk = g_last.chunk;
    return PDC_OK;
}

int pdc_dcf_scan_dev(int device, void *stream, const double *d_ta, const double *d_a, int64_t na, const double *d_tb,
                     const double *d_b, int64_t nb, const double *d_edges, int64_t nlag, int skip_same_index,
                     int64_t chunk, int64_t *d_pairs, double *d_sums) {
    PDC_TRY(dcf_validate(na, nb, nlag, skip_same_index, chunk, d_pairs && d_sums));
    PDC_REQUIRE(d_edges && (na == 0 || (d_ta && d_a)) && (nb == 0 || (d_tb && d_b)), "dcf: NULL argument");
    const DcfPlan plan = dcf_plan(na, nb, nlag, chunk);
    PDC_TRY(dcf_fits(plan));
    PDC_TRY(use_device(device));
    hipStream_t st = (hipStream_t)stream;
    void *work = nullptr;
    ScratchPin pin;
    PDC_TRY(pin.take(device, st, plan.total, &work));
    return dcf_enqueue(st, d_ta, d_a, na, d_tb, d_b, nb, d_edges, nlag, skip_same_index, plan, d_pairs, d_sums, work);
}

int pdc_dcf_scan(const double *ta, const double *a, int64_t na, const double *tb, const double *b, int64_t nb,
                 const double *edges, int64_t nlag, int skip_same_index, int64_t chunk, int64_t *pairs_out,
                 double *sums_out, int device) {
    PDC_TRY(dcf_validate(na, nb, nlag, skip_same_index, chunk, pairs_out && sums_out));
    PDC_REQUIRE(edges && (na == 0 || (ta && a)) && (nb == 0 || (tb && b)), "dcf: NULL argument");
    const DcfPlan plan = dcf_plan(na, nb, nlag, chunk);
    PDC_TRY(dcf_fits(plan));   // (sizes alone, before an array is read)
    PDC_TRY(dcf_check_times("ta", ta, na));
    PDC_TRY(dcf_check_times("tb", tb, nb));
    for (int64_t k = 0; k <= nlag; ++k) {
        PDC_REQUIRE(std::isfinite(edges[k]), "dcf: edges[%lld] is not finite", (long long)k);
        PDC_REQUIRE(k == 0 || edges[k] > edges[k - 1], "dcf: edges must be strictly increasing (at %lld)", (long long)k);
    }
    HostCall hc(device);
    PDC_TRY(hc.status);
    const bool same = ta == tb && a == b && na == nb;   // autocorrelation: one copy of the curve goes up
    Carve ci;   // ta | a | tb | b | edges share a block
    const int64_t at_ta = ci.take(na * 8), at_a = ci.take(na * 8);
    const int64_t at_tb = same ? at_ta : ci.take(nb * 8), at_b = same ? at_a : ci.take(nb * 8);
    const int64_t at_edges = ci.take((nlag + 1) * 8);
    char *d_in = hc.out<char>(SLOT_IN0, ci.at);
    Carve co;   // pairs | sums another
    const int64_t at_pairs = co.take(nlag * 8), at_sums = co.take(kSums * nlag * 8);
    char *d_out = hc.out<char>(SLOT_OUT0, co.at);
    void *d_work = hc.reserve(SLOT_WORK, plan.total);
    PDC_TRY(hc.status);
    hc.put(d_in + at_ta, na ? ta : nullptr, na * 8);
    hc.put(d_in + at_a, na ? a : nullptr, na * 8);
    if (!same) {
        hc.put(d_in + at_tb, nb ? tb : nullptr, nb * 8);
        hc.put(d_in + at_b, nb ? b : nullptr, nb * 8);
    }
    hc.put(d_in + at_edges, edges, (nlag + 1) * 8);
    PDC_TRY(hc.status);
    int64_t *d_pairs = reinterpret_cast<int64_t *>(d_out + at_pairs);
    double *d_sums = reinterpret_cast<double *>(d_out + at_sums);
    PDC_TRY(dcf_enqueue(hc.stream(), reinterpret_cast<double *>(d_in + at_ta), reinterpret_cast<double *>(d_in + at_a), na,
                        reinterpret_cast<double *>(d_in + at_tb), reinterpret_cast<double *>(d_in + at_b), nb,
                        reinterpret_cast<double *>(d_in + at_edges), nlag, skip_same_index, plan, d_pairs, d_sums, d_work));
    hc.back(pairs_out, d_pairs, nlag * 8);
    hc.back(sums_out, d_sums, kSums * nlag * 8);
    return hc.finish();
}

}  // extern "C"
