// What the H-test units share (htest.hip: one frequency axis; htest_fdot.hip: the frequency - spin-down plane): the
// 48-byte event records and the kernel that makes them, the harmonics' running sums, a part's run of chunks, the store
// and the ascending-order sum of the parts' partial sums, the epilogue from the 2 HT sums of a bin to Z^2_m, H and its
// m, the ladder of kernel instances with its dispatch, the workspace sizes and the argument checks.  Everything is
// internal to the unit that includes it (anonymous namespace): each unit carries its own copy of the prep kernel.
#pragma once
#include "pdc_internal.h"
#include "harmonic_sums.h"

#include <cmath>

namespace {

using namespace pdc;

constexpr int kPrepBlock = 1024;
constexpr int kFinishBlock = 256;
constexpr int kChunk = 64;      // events per rotation-table chunk
constexpr int kMaxHarm = 20;
constexpr int kTile = 1024;     // frequencies per tile, every instantiation
constexpr int kMinChunks = 8;   // chunks a part keeps under the automatic rule
constexpr int kMaxParts = 65535;

struct HtPrepArgs {
    const double *t, *w;
    int64_t n;
    double delta;
    double *rec;    // [n + 2][6]
    double *scal;   // {sum w^2}
};

__global__ __launch_bounds__(kPrepBlock) void htest_prep_kernel(HtPrepArgs a) {
    __shared__ double red[kPrepBlock / 64];
    const int tid = threadIdx.x;
    const double t0 = a.t[0];
    double w2 = 0.0;
    for (int64_t i = tid; i < a.n; i += kPrepBlock) {
        const double w = a.w ? a.w[i] : 1.0;
        w2 += w * w;
        put_record(a.rec + i * 6, w, w, a.delta, a.t[i] - t0);
    }
    put_spare_records(a.rec, a.n, tid);
    w2 = block_sum<kPrepBlock>(w2, red);
    if (tid == 0) a.scal[0] = w2;
}

// ---- epilogue, shared by the fused and the finish paths --------------------------------------------------------------
// cs(k) = {C, S} of harmonic k + 1.  Cumulative Z^2_m in ascending m; H keeps the first maximum as np.argmax does (a NaN
// candidate wins over finite ones, the first NaN stays).  Each output is written only where asked for.
template <int HT, class Sums>
__device__ __forceinline__ void htest_epilogue(int nharm, double scale, Sums cs, int64_t j, double *h_out, int32_t *m_out,
                                               double *z2_out) {
    double cum = 0.0, z = 0.0, best = 0.0;
    int best_m = 1;
#pragma unroll
    for (int k = 1; k <= HT; ++k) {
        if (k <= nharm) {
            const double2 v = cs(k - 1);
            cum += v.x * v.x + v.y * v.y;
            z = scale * cum;
            const double cand = z - (double)(4 * k - 4);
            if (k == 1 || cand > best || (cand != cand && best == best)) {
                best = cand;
                best_m = k;
            }
        }
    }
    if (h_out) h_out[j] = best;
    if (m_out) m_out[j] = best_m;
    if (z2_out) z2_out[j] = z;
}

// Harmonics 1 .. HT of one (event, frequency) pair (harmonic_ladder), each added to its running sums with weight w:
// 4 HT - 2 fma.
template <int HT, int K>
__device__ __forceinline__ void add_harmonics(double (&Ck)[HT][K], double (&Sk)[HT][K], const int k, const double w,
                                              const double s, const double c) {
    harmonic_ladder<HT>(s, c, [&](const int m, const double sm, const double cm) {
        Ck[m - 1][k] = __builtin_fma(w, cm, Ck[m - 1][k]);
        Sk[m - 1][k] = __builtin_fma(w, sm, Sk[m - 1][k]);
    });
}

// ---- sample parts -----------------------------------------------------------------------------------------------------
// Part `part` of `parts` takes a run of whole chunks, events [s_beg, s_end) (an empty run adds zeros).
__device__ __forceinline__ void part_run(int part, int parts, int64_t n, int64_t &s_beg, int64_t &s_end) {
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    s_beg = (int64_t)part * chunks / parts * kChunk;
    s_end = (int64_t)(part + 1) * chunks / parts * kChunk;
    if (s_end > n) s_end = n;
}

// A part's sums of a thread's K bins from jl on, to its block out[2 HT][nf]: rows k < nharm of C, then of S.
template <int HT, int K>
__device__ __forceinline__ void store_partial(double *out, int64_t nf, int nharm, int64_t jl, const double (&Ck)[HT][K],
                                              const double (&Sk)[HT][K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t j = jl + k;
        if (j < nf) {
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                if (m < nharm) {
                    out[(int64_t)m * nf + j] = Ck[m][k];
                    out[(int64_t)(HT + m) * nf + j] = Sk[m][k];
                }
            }
        }
    }
}

// {C, S} of harmonic m + 1 at bin j: the parts' blocks from p0 on (`ht` rows of C, `ht` of S each) added in ascending
// order, reads coalesced over bins.  No atomics: for a given `parts` the bits are the same from call to call.
__device__ __forceinline__ double2 sum_parts(const double *p0, int ht, int64_t nf, int parts, int64_t j, int m) {
    const int64_t part_stride = (int64_t)2 * ht * nf;
    const double *pc = p0 + (int64_t)m * nf + j, *ps = pc + (int64_t)ht * nf;
    double c = 0.0, s = 0.0;
    for (int p = 0; p < parts; ++p) {
        c += pc[p * part_stride];
        s += ps[p * part_stride];
    }
    return make_double2(c, s);
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct Rung {
    int ht, k, block;
};
constexpr Rung kLadder[] = {{2, 4, 256}, {4, 4, 256}, {8, 4, 256}, {12, 4, 256}, {16, 2, 512}, {20, 2, 512}};

constexpr int kRungs = sizeof(kLadder) / sizeof(kLadder[0]);

inline const Rung *rung_of(int nharm) {
    if (nharm < 1 || nharm > kMaxHarm) return nullptr;
    for (const Rung &r : kLadder)
        if (r.ht >= nharm) return &r;
    return nullptr;
}

// f(RungAt<I>()) for the entry I of kLadder with rung.ht, and its status: the kernel instances a unit launches are
// <R::ht, R::k, R::block> of that one table.
template <int I>
struct RungAt {
    static constexpr int ht = kLadder[I].ht, k = kLadder[I].k, block = kLadder[I].block;
};
template <int I = 0, class F>
int with_rung(const Rung &rung, F f) {
    if (rung.ht == kLadder[I].ht) return f(RungAt<I>());
    if constexpr (I + 1 < kRungs) return with_rung<I + 1>(rung, f);
    PDC_REQUIRE(false, "htest: HT = %d is no entry of the ladder", rung.ht);
    return PDC_OK;
}

// dynamic LDS of a scan instance: [kChunk + 1] table rows of 8 COLS + 8 + 1 entries
constexpr int scan_lds_bytes(int block) { return (kChunk + 1) * (block / 64 * 8 + 8 + 1) * (int)sizeof(double2); }

inline int64_t rec_bytes(int64_t n) { return up256((n + 2) * 48) + 256; }
inline int64_t partial_bytes(int64_t nf, int ht, int parts) { return parts > 1 ? (int64_t)parts * 2 * ht * nf * 8 : 0; }

// The automatic parts rule over `tiles` workgroups per part: two workgroups per CU where the tiles alone do not give
// them, while a part keeps at least kMinChunks chunks.  (An empty grid counts as one tile: callers launch nothing then.)
inline int64_t auto_parts(int64_t n, int64_t tiles, int cus) {
    if (tiles < 1) tiles = 1;
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    const int64_t want = (2 * (int64_t)cus + tiles - 1) / tiles, keep = chunks / kMinChunks;
    return want < keep ? want : keep;
}

inline int ht_validate(int64_t n, double delta, int64_t j_begin, int64_t nf, int nharm, int parts, bool any_output) {
    PDC_REQUIRE(n >= 1, "htest: at least one event is needed (got %lld)", (long long)n);
    PDC_REQUIRE(nf >= 0 && j_begin >= 0, "htest: negative size");
    PDC_REQUIRE(nharm >= 1 && nharm <= kMaxHarm, "htest: nharm must be 1 .. %d (got %d)", kMaxHarm, nharm);
    PDC_REQUIRE(parts >= 0, "htest: parts must be >= 0 (got %d)", parts);
    PDC_REQUIRE(std::isfinite(delta) && delta > 0.0, "htest: the grid step must be finite and positive");
    PDC_REQUIRE(any_output, "htest: every output is NULL");
    PDC_REQUIRE((nf + kTile - 1) / kTile < ((int64_t)1 << 31), "htest: grid too large");
    return PDC_OK;
}

// The prep launch: records at `work`, sum w^2 right after them (rec_bytes(n) in all).
inline int ht_enqueue_prep(hipStream_t st, const double *d_t, const double *d_w, int64_t n, double delta, void *work,
                           HtPrepArgs &p) {
    p.t = d_t;
    p.w = d_w;
    p.n = n;
    p.delta = delta;
    p.rec = static_cast<double *>(work);
    p.scal = reinterpret_cast<double *>(static_cast<char *>(work) + up256((n + 2) * 48));
    hipLaunchKernelGGL(htest_prep_kernel, dim3(1), dim3(kPrepBlock), 0, st, p);
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

}  // namespace
