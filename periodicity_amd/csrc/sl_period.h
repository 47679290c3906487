// Shared by the one-workgroup-per-period StringLength kernels of stringlength.hip and sl_ragged.inc (inside the
// anonymous namespace of the unit): sl_scan_kernel, sl_fast_kernel, sl_duo_kernel, sl_duo_ragged_kernel, the one-cycle
// and prep kernels and their slr:: counterparts.  One definition of every phase of a period, each taking what it
// uses as parameters:
//   PeriodLds           the dynamic LDS block of a period, carved once (host launchers size it from the same type)
//   (sl_p1.inc)         P1: fold, coarse histogram, bucket ids in registers - text in the kernel bodies: see there
//   permute             P2: the permutation order[], grouped by coarse bucket (duo kernels; sl_fast_kernel types it out)
//   range_table         the range table of a slice of buckets [b0, b1)
//   walk_ranges         P3a: wave-autonomous ranges (its lambdas: sl_p3a.inc, which sl_fast_kernel includes itself)
//   sort_deferred_lds   P3b: a deferred range of <= DCAP samples, bitonic-sorted in LDS by the whole workgroup
//   links_and_total     P3c: links between non-empty ranges, the closing segment, the workgroup's total
//   duo_period          one period of the two- / four-workgroups-per-CU kernels, from a DuoCurve
//   is_one_cycle, onecycle_sum, prep_sample   the bodies of the one-cycle pre-pass and of the prep kernels
// Every function is __device__ __forceinline__; a kernel's summation order (hence its bits) is decided by its block size,
// a template parameter wherever it matters.
// `tid` is the CALLER's opaque copy of the thread id (asm volatile("" : "+v"(tid)), once per period): addresses and
// masks built from it are not hoisted out of the period loop and spilled, in the phase or in the caller's later use.
#pragma once

constexpr int kBuckets = 2048;       // coarse buckets over [0, 1]
constexpr int kBucketsLarge = 8192;  // ... for N >= 65536, so that a bucket still fits a wave's range
constexpr int kBlock = 1024;
constexpr int kWaves = kBlock / 64;
constexpr int kWin = 192;        // sorted positions per range window
constexpr int kRCap = 256;       // samples a wave sorts by itself (4 per lane)
constexpr int kRPer = kRCap / 64;
constexpr int kWFine = 256;      // fine buckets per wave range
constexpr int kCPL = kWFine / 64; // fine counters per lane (multiple of 4)
constexpr int kWInsertMax = 16;  // fullest fine bucket the predecessor-counting finish accepts
constexpr int kDCap = 2048;      // workgroup-level (deferred) LDS sort capacity
constexpr int kMaxRanges = 1024; // ranges per slice
constexpr int kMaxGrid = 1024;
constexpr int kLdsTotal = 163840;

template <typename IdxT>
struct Lds {
    // per wave: keys u64[kRCap] | fine u32[kWFine + 4] | idx IdxT[kRCap]
    static constexpr int wave_bytes = ((kRCap * 8 + (kWFine + 4) * 4 + kRCap * (int)sizeof(IdxT)) + 15) & ~15;
    // the coarse histogram is only alive in P1/P2 and the wave scratch only in P3: they share LDS
    static constexpr int fixed = kWaves * wave_bytes + (kMaxRanges + 8) * 4 + 128;
    static constexpr int capacity = (kLdsTotal - fixed - 1024) / (int)sizeof(IdxT);  // slice size
    static_assert(kWaves * wave_bytes >= kDCap * (8 + (int)sizeof(IdxT)), "deferred sort must fit");
    static_assert(capacity / kWin + 1 <= kMaxRanges, "range table too small");
    static_assert(capacity < 65536, "slice positions are stored as 16-bit offsets");
};

// LDS traffic between lanes of ONE wave: order the accesses without a workgroup barrier.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Exclusive prefix sum of a[0..NB) in place (NB / BLOCK entries per thread); returns the total.
template <int NB, int BLOCK = kBlock>
__device__ __forceinline__ unsigned scan_buckets(unsigned *a, unsigned *wave_tot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int per = NB / BLOCK;
    static_assert(per * BLOCK == NB, "bucket count must be a multiple of the block size");
    unsigned local[per], sum = 0;
#pragma unroll
    for (int e = 0; e < per; ++e) {
        local[e] = a[tid * per + e];
        sum += local[e];
    }
    unsigned incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    __syncthreads();
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned run = incl - sum, all = 0u;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        if (w < wave) run += wave_tot[w];
        all += wave_tot[w];
    }
#pragma unroll
    for (int e = 0; e < per; ++e) {
        a[tid * per + e] = run;
        run += local[e];
    }
    __syncthreads();
    return all;
}

// Ascending bitonic sort of P (power of two) (key, index) pairs by (key, index), whole workgroup.
template <typename IdxT, typename KeyPtr, typename IdxPtr>
__device__ __forceinline__ void bitonic_sort(KeyPtr K, IdxPtr I, int P) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int c = threadIdx.x; c < (P >> 1); c += (int)blockDim.x) {
                const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
                const int l = i | j;
                const unsigned long long ka = K[i], kb = K[l];
                const IdxT ia = I[i], ib = I[l];
                const bool up = (i & k) == 0;
                const bool a_gt_b = ka > kb || (ka == kb && ia > ib);
                if (a_gt_b == up) {
                    K[i] = kb;
                    K[l] = ka;
                    I[i] = ib;
                    I[l] = ia;
                }
            }
            __syncthreads();
        }
    }
}

// Sum of hypot(dm, dphi) over consecutive sorted points j-1 -> j, j in [1, cnt), whole workgroup.
template <typename KeyPtr, typename IdxPtr>
__device__ __forceinline__ double segment_sum(KeyPtr K, IdxPtr I, int cnt, const double *m) {
    const int lane = threadIdx.x & 63;
    double total = 0.0;
    for (int j0 = 0; j0 < cnt; j0 += (int)blockDim.x) {
        const int j = j0 + threadIdx.x;
        const bool live = j < cnt;
        double phi = 0.0, mm = 0.0;
        if (live) {
            phi = __longlong_as_double((long long)K[j]);
            mm = m[I[j]];
        }
        double pphi = __shfl_up(phi, 1, 64);
        double pm = __shfl_up(mm, 1, 64);
        bool ok = live;
        if (lane == 0 && live) {
            if (j > 0) {
                pphi = __longlong_as_double((long long)K[j - 1]);
                pm = m[I[j - 1]];
            } else {
                ok = false;
            }
        }
        if (ok) total += hypot(mm - pm, phi - pphi);
    }
    return total;
}

namespace fast {

constexpr int kNB = kBuckets;
constexpr int kFWin = 216;             // sorted positions per range window (a range = window + < one bucket)
constexpr int kFCap = 255;             // samples a wave ranks by itself: counts and starts fit in bytes
constexpr int kFine = 1024;            // fine buckets per range, 8-bit counters packed four to a word
static_assert(kFine + 16 <= (kWFine + 4) * 4, "byte counters live in the general kernel's counter area");

typedef double rec_t __attribute__((ext_vector_type(2)));   // (t, m)

// RN(t / period) without the division: y = RN(1 / period); q0 = RN(t y) is within 1.5 ulp of the
// quotient, one fma correction makes it faithful, and for a faithful q and a correctly rounded
// reciprocal Markstein's theorem (IBM J. Res. Dev. 34, 1990; Muller et al., Handbook of
// Floating-Point Arithmetic, "division with an FMA") says the second correction IS the correctly
// rounded quotient.  The theorem needs no over/underflow and a divisor whose significand is not all
// ones: `safe` (wave-uniform) says so, otherwise the IEEE division runs.
__device__ __forceinline__ double exact_quotient(double t, double period, double y, bool safe) {
    if (!safe) return t / period;
    const double q0 = t * y;
    const double r0 = __builtin_fma(-period, q0, t);
    const double q1 = __builtin_fma(r0, y, q0);
    const double r1 = __builtin_fma(-period, q1, t);
    return __builtin_fma(r1, y, q1);
}

__device__ __forceinline__ bool period_is_safe(double period, bool t_safe) {
    const double ap = __builtin_fabs(period);
    const unsigned long long frac = (unsigned long long)__double_as_longlong(period) & 0xFFFFFFFFFFFFFull;
    return t_safe && ap >= 1e-150 && ap <= 1e150 && frac != 0xFFFFFFFFFFFFFull;
}

// ((t - 0) / period) % 1 as numpy computes it (core.py:544); NaN when the quotient is not finite.
__device__ __forceinline__ double fast_phase(double t, double period, double y, bool safe) {
    const double q = exact_quotient(t, period, y, safe);
    return q - __builtin_floor(q);
}

__device__ __forceinline__ unsigned long long phase_key(double phi) {
    // monotone for phi in [0, 1]; every NaN gets one pattern, above all numbers, so that NaN phases
    // keep their time order (stable sort)
    return phi == phi ? (unsigned long long)__double_as_longlong(phi) : 0x7FF8000000000000ull;
}

// the bits of a double as they sit in the 64-bit key array
__device__ __forceinline__ unsigned long long key_bits(double x) { return (unsigned long long)__double_as_longlong(x); }

template <int NB = kNB>
__device__ __forceinline__ int coarse_of(double phi) {
    const unsigned b = (unsigned)(phi * (double)NB);            // exact product; v_cvt_u32 saturates
    const unsigned c = b < (unsigned)(NB - 1) ? b : (unsigned)(NB - 1);
    return phi == phi ? (int)c : NB - 1;
}

// Wave-wide inclusive scan / maximum by DPP row shifts and row broadcasts (gfx9 encodings: row_shr:n =
// 0x110 + n, row_bcast15 = 0x142, row_bcast31 = 0x143); no LDS permutes.  The maximum ends in lane 63.
#define PDC_DPP(old, src, ctrl, rmask) \
    (unsigned)__builtin_amdgcn_update_dpp((int)(old), (int)(src), (ctrl), (rmask), 0xf, false)
__device__ __forceinline__ unsigned wave_scan_add(unsigned v) {
    v += PDC_DPP(0u, v, 0x111, 0xf);
    v += PDC_DPP(0u, v, 0x112, 0xf);
    v += PDC_DPP(0u, v, 0x114, 0xf);
    v += PDC_DPP(0u, v, 0x118, 0xf);
    v += PDC_DPP(0u, v, 0x142, 0xa);
    v += PDC_DPP(0u, v, 0x143, 0xc);
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {   // valid in lane 63 -> broadcast
    unsigned u;
    u = PDC_DPP(0u, v, 0x111, 0xf); v = u > v ? u : v;
    u = PDC_DPP(0u, v, 0x112, 0xf); v = u > v ? u : v;
    u = PDC_DPP(0u, v, 0x114, 0xf); v = u > v ? u : v;
    u = PDC_DPP(0u, v, 0x118, 0xf); v = u > v ? u : v;
    u = PDC_DPP(0u, v, 0x142, 0xa); v = u > v ? u : v;
    u = PDC_DPP(0u, v, 0x143, 0xc); v = u > v ? u : v;
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// Wave-wide sum of doubles in a FIXED order (the scan pattern above on both halves of the double; the
// total ends in lane 63 and is broadcast): no LDS permutes on the critical path of a range.
#define PDC_DPP_F64(v, ctrl, rmask)                                                                          \
    __longlong_as_double(((long long)PDC_DPP(0u, (unsigned)(__double_as_longlong(v) >> 32), ctrl, rmask) << 32) | \
                         (long long)PDC_DPP(0u, (unsigned)__double_as_longlong(v), ctrl, rmask))
__device__ __forceinline__ double wave_sum_fixed(double v) {
    v += PDC_DPP_F64(v, 0x111, 0xf);
    v += PDC_DPP_F64(v, 0x112, 0xf);
    v += PDC_DPP_F64(v, 0x114, 0xf);
    v += PDC_DPP_F64(v, 0x118, 0xf);
    v += PDC_DPP_F64(v, 0x142, 0xa);
    v += PDC_DPP_F64(v, 0x143, 0xc);
    const long long b = __double_as_longlong(v);
    return __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(b >> 32), 63) << 32) |
                                (unsigned)__builtin_amdgcn_readlane((int)b, 63));
}

// x of the lane below (lane 0: `first`), by DPP wave_shr:1 on both halves - no LDS permute
__device__ __forceinline__ double lane_below(double x, double first) {
    const long long xb = __double_as_longlong(x), fb = __double_as_longlong(first);
    const int lo = __builtin_amdgcn_update_dpp((int)fb, (int)xb, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(fb >> 32), (int)(xb >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double read_lane(double x, int l) {   // l wave-uniform
    const long long xb = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)xb, l), hi = __builtin_amdgcn_readlane((int)(xb >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// sqrt(x^2 + y^2) for |x|, |y| <= ~1e150 whose squares do not underflow to a subnormal that matters:
// here |dm| <= 0.5 and |dphi| <= 1.  rsq seed, one coupled Goldschmidt step, one Newton step.
__device__ __forceinline__ double short_hypot(double x, double y) {
    const double s = __builtin_fma(x, x, y * y);
    const double r = __builtin_amdgcn_rsq(s);
    const double g0 = s * r, h0 = 0.5 * r;
    const double e0 = __builtin_fma(-h0, g0, 0.5);
    const double g1 = __builtin_fma(g0, e0, g0), h1 = __builtin_fma(h0, e0, h0);
    const double d1 = __builtin_fma(-g1, g1, s);
    const double g2 = __builtin_fma(d1, h1, g1);
    return (s > 0.0 && s < __builtin_inf()) ? g2 : s;        // 0, +inf and NaN pass through
}

// Four phases at once: ONE wave-uniform branch on `safe` per group, so that the four dependent fma
// chains sit in one basic block and overlap.
__device__ __forceinline__ void phases4(const double (&t)[4], double period, double y, bool safe,
                                        double (&phi)[4]) {
    double q[4];
    if (safe) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double q0 = t[u] * y;
            const double r0 = __builtin_fma(-period, q0, t[u]);
            const double q1 = __builtin_fma(r0, y, q0);
            const double r1 = __builtin_fma(-period, q1, t[u]);
            q[u] = __builtin_fma(r1, y, q1);
        }
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = t[u] / period;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) phi[u] = q[u] - __builtin_floor(q[u]);
}

// ---- the dynamic LDS block of one period -------------------------------------------------------------------------
//   [WAVES x WAVE_BYTES]  P3a: per-wave scratch (keys u64[kRCap] | fine u32[kWFine + 4] | idx IdxT[kRCap]); the coarse
//                         histogram (P1/P2, [NB + 64]: 64 dummy buckets for samples past the end) and the deferred sort's
//                         keys and indices (P3b, [DCAP] each) alias it - each alive in its own phase only
//   [2 x (RANGES + 8)]    range table: first bucket / first sorted position of every range, 16-bit
//   [16]                  defer: bits of the deferred ranges in [0..14], [15] the next range to hand out (P3a)
//   [slice + 64]          order: the permutation (64 dummy slots behind it)
template <typename IdxT, int WAVES, int WAVE_BYTES, int RANGES, int DCAP>
struct PeriodLds {
    typedef IdxT idx_t;
    static constexpr int waves = WAVES, dcap = DCAP;
    static constexpr int fixed = WAVES * WAVE_BYTES + 2 * (RANGES + 8) * 2 + 64;
    static_assert(WAVES * WAVE_BYTES >= DCAP * (8 + (int)sizeof(IdxT)), "aliases must fit: the deferred sort");
    static_assert(RANGES <= 15 * 32, "deferred-range bits live in defer[0..14]");
    template <int NB>
    static constexpr bool holds_histogram = WAVES * WAVE_BYTES >= (NB + 64) * 4;
    // entries of order[] for a slice (the 64 dummy slots, rounded up to 16 bytes), and the bytes of the whole block
    static constexpr int64_t order_entries(int64_t slice) { return (slice + 64 + 7) & ~(int64_t)7; }
    static constexpr size_t bytes(int64_t slice) { return (size_t)fixed + (size_t)order_entries(slice) * sizeof(IdxT); }

    unsigned *hist;                  // P1/P2 alias
    unsigned long long *bkeys;       // P3b alias
    IdxT *bidx;                      // P3b alias
    unsigned short *bndb, *bnds;
    unsigned *defer;
    IdxT *order;
    unsigned long long *keys_w;      // this wave's scratch
    unsigned *fine_w;
    IdxT *idx_w;

    static __device__ __forceinline__ PeriodLds carve(unsigned char *lds_raw, int wave) {
        PeriodLds v;
        v.hist = reinterpret_cast<unsigned *>(lds_raw);
        v.bkeys = reinterpret_cast<unsigned long long *>(lds_raw);
        v.bidx = reinterpret_cast<IdxT *>(v.bkeys + DCAP);
        v.bndb = reinterpret_cast<unsigned short *>(lds_raw + WAVES * WAVE_BYTES);
        v.bnds = v.bndb + RANGES + 8;
        v.defer = reinterpret_cast<unsigned *>(v.bnds + RANGES + 8);
        v.order = reinterpret_cast<IdxT *>(v.defer + 16);
        v.keys_w = reinterpret_cast<unsigned long long *>(lds_raw + wave * WAVE_BYTES);
        v.fine_w = reinterpret_cast<unsigned *>(lds_raw + wave * WAVE_BYTES + kRCap * 8);
        v.idx_w = reinterpret_cast<IdxT *>(lds_raw + wave * WAVE_BYTES + kRCap * 8 + (kWFine + 4) * 4);
        return v;
    }
};

// the sample at a position of the permutation, as it stands in order[]
template <typename IdxT>
struct OrderPlain {
    const IdxT *order;
    __device__ __forceinline__ unsigned operator()(int pos) const { return (unsigned)order[pos]; }
};

// a workgroup's range scratch (global): the 4-double summary {first phi, first m, last phi, last m}, the sample count
// and the string length inside every range
struct RangeScratch {
    double *rsum;
    int *rcnt;
    double *rlen;
};

// ---- P2: the permutation, grouped by coarse bucket, from the bucket ids of P1 (t[] is not touched again) ------------
// On return (after the caller's barrier) hist[b] = END position of bucket b.
template <int KMAX, int BLK, int G, typename L>
__device__ __forceinline__ void permute(const L &v, const unsigned (&pk)[(KMAX + 1) / 2], int n, int tid, int lane) {
    typedef typename L::idx_t IdxT;
#pragma unroll
    for (int k0 = 0; k0 < KMAX; k0 += G) {
        if (k0 * BLK < n) {   // workgroup-uniform
            unsigned pos[G];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (k0 + u < KMAX) {
                    const unsigned b = (pk[(k0 + u) >> 1] >> (((k0 + u) & 1) * 16)) & 0xFFFFu;
                    pos[u] = atomicAdd(&v.hist[b], 1u);
                }
            }
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (k0 + u < KMAX) {
                    const int i = (k0 + u) * BLK + tid;
                    v.order[i < n ? pos[u] : (unsigned)(n + lane)] = (IdxT)i;
                }
            }
        }
    }
}

// ---- the range table of the slice of buckets [b0, b1), whose slice_n samples start at sorted position `consumed` ----
// (one slice: (0, NB, 0)).  Range r starts at the first bucket whose start position is >= consumed + r * kFWin.
// Barriers: before (hist[b] = END position of bucket b) and after (the histogram is dead from there on: its LDS becomes
// wave scratch).
template <int BLK, typename L>
__device__ __forceinline__ void range_table(const L &v, int b0, int b1, int consumed, int slice_n, int nranges, int tid) {
    __syncthreads();
    for (int r = tid; r <= nranges; r += BLK) {
        int b = b0, s0 = 0;
        if (r > 0) {
            const unsigned x = (unsigned)consumed + (unsigned)r * kFWin;
            int l = b0, h = b1;   // smallest j in [b0, b1) with end(j) >= x, b1 if none
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (v.hist[mid] >= x) h = mid; else l = mid + 1;
            }
            b = l < b1 ? l + 1 : b1;
            s0 = l < b1 ? (int)v.hist[l] - consumed : slice_n;
        }
        v.bndb[r] = (unsigned short)b;
        v.bnds[r] = (unsigned short)s0;
    }
    __syncthreads();
}

// ---- P3a: wave-autonomous ranges -----------------------------------------------------------------------------------
// One wave's walk over the ranges of a slice (no workgroup barrier inside): `wave` first, then whatever the ticket in
// defer[15] hands out.  `request` fetches the records of a range one range ahead of their use, `process` ranks and
// sums one range; the read-ahead state (n_cnt .. r_next) lives between them.
//   order_get(pos)   the sample at a slice position: OrderPlain, or the 16 bits + planes of sl_fast_kernel's PL > 0
//                    instances
//   rec, n           the curve's (t, m) records (n: the double-gather experiment only)
//   rs, r_base       the workgroup's range scratch and this slice's first slot in it
//   EMIT             besides the length, the sorted (phase, m) records go to emit_row[emit_at + position in the slice] -
//                    the Supersmoother's sort reuses the kernel and wants the sorted curve itself
// (Inner lambdas over local state - as a struct with member functions the same statements cost sl_fast_kernel a VGPR in
// five instances - and the lambdas are sl_p3a.inc, which sl_fast_kernel includes instead of calling this: DESIGN 4.3c.)
template <typename IdxT, int NB, bool EMIT, typename L, typename OrderGet>
__device__ __forceinline__ void walk_ranges(const L &v, OrderGet order_get, const rec_t *rec, int n,
                                            const RangeScratch &rs, int r_base, int nranges, double period, double y,
                                            bool safe, int lane, int wave, rec_t *emit_row, int emit_at) {
    const unsigned short *const bndb = v.bndb, *const bnds = v.bnds;
    unsigned *const defer = v.defer;
    unsigned long long *const keys_w = v.keys_w;
    unsigned *const fine_w = v.fine_w;
    IdxT *const idx_w = v.idx_w;
#include "sl_p3a.inc"
    if (wave < nranges) request(wave);
    for (int r = wave; r < nranges; r = r_next) {
        if (n_cnt > 192) process(r, std::true_type{});
        else process(r, std::false_type{});
    }
}


// ---- P3b: one deferred range of cnt <= DCAP samples (slice positions [s_lo, s_lo + cnt)), whole workgroup ------------
// Pads to a power of two, bitonic-sorts (key, index) in LDS, adds the segments inside the range (returned: this
// thread's share) and leaves the range's summary in `ends`.  key_of(t): the 64-bit sort key of a sample's phase - the
// kernel's own fold.  EMIT: the sorted (phase, m) records go to emit_to[0 .. cnt).
template <int BLK, bool EMIT, typename IdxT, typename OrderGet, typename KeyOf>
__device__ __forceinline__ double sort_deferred_lds(unsigned long long *bkeys, IdxT *bidx, OrderGet order_get, int s_lo,
                                                    int cnt, const double *t, const double *m, KeyOf key_of, int tid,
                                                    rec_t *emit_to, double (&ends)[4]) {
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int s = tid; s < P; s += BLK) {
        if (s < cnt) {
            const IdxT id = (IdxT)order_get(s_lo + s);
            bkeys[s] = key_of(t[id]);
            bidx[s] = id;
        } else {
            bkeys[s] = ~0ull;
            bidx[s] = (IdxT)~0u;
        }
    }
    __syncthreads();
    bitonic_sort<IdxT>(bkeys, bidx, P);
    const double inside = segment_sum(bkeys, bidx, cnt, m);
    if constexpr (EMIT)
        for (int s = tid; s < cnt; s += BLK) {
            rec_t o;
            o.x = __longlong_as_double((long long)bkeys[s]);
            o.y = m[bidx[s]];
            emit_to[s] = o;
        }
    ends[0] = __longlong_as_double((long long)bkeys[0]);
    ends[1] = m[bidx[0]];
    ends[2] = __longlong_as_double((long long)bkeys[cnt - 1]);
    ends[3] = m[bidx[cnt - 1]];
    return inside;
}

// ---- P3c: links between consecutive non-empty ranges + the closing segment, then the workgroup's total --------------
// `total`: this thread's share so far.  Thread tid adds ranges tid, tid + BLK, ...: the block size decides the summation
// order.  ADD_RLEN: the lengths inside the ranges are in rlen[] (sl_scan_kernel adds them to `total` as it goes).
// Returns the period's string length in thread 0 (0 elsewhere); the caller's barrier frees red[].
template <int BLK, bool ADD_RLEN>
__device__ __forceinline__ double links_and_total(double total, const double *rsum, const int *rcnt, const double *rlen,
                                                  int nr, int tid, int lane, int wave, double *red) {
    for (int r = tid; r < nr; r += BLK) {
        if (rcnt[r] > 0) {
            if constexpr (ADD_RLEN) total += rlen[r];
            int q = r - 1;
            while (q >= 0 && rcnt[q] == 0) --q;
            if (q >= 0)
                total += hypot(rsum[(int64_t)r * 4 + 1] - rsum[(int64_t)q * 4 + 3],
                               rsum[(int64_t)r * 4 + 0] - rsum[(int64_t)q * 4 + 2]);
        }
    }
    if (tid == 0 && nr > 0) {
        int f0 = 0, l0 = nr - 1;
        while (f0 < nr && rcnt[f0] == 0) ++f0;
        while (l0 >= 0 && rcnt[l0] == 0) --l0;
        // closing segment of np.roll(-1): first minus last, no phase wrap (phase.py:50)
        if (f0 < nr && l0 >= 0)
            total += hypot(rsum[(int64_t)f0 * 4 + 1] - rsum[(int64_t)l0 * 4 + 3],
                           rsum[(int64_t)f0 * 4 + 0] - rsum[(int64_t)l0 * 4 + 2]);
    }
    total = wave_sum(total);
    if (lane == 0) red[wave] = total;
    __syncthreads();
    double sum = 0.0;
    if (tid == 0)
        for (int w = 0; w < BLK / 64; ++w) sum += red[w];
    return sum;
}

// ---- one period of the two- / four-workgroups-per-CU kernels (namespace duo) ----------------------------------------
// The curve a period belongs to: the single call's one curve, or the ragged batch's curve of the ticket.
struct DuoCurve {
    const double *t, *m;
    const rec_t *rec;
    const double *periods;
    double *ell;
    unsigned char *todo;    // [periods]: 1 = left to the one-workgroup kernel
    int n;
    bool t_safe;            // every t is 0 or 1e-150 <= |t| <= 1e150
    unsigned *marked;       // the counter of periods left to the one-workgroup kernel
};

// A period from P2 on: P2, the range table, P3a, P3b (LDS sort; a deferred range beyond L::dcap marks the period), P3c
// and the period's result: ell[p], or todo[p] = 1 and one more in *marked.  P1 has run in the calling kernel's body
// (sl_p1.inc) for this period, y and safe: pk[] holds its bucket ids, hist[] the bucket starts, and `tid` is the opaque
// copy of the thread id that P1 used.  Same algorithm, arithmetic and summation order per range as sl_fast_kernel's
// one-slice instances.  red ([BLK / 64]) and s_bad (zeroed by the caller with the ticket) are the kernel's static LDS.
template <int KMAX, int BLK, int NBL, typename L>
__device__ __forceinline__ void duo_period(const DuoCurve &c, int64_t p, double period, double y, bool safe, int tid,
                                           const unsigned (&pk)[(KMAX + 1) / 2], const L &v, const RangeScratch &rs,
                                           double *red, unsigned *s_bad, int lane, int wave) {
    typedef typename L::idx_t IdxT;
    const int n = c.n;
    double total = 0.0;

    permute<KMAX, BLK, 4>(v, pk, n, tid, lane);
    const int nranges = (n + kFWin - 1) / kFWin;
    range_table<BLK>(v, 0, NBL, 0, n, nranges, tid);

    // ---- P3a: wave-autonomous ranges (this workgroup's BLK / 64 waves) --------------------------------------
    const OrderPlain<IdxT> order_get{v.order};
    walk_ranges<IdxT, NBL, false>(v, order_get, c.rec, n, rs, 0, nranges, period, y, safe, lane, wave, nullptr, 0);
    __syncthreads();

    // ---- P3b: deferred ranges, whole workgroup (LDS sort; larger ones mark the period) ----------
    auto key_of = [&](double tv) { return phase_key(fast_phase(tv, period, y, safe)); };
    for (int w32 = 0; w32 < (nranges + 31) / 32; ++w32) {
        unsigned bits = v.defer[w32];
        while (bits) {
            const int r = w32 * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            const int s_lo = v.bnds[r], cnt = (int)v.bnds[r + 1] - s_lo;
            if (cnt > L::dcap) {      // (workgroup-uniform)
                if (tid == 0) *s_bad = 1u;
                continue;
            }
            double ends[4];
            total += sort_deferred_lds<BLK, false>(v.bkeys, v.bidx, order_get, s_lo, cnt, c.t, c.m, key_of, tid, nullptr,
                                                   ends);
            if (tid == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) rs.rsum[(int64_t)r * 4 + k] = ends[k];
                rs.rcnt[r] = cnt;
                rs.rlen[r] = 0.0;   // (its segments were added to `total` by the whole workgroup, in a fixed order)
            }
            __syncthreads();
        }
    }
    __syncthreads();  // every summary of this item (global, this workgroup's) is visible

    const double sum = links_and_total<BLK, true>(total, rs.rsum, rs.rcnt, rs.rlen, nranges, tid, lane, wave, red);
    if (tid == 0) {
        c.todo[p] = *s_bad ? 1 : 0;
        if (*s_bad) atomicAdd(c.marked, 1u);
        else c.ell[p] = sum;
    }
}

// ---- periods of ONE cycle, and the prep kernels' per-sample work ----------------------------------------------------
// The samples span less than one cycle of `period`: all in one, or the later ones in the next with phases BELOW the
// first sample's - sorted order = those, then the earlier ones, each as they stand: the same segments, the pair across
// the cycle boundary being the closing one.  NaN: no.  bad0 / bad1: sl_tame_kernel's words (some |t| outside {0} u
// [1e-150, 1e150]; t not non-decreasing).  (t[] is read only when n >= 2.)
__device__ __forceinline__ bool is_one_cycle(const double *t, int64_t n, double period, unsigned bad0, unsigned bad1) {
    if (bad1 != 0u || n < 2) return false;
    const double y = 1.0 / period;
    const bool safe = period_is_safe(period, bad0 == 0u);
    const double q0 = exact_quotient(t[0], period, y, safe), q1 = exact_quotient(t[n - 1], period, y, safe);
    const double c0 = __builtin_floor(q0), c1 = __builtin_floor(q1);
    return period > 0.0 && (c1 - c0 == 0.0 || (c1 - c0 == 1.0 && q1 - c1 < q0 - c0));
}

// The string length of a one-cycle period, the segments summed as the samples stand, by a workgroup of BLOCK threads
// (the reduction shape - hence the bits - is BLOCK's: per-thread strides, wave_sum_fixed, the waves in order, then the
// closing segment).  Valid in thread 0; the caller's barrier frees red[BLOCK / 64].
template <int BLOCK>
__device__ __forceinline__ double onecycle_sum(const double *t, const double *m, int64_t n, double period, bool safe,
                                               double *red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double y = 1.0 / period;
    double acc = 0.0;
    for (int64_t i = tid + 1; i < n; i += BLOCK) {        // segment (i - 1, i)
        const double p1 = fast_phase(t[i], period, y, safe), p0 = fast_phase(t[i - 1], period, y, safe);
        acc += short_hypot(m[i] - m[i - 1], p1 - p0);
    }
    acc = wave_sum_fixed(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    double total = 0.0;
    if (tid == 0) {
        for (int x = 0; x < BLOCK / 64; ++x) total += red[x];
        // closing segment of np.roll(-1): first minus last, no phase wrap (phase.py:50)
        total += hypot(m[0] - m[n - 1], fast_phase(t[0], period, y, safe) - fast_phase(t[n - 1], period, y, safe));
    }
    return total;
}

// What the prep kernels make of sample i: its (t, m) record (returned, and stored to rec[i] unless rec is NULL), and
// the two flags OR-ed over a curve - wild: |t| outside {0} u [1e-150, 1e150] (exact_quotient's shortcut is off);
// unsorted: t[i - 1] <= t[i] does not hold (NaN counts).
struct PrepFlags {
    bool wild = false, unsorted = false;
};
__device__ __forceinline__ rec_t prep_sample(const double *t, const double *m, int64_t i, rec_t *rec, PrepFlags &f) {
    const double tv = t[i];
    rec_t v;
    v.x = tv;
    v.y = m[i];
    if (rec) rec[i] = v;
    const double at = __builtin_fabs(tv);
    f.wild = f.wild || !(at == 0.0 || (at >= 1e-150 && at <= 1e150));
    f.unsorted = f.unsorted || (i > 0 && !(t[i - 1] <= tv));
    return v;
}

}  // namespace fast
