// Device-side peak picking for FSeries consumers, for a batch of spectra resident in HBM.
//
// highest_peak*: FSeries.period_at_highest_peak (upstream core.py:952-955) = find_peaks (core.py:283-317) =
// scipy.signal.find_peaks(values, prominence=0.0) = scipy's _local_maxima_1d, then the NaN-aware maximum over those
// peaks (core.py:202-220, first maximum on ties).
//
// scipy's rule, restated: i is the left edge of a peak when x[i-1] < x[i]; walk right over the flat top while
// x[j] == x[i]; it is a peak only if the sample after the flat top is lower, and the reported index is the midpoint
// (left + right) // 2 of the flat top.  The first and last sample are never peaks; comparisons with NaN are false, so
// NaN is never part of one.
//
// peaks_topk_kernel<SORT>: all find_peaks() maxima with their scipy prominences (scipy.signal.peak_prominences,
// wlen=None: walk left and right from the peak while x[i] <= x[peak], remember the lowest sample on each side,
// prominence = x[peak] - max of the two), ranked by height (psort_by_peak, core.py:944-946) or by prominence
// (psort_by_prominence :948-950, period_at_highest_prominence :957-961); the first k come back, together with the two
// sign changes of x - (x[peak] - key/2) that periods_at_half_max (:963-978) looks up: the last one left of the peak and
// the first one from the peak rightwards (np.diff(np.signbit(..)), core.py:362).  Equal heights / prominences rank the
// lower bin first - a documented deviation: upstream's argsort()[::-1] is an unstable sort read
// backwards, which for short arrays puts the HIGHER bin first; the host-side FSeries methods run numpy as upstream does.
//
// One workgroup per spectrum.  Only k peaks are wanted, and walking every maximum (6300 per 5e4-bin row) is not needed
// to rank them:
//   * prominence <= height - (lowest sample of the row): a maximum with  height - lowest < tau  cannot be among the k
//     most prominent once k prominences >= tau are known;
//   * ranked by height, only the k winners need a prominence at all.
// A call of k > kPkMaxK ranks runs as launches of kPkMaxK, each ranking what comes AFTER the last winner of the launch
// before in the total order (key descending, bin ascending); a maximum collected twice is reported once.
//
// Decomposition (everything __device__ __forceinline__: the walks as one real function cost scratch at every call and
// 30 % of the sweep)
//   dpp_double, readlane_double, wave_min_to_lane63<T>   a double through DPP / readlane as two 32-bit halves
//   cand_before, after, fold_best     the total order (key descending, bin ascending; bin -1: no entry)
//   TopkLds, TopkFixed<SORT>          the dynamic LDS block (block extrema, candidate list), carved once; the fixed arrays
//   wave_extrema                      minimum / maximum of a block over the wave; a block holding a NaN has bmax = +inf
//   block_min                         minimum of a per-thread double over the workgroup
//   run<DIR>, walk<DIR>               lowest sample met from a bin on while x[i] <= h, sixteen lanes per walk, hopping
//                                     over the blocks whose extrema cannot stop it
//   walk_candidates                   prominences of the candidates that have none: one group per candidate (> 16 of
//                                     them), else left and right walks side by side on the two halves of the workgroup
//   best_after                        a lane's best entry strictly after the previous winner: both phases of a few-ranks ranking
//   chunk_max                         highest block maximum over a chunk: the second sweep's mask and its loop
//   half_max<GROUP>                   the two half-maximum crossings of every ranked peak, GROUP lanes per peak
// peaks_topk_kernel holds the rest.  The standing rule of gls_sums.h applies: both instances sit at an occupancy edge (80
// and 96 registers), and four pieces are text, each with its cost beside it: the separate block-extrema pass, the
// rankings and the sweep as lambdas inside the kernel, and scipy's flat-top rule in highest_peak_kernel and in the sweep
// (profiles/r24_peaks_ab.txt).
#include <type_traits>

#include "pdc_internal.h"

using namespace pdc;

namespace {

constexpr int kBlock = 256;

// a double through DPP as its two 32-bit halves (lanes without a source keep `old`)
template <int CTRL>
__device__ __forceinline__ double dpp_double(double old, double src) {
    const long long ob = __double_as_longlong(old), sb = __double_as_longlong(src);
    const int lo = __builtin_amdgcn_update_dpp((int)ob, (int)sb, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(ob >> 32), (int)(sb >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
template <int CTRL>
__device__ __forceinline__ int dpp_value(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ double dpp_value(double v) { return dpp_double<CTRL>(v, v); }

__device__ __forceinline__ double readlane_double(double v, int lane) {
    const long long b = __double_as_longlong(v);
    return __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(b >> 32), lane) << 32) |
                                (unsigned)__builtin_amdgcn_readlane((int)b, lane));
}

// minimum over the wave, valid in lane 63: row shifts and row broadcasts (DPP), no LDS traffic
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_min(T v) {
    const T o = dpp_value<CTRL>(v);
    return o < v ? o : v;
}
template <typename T>
__device__ __forceinline__ T wave_min_to_lane63(T v) {
    return dpp_min<0x143>(dpp_min<0x142>(dpp_min<0x118>(dpp_min<0x114>(dpp_min<0x112>(dpp_min<0x111>(v))))));
}

// The total order of the rankings: key descending, bin ascending; bin -1 is "no entry".
__device__ __forceinline__ bool cand_before(double ka, long long ia, double kb, long long ib) {
    return ib < 0 || (ia >= 0 && (ka > kb || (ka == kb && ia < ib)));
}
// (key, bin) comes strictly after the previous winner (pk, pidx)
__device__ __forceinline__ bool after(double key, long long bin, double pk, long long pidx) {
    return key < pk || (key == pk && bin > pidx);
}
// (where neither side has an entry the copy of an unused value is harmless: the value of bin -1 is never output)
__device__ __forceinline__ void fold_best(double ov, long long oi, double &best, long long &best_i) {
    if (cand_before(ov, oi, best, best_i)) {
        best = ov;
        best_i = oi;
    }
}
__device__ __forceinline__ void wave_fold_best(double &best, long long &best_i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fold_best(__shfl_down(best, o, 64), __shfl_down(best_i, o, 64), best, best_i);
}

// `segs` workgroups per row, each the maxima whose rising edge lies in its share of the bins (a flat top is read on
// across the share's end, so every maximum belongs to exactly one share); segs > 1 leaves (value, bin) per share in
// part_v / part_i for highest_peak_merge_kernel.  (A single workgroup reads a row at 5 GB/s: 16 ms for the 1e7 bins of
// one C4 spectrum.)
__global__ __launch_bounds__(kBlock) void highest_peak_kernel(const double *power, int64_t nf, int segs,
                                                              int64_t *idx_out, double *val_out,
                                                              double *part_v, long long *part_i) {
    __shared__ double red_v[kBlock / 64];
    __shared__ long long red_i[kBlock / 64];
    const int64_t row = blockIdx.x / (unsigned)segs, seg = blockIdx.x % (unsigned)segs;
    const double *x = power + row * nf;
    const int64_t share = (nf + segs - 1) / segs;
    const int64_t lo = seg * share > 1 ? seg * share : 1, hi = (seg + 1) * share < nf - 1 ? (seg + 1) * share : nf - 1;
    double best = 0.0;
    long long best_i = -1;
    // scipy's rule is typed out here and in the sweep: through one shared flat-top function this loop keeps fewer loads
    // in flight (20 registers instead of 24) and the kernel takes 0.47 instead of 0.43 ms on the C3 batch
    for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {  // ascending per thread
        const double v = x[i];
        if (!(x[i - 1] < v)) continue;
        int64_t ahead = i + 1;
        while (ahead < nf - 1 && x[ahead] == v) ++ahead;
        if (!(x[ahead] < v)) continue;
        const long long mid = (long long)((i + ahead - 1) / 2);
        if (best_i < 0 || v > best) {
            best = v;
            best_i = mid;
        }
    }
    wave_fold_best(best, best_i);
    if ((threadIdx.x & 63) == 0) {
        red_v[threadIdx.x >> 6] = best;
        red_i[threadIdx.x >> 6] = best_i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) fold_best(red_v[w], red_i[w], best, best_i);
        if (segs > 1) {
            part_v[blockIdx.x] = best;
            part_i[blockIdx.x] = best_i;
        } else {
            if (idx_out) idx_out[row] = best_i;
            if (val_out) val_out[row] = best_i >= 0 ? best : __builtin_nan("");
        }
    }
}

// one wave per row: the shares' winners, the higher value first, the lower bin on equal values
__global__ __launch_bounds__(64) void highest_peak_merge_kernel(const double *part_v, const long long *part_i, int segs,
                                                                int64_t *idx_out, double *val_out) {
    const int64_t row = blockIdx.x;
    double best = 0.0;
    long long best_i = -1;
    for (int s = threadIdx.x; s < segs; s += 64) fold_best(part_v[row * segs + s], part_i[row * segs + s], best, best_i);
    wave_fold_best(best, best_i);
    if (threadIdx.x == 0) {
        if (idx_out) idx_out[row] = best_i;
        if (val_out) val_out[row] = best_i >= 0 ? best : __builtin_nan("");
    }
}

// ---- top-k peaks with prominences and half-maximum crossings ------------------------------------------
constexpr int kPkBlock = 256;
constexpr int kPkWaves = 5;          // workgroups per CU asked of the SORT instance (96 registers); the other one more (80)
constexpr int kPkMaxBlocks = 4096;   // LDS: two doubles per block
constexpr int kPkMaxK = 128;         // ranked peaks per launch
constexpr int kPkMaxKTotal = 1024;   // ... per call
constexpr int kPkSortFrom = 16;      // rankings of more entries sort the list (the SORT instance: four more registers)
constexpr int kPkPre = 132;          // by prominence: the first walks go to the k + 4 highest maxima, in a later launch to
                                     // 2 k + 4 seeds (a tighter threshold for the second sweep)
constexpr int kPkWalkLoads = 8;      // loads a lane of a walk has in flight: 4 / 8 / 16 = 70 / 77 / 95 registers
constexpr int kPkAhead = 2;          // chunks in flight ahead of the one examined (first sweep): fits the 80 registers
constexpr int kPkChunk = 1024;       // bins per sweep step
constexpr int kPkPer = kPkChunk / kPkBlock;   // consecutive bins per lane
constexpr int kPkFusedShift = 8;     // 256-bin blocks = one wave's stretch of a chunk: extrema come with the sweep
static_assert(kPkPer * 64 == 1 << kPkFusedShift, "a wave's stretch is one block");
constexpr int kPkCap = 1024;         // candidate slots in LDS (20 B each): a chunk adds at most kPkChunk / 2
static_assert(kPkMaxK + 4 <= kPkPre && kPkPre <= kPkCap / 4, "win_* and the candidate list hold the first walks");

struct PeakArgs {
    const double *power;
    int64_t nf;
    int k, by_prominence, blk_shift;
    int k_total, k_off;   // the outputs are [rows][k_total]; this launch fills columns k_off .. k_off + k - 1 and ranks
                          // only what comes after column k_off - 1 in the total order
    int64_t nblk;
    long long *count, *idx, *half_lo, *half_hi;
    double *height, *prom;
};

// The dynamic LDS block of a row (launch_topk sizes it from the same type).
struct TopkLds {
    double *bmin, *bmax;   // [nblk] block extrema
    double *ch, *cp;       // [kPkCap] candidates: height, prominence (NaN: not walked yet),
    int *ci;               //          bin (rows have < 2^31 bins: launch_topk)
    __device__ __forceinline__ TopkLds(unsigned char *raw, int64_t nblk) {
        bmin = reinterpret_cast<double *>(raw);
        bmax = bmin + nblk;
        ch = bmax + nblk;
        cp = ch + kPkCap;
        ci = reinterpret_cast<int *>(cp + kPkCap);
    }
    static size_t bytes(int64_t nblk) { return (size_t)(nblk > 0 ? nblk : 1) * 16 + (size_t)kPkCap * (8 + 8 + 4) + 16; }
};

// The fixed LDS arrays, one instance per kernel.
template <bool SORT>
struct TopkFixed {
    static constexpr int kWin = SORT ? kPkPre : kPkSortFrom + 4;   // winners a ranking of this instance can be asked for
    static constexpr int kTop = kPkSortFrom + 4;                   // few-ranks rankings: every wave's winners
    static_assert(kWin >= kTop && kPkSortFrom <= 16, "rank_by_rounds fills win_*[0 .. m), m <= kPkSortFrom");
    double win_key[kWin], win_h[kWin], win_p[kWin];
    long long win_idx[kWin];
    double low[2][8][2];                // the walks of a pass: lowest sample met leftwards / rightwards
    double red_k[kPkBlock / 64];
    long long count[kPkBlock / 64];
    double thr;                         // threshold of the sweep under way
    int wtop[kPkBlock / 64 * kTop];     // slots of the candidate list
    unsigned need[32];                  // second sweep: chunks that can hold a candidate at the initial tau
    int red_e[kPkBlock / 64];
    int ncand, first;
};

// What a phase needs to know of its row and of its thread.
struct Row {
    const double *x;
    int64_t nf, nblk;
    int sh;   // bins per block = 1 << sh
    int tid, lane, wave;
};

// The start of a ranking: everything (any = false), or what comes strictly after (key, bin).
struct After {
    bool any;
    double key;
    long long bin;
};

// Minimum and maximum of a block over the wave, valid in lane 63.  A block holding a NaN has bmax = +inf: it never
// lets a walk hop over it (a NaN stops a walk, as x[i] <= x[peak] is false).
__device__ __forceinline__ void wave_extrema(double &mn, double &mx, bool isnan) {
    mn = wave_min_to_lane63(mn);
    mx = -wave_min_to_lane63(-mx);
    if (__any(isnan)) mx = __builtin_inf();
}

// minimum of every thread's v over the workgroup (two barriers)
__device__ __forceinline__ double block_min(double v, double *red, int lane, int wave) {
    for (int o = 32; o > 0; o >>= 1) {
        const double om = __shfl_xor(v, o, 64);
        v = om < v ? om : v;
    }
    if (lane == 0) red[wave] = v;
    __syncthreads();
    for (int w = 0; w < kPkBlock / 64; ++w) v = red[w] < v ? red[w] : v;
    __syncthreads();
    return v;
}

// highest block maximum over the bins [c0, c1)
__device__ __forceinline__ double chunk_max(const double *bmax, int64_t c0, int64_t c1, int sh) {
    double tmx = -__builtin_inf();
    for (int64_t b = c0 >> sh; b < ((c1 + ((int64_t)1 << sh) - 1) >> sh); ++b) tmx = bmax[b] > tmx ? bmax[b] : tmx;
    return tmx;
}

// ---- half-maximum crossings of the ranked peaks (periods_at_half_max) -----------------------------------------------
// GROUP lanes per ranked peak, 64 / GROUP peaks per wave side by side, no workgroup barriers: 4 GROUP bins per step
// outwards from the peak, four loads per lane in flight, the nearest sign change by ballot.  The crossings of a
// periodogram's peaks lie a few bins from the maximum, so many peaks take a quarter wave each: a wave per peak spent
// 136 us of a row's 835 in a 128-rank launch.
template <int GROUP>
__device__ __forceinline__ void half_max(const double *x, int64_t nf, int lane, int wave, const long long *win_idx,
                                         const double *win_key, const PeakArgs &a, int nwin, int64_t ob) {
    const int sub = lane & (GROUP - 1), grp = lane / GROUP;
    auto group_bits = [&](bool f) -> unsigned long long {
        const unsigned long long all = __ballot(f);
        return GROUP == 64 ? all : (all >> (GROUP * grp)) & ((1ull << (GROUP & 63)) - 1ull);
    };
    for (int r0 = wave * (64 / GROUP); r0 < a.k; r0 += (kPkBlock / 64) * (64 / GROUP)) {
        const int rk = r0 + grp;
        const long long idmax = (rk < a.k && rk < nwin) ? win_idx[rk] : -1;
        long long lo_abs = -1, hi_abs = -1;
        const double half = idmax >= 0 ? x[idmax] - win_key[rk] / 2 : 0.0;     // core.py:972 (height or prominence)
        auto flips = [&](int64_t i) {                       // signbit(x[i]-half) != signbit(x[i+1]-half)
            return (__double_as_longlong(x[i] - half) < 0) != (__double_as_longlong(x[i + 1] - half) < 0);
        };
        // last sign change inside x[:idmax]: pairs (i, i+1), i+1 <= idmax-1; nearest to the peak first
        for (int64_t top = idmax - 2;; top -= 4 * GROUP) {
            const bool go = idmax >= 0 && hi_abs < 0 && top >= 0;
            if (!__any(go)) break;                          // (wave-uniform)
            bool f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = top - (GROUP * u + sub);
                f[u] = go && i >= 0 && flips(i);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned long long bits = group_bits(f[u]);
                if (bits && hi_abs < 0) hi_abs = top - (GROUP * u + __builtin_ctzll(bits));
            }
        }
        // first sign change from the peak rightwards: pairs (idmax+i, idmax+i+1)
        for (int64_t base = idmax;; base += 4 * GROUP) {
            const bool go = idmax >= 0 && lo_abs < 0 && base < nf - 1;
            if (!__any(go)) break;                          // (wave-uniform)
            bool f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = base + GROUP * u + sub;
                f[u] = go && i < nf - 1 && flips(i);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned long long bits = group_bits(f[u]);
                if (bits && lo_abs < 0) lo_abs = base + GROUP * u + __builtin_ctzll(bits);
            }
        }
        if (sub == 0 && rk < a.k) {
            if (a.half_lo) a.half_lo[ob + rk] = lo_abs;
            if (a.half_hi) a.half_hi[ob + rk] = hi_abs;
        }
    }
}

// A lane's best entry strictly after the previous winner (pk, pidx) among the slots q = q0, q0 + stride, .. < nq of
// the candidate list (VIA = false) or of the slots that via[] names (-1: none).
template <bool VIA>
__device__ __forceinline__ void best_after(const double *ch, const double *cp, const int *ci, const int *via, int q0, int stride, int nq, bool by_prom,
                                           bool any_prev, double pk, long long pidx, double &lk, int &li, int &le) {
    lk = 0.0;
    li = -1;
    le = -1;
    for (int q = q0; q < nq; q += stride) {
        const int e = VIA ? via[q] : q;
        if (VIA && e < 0) continue;
        const double key = by_prom ? cp[e] : ch[e];
        const int bin = ci[e];
        if ((!any_prev || after(key, bin, pk, pidx)) && cand_before(key, bin, lk, li)) {
            lk = key;
            li = bin;
            le = e;
        }
    }
}

// ---- walks: sixteen lanes together, arguments uniform over the group --------------------------------------------
__device__ __forceinline__ double group_min(double m) {
    for (int o = 8; o > 0; o >>= 1) {
        const double om = __shfl_xor(m, o, 64);
        m = om < m ? om : m;
    }
    return m;
}
__device__ __forceinline__ unsigned group_ballot(bool p, int lane) {
    return (unsigned)((__ballot(p) >> (lane & 48)) & 0xffffull);
}

// `count` bins from `start` on in direction DIR, 16 x kPkWalkLoads per step; true when the walk ended among them.
// (32-bit bin numbers inside a walk: the row pointer stays a scalar base and a load takes one address register)
template <int DIR>
__device__ __forceinline__ bool run(const double *x, double h, int start, int count, int lane, double &low) {
    const int gl = lane & 15;
    for (int o = 0; o < count; o += 16 * kPkWalkLoads) {
        double v[kPkWalkLoads];
#pragma unroll
        for (int u = 0; u < kPkWalkLoads; ++u) {
            const int k = o + 16 * u + gl;
            v[u] = k < count ? x[(unsigned)(start + DIR * k)] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kPkWalkLoads; ++u) {
            const bool valid = o + 16 * u + gl < count;
            const unsigned sb = group_ballot(valid && !(v[u] <= h), lane);
            const int first = sb ? __builtin_ctz(sb) : 16;
            const double m = group_min(valid && gl < first ? v[u] : __builtin_inf());
            low = m < low ? m : low;
            if (sb) return true;
        }
    }
    return false;
}

// Lowest sample met walking from bin `from` in direction DIR (+1 / -1) while x[i] <= h (scipy's loop): the rest of
// the first block, then 16 blocks per step over the block extrema in LDS - whole blocks that cannot stop the walk are
// hopped over -, then the block that does stop it.  A step costs one memory latency instead of one per bin: the
// highest peak of a 5e4-bin row (900 single steps) takes ~12.
template <int DIR>
__device__ __forceinline__ double walk(const TopkLds &l, const Row &r, int from, double h) {
    double low = h;
    const int nfi = (int)r.nf, nblki = (int)r.nblk, sh = r.sh, gl = r.lane & 15;
    const int b0 = from >> sh;
    const int b0_end = ((b0 + 1) << sh) < nfi ? ((b0 + 1) << sh) : nfi;
    if (run<DIR>(r.x, h, from, DIR > 0 ? b0_end - from : from - (b0 << sh) + 1, r.lane, low)) return low;
    int b = b0 + DIR;
    for (;;) {
        const int bb = b + DIR * gl;
        const bool pass = bb >= 0 && bb < nblki && l.bmax[bb] <= h;
        const unsigned fb = group_ballot(!pass, r.lane);
        const int first = fb ? __builtin_ctz(fb) : 16;
        const double m = group_min(gl < first ? l.bmin[bb] : __builtin_inf());   // (the lanes below `first` pass: in range)
        low = m < low ? m : low;
        if (fb) {
            b += DIR * first;
            break;
        }
        b += 16 * DIR;
    }
    if (b < 0 || b >= nblki) return low;   // reached the border of the signal
    const int b_end = ((b + 1) << sh) < nfi ? ((b + 1) << sh) : nfi;
    run<DIR>(r.x, h, DIR > 0 ? b << sh : b_end - 1, b_end - (b << sh), r.lane, low);   // this block holds a sample > h (or a NaN)
    return low;
}

// Prominences of the candidates that have none yet (a ranking leaves its winners - walked - in front, a sweep appends).
template <bool SORT>
__device__ __forceinline__ void walk_candidates(const TopkLds &l, TopkFixed<SORT> &s, const Row &r) {
    const int n = s.ncand, tid = r.tid, gl = r.lane & 15;
    if (tid == 0) s.first = n;
    __syncthreads();
    for (int e = tid; e < n; e += kPkBlock)
        if (!(l.cp[e] == l.cp[e])) atomicMin(&s.first, e);
    __syncthreads();
    const int t0 = s.first;
    if (n - t0 > 16) {
        // many (a later launch, a second sweep that found a lot): one group per candidate, left then right, no barrier
        // between candidates (the walks are bound by how many are in flight, not by a candidate's own chain of latencies)
        for (int e = t0 + (tid >> 4); e < n; e += kPkBlock / 16) {
            if (l.cp[e] == l.cp[e]) continue;
            const double v = l.ch[e];
            const int at = l.ci[e];
            const double lo = walk<-1>(l, r, at, v), hi = walk<+1>(l, r, at, v);
            if (gl == 0) l.cp[e] = v - (lo > hi ? lo : hi);
        }
        __syncthreads();
        return;
    }
    // few: eight candidates a pass, the groups of waves 0 and 1 walk left, those of waves 2 and 3 right (the walks are
    // chains of dependent loads).  The direction is the wave's, so both walks keep a compile-time stride: a stride per
    // group cost 14 registers = the sixth workgroup per CU.
    const int slot = (tid >> 4) & 7;
    const bool right = __builtin_amdgcn_readfirstlane(r.wave) >= 2;
    int par = 0;
    for (int base = t0; base < n; base += 8, par ^= 1) {
        const int e = base + slot;
        if (e < n && !(l.cp[e] == l.cp[e])) {
            const double v = l.ch[e];
            const int at = l.ci[e];
            const double low = right ? walk<+1>(l, r, at, v) : walk<-1>(l, r, at, v);
            if (gl == 0) s.low[par][slot][right ? 1 : 0] = low;
        }
        __syncthreads();
        if (tid < 8 && base + tid < n && !(l.cp[base + tid] == l.cp[base + tid])) {
            const double lo = s.low[par][tid][0], hi = s.low[par][tid][1];
            l.cp[base + tid] = l.ch[base + tid] - (lo > hi ? lo : hi);
        }
        // (the next pass writes the other half of low[] and other candidates; its barrier orders these reads before the
        // pass after it)
    }
    __syncthreads();
}

// PDC_PK_DBG (developer builds, tools/peaks_stamps.py): s_memrealtime stamps (10 ns ticks) of every row's phases
#ifdef PDC_PK_DBG
__device__ unsigned long long pk_dbg[8192 * 16];
#define PK_STAMP(i)                                                                                   \
    if (tid == 0 && blockIdx.x < 8192) pk_dbg[blockIdx.x * 16 + (i)] = __builtin_amdgcn_s_memrealtime();
#else
#define PK_STAMP(i)
#endif

// SORT: the instance for launches of more than kPkSortFrom ranks and for the later launches of a call (its rankings
// sort the candidate list; four more registers, five workgroups per CU instead of six - which cost the few-ranks
// launches 10 %, so they keep their own).
// The kernel is its LDS views, the separate block-extrema pass, the rankings, the sweep, the prologue of a later launch,
// the sequence of phase calls with their stamps, and the output stores.  Three phases are text here (lambdas) under the
// standing rule of gls_sums.h.  The few-ranks instance sits at its 80 registers: as __forceinline__ functions with the
// same bodies the block-extrema pass and the sweep cost it 2 spilled registers each, reloaded inside the first sweep's
// loop.  The rankings as functions cost the SORT instance 0.5 - 1 % on the launches of 128 ranks.
template <bool SORT>
__global__ __launch_bounds__(kPkBlock, SORT ? kPkWaves : kPkWaves + 1) void peaks_topk_kernel(PeakArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const TopkLds l(lds_raw, a.nblk);
    double *const bmin = l.bmin, *const bmax = l.bmax, *const ch = l.ch, *const cp = l.cp;
    int *const ci = l.ci;
    __shared__ TopkFixed<SORT> s;
    constexpr int kTop = TopkFixed<SORT>::kTop;   // (rank_candidates)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *x = a.power + (int64_t)blockIdx.x * a.nf;
    const int64_t nf = a.nf;
    const int sh = a.blk_shift;
    const Row r = {x, nf, a.nblk, sh, tid, lane, wave};
    const int64_t blk = (int64_t)1 << sh;
    const double inf = __builtin_inf();

    // Per-block minimum / maximum, a wave per block, coalesced: rows of more than 1M bins, whose blocks are larger than
    // a wave's stretch of a chunk (with 256-bin blocks the first sweep does this on its way).  Same NaN rule as
    // wave_extrema: a block holding a NaN has bmax = +inf.
    for (int64_t b = wave; b < a.nblk && sh != kPkFusedShift; b += kPkBlock / 64) {
        double mn = inf, mx = -inf;
        bool nan = false;
        const int64_t e = (b + 1) * blk < nf ? (b + 1) * blk : nf;
        for (int64_t i = b * blk + lane; i < e; i += 64) {
            const double v = x[i];
            nan = nan || v != v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double omn = __shfl_xor(mn, o, 64), omx = __shfl_xor(mx, o, 64);
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
        }
        if (__any(nan)) mx = inf;
        if (lane == 0) {
            bmin[b] = mn;
            bmax[b] = mx;
        }
    }
    if (tid == 0) {
        s.ncand = 0;
        s.thr = -inf;
    }
    __syncthreads();
    const bool excl = SORT && a.k_off > 0;   // (later launches of a call always run the SORT instance: launch_topk)
    double prev_key = inf;
    long long prev_idx = -1;
    double h_cut = inf;   // (later launches by prominence) lowest height among the winners already output
    // The m best candidates (by height or by prominence; ties: lower bin first; the same bin only once)
    // into win_*[0 .. m), by m rounds of "best entry strictly after the previous winner"; the list is then
    // cut down to those.  Returns how many there are.
    auto rank_candidates = [&](int m, bool by_prom) __attribute__((always_inline)) -> int {
        const int n = s.ncand;
        double pk = inf;          // previous winner (key, bin): everything is "after" (+inf, -1)
        long long pidx = -1;
        // a later launch of a call: rankings by the call's own key start after the last winner of the launch before
        bool ex = excl && by_prom == (a.by_prominence != 0);
        if (ex) {
            pk = prev_key;
            pidx = prev_idx;
        } else if (excl && a.by_prominence) {
            // ... and the SEEDS of a later launch by prominence - the rankings by height that pick the maxima walked
            // first, whose K-th prominence becomes the threshold tau of the second sweep - are the highest maxima
            // BELOW the lowest height any earlier launch has output: none of them is an earlier winner, so all of them
            // count towards tau (the highest maxima of the row are mostly winners already output: tau would stay -inf
            // and the second sweep would collect and walk EVERY maximum).  Any set of seeds gives a valid tau.
            ex = true;
            pk = h_cut;
            pidx = 0x7fffffff;   // (strictly below h_cut)
        }
        int found = 0;
        if (SORT && m > kPkSortFrom) {
            // Many ranks: the rounds below would cost 0.3 ms per ranking of 68.  Instead the whole list is sorted in LDS (bitonic, by key descending then bin ascending; unused
            // slots last), duplicates of a bin and entries not after the previous launch's last winner are dropped,
            // and the first m that remain are the winners: ~55 compare-exchange steps for a full list.
            int P = 2;
            while (P < n) P <<= 1;
            for (int e = n + tid; e < P; e += kPkBlock) {
                ci[e] = -1;
                ch[e] = -inf;
                cp[e] = -inf;
            }
            __syncthreads();
            for (int kk = 2; kk <= P; kk <<= 1) {
                for (int j = kk >> 1; j > 0; j >>= 1) {
                    for (int c = tid; c < (P >> 1); c += kPkBlock) {
                        const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1)), l = i | j;
                        const double ka = by_prom ? cp[i] : ch[i], kb = by_prom ? cp[l] : ch[l];
                        const int ia = ci[i], ib = ci[l];
                        // (a NaN key - none is expected here - sorts with the unused slots' -inf)
                        const bool b_first = cand_before(kb == kb ? kb : -inf, ib, ka == ka ? ka : -inf, ia);
                        const bool up = (i & kk) == 0;
                        if (b_first == up && !(ia == ib && ka == kb)) {
                            const double ha = ch[i], pa = cp[i];
                            ch[i] = ch[l];
                            cp[i] = cp[l];
                            ci[i] = ib;
                            ch[l] = ha;
                            cp[l] = pa;
                            ci[l] = ia;
                        }
                    }
                    __syncthreads();
                }
            }
            int taken = 0;                                       // winners so far (workgroup-uniform)
            for (int base = 0; base < n && taken < m; base += kPkBlock) {
                const int e = base + tid;
                bool ok = false;
                double key = 0.0;
                long long bin = -1;
                if (e < n) {
                    key = by_prom ? cp[e] : ch[e];
                    bin = ci[e];
                    ok = bin >= 0 && (e == 0 || ci[e - 1] != (int)bin) && (!ex || after(key, bin, pk, pidx));
                }
                const unsigned long long mask = __ballot(ok);
                if (lane == 0) s.red_e[wave] = __builtin_popcountll(mask);
                __syncthreads();
                int rank = taken + __builtin_popcountll(mask & ((1ull << lane) - 1ull)), total = 0;
                for (int w = 0; w < kPkBlock / 64; ++w) {
                    if (w < wave) rank += s.red_e[w];
                    total += s.red_e[w];
                }
                if (ok && rank < m) {
                    s.win_key[rank] = key;
                    s.win_idx[rank] = bin;
                    s.win_h[rank] = ch[e];
                    s.win_p[rank] = cp[e];
                }
                taken += total;
                __syncthreads();
            }
            found = taken < m ? taken : m;
        } else {
            // Few ranks: two phases without a barrier inside - (1) every wave ranks the m best of ITS share of
            // the list (entry e belongs to wave (e / 64) mod 4), m rounds of "best entry strictly after the wave's previous
            // winner", the winners' slots to s.wtop[wave][]; (2) after one barrier every wave ranks the <= 4 m slots of
            // s.wtop the same way - all four get the same answer, so none waits for another.  A round is a maximum of the
            // keys over the wave by DPP, the lowest bin among the lanes that hold it, and a ballot: no LDS crossbar, no
            // barrier (a block reduction per round, two barriers each, took 11.7 us for the 8 rounds of a k = 4 call by
            // prominence, three rankings per row).
            // best (key descending, bin ascending) over the wave of every lane's (key, bin >= 0 or -1: none, slot)
            auto wave_best = [&](double key, int bin, int slot, double &bk, int &bi, int &be) __attribute__((always_inline)) -> bool {
                const double kk = bin >= 0 ? key : -inf;
                const double top = -readlane_double(wave_min_to_lane63(-kk), 63);
                const bool tied = bin >= 0 && kk == top;
                const int lowest = __builtin_amdgcn_readlane(wave_min_to_lane63(tied ? bin : 0x7fffffff), 63);
                const unsigned long long who = __ballot(tied && bin == lowest);
                if (who == 0ull) return false;
                const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(who));
                // (the winner's own bits: a tie of -0.0 and +0.0 keys is a tie, but the half-maximum level downstream takes
                // the sign along - tools/fuzz_peaks.py case 23)
                bk = readlane_double(key, src);
                bi = lowest;
                be = __builtin_amdgcn_readlane(slot, src);
                return true;
            };
            {   // phase 1
                double wpk = pk;
                int wpi = (int)pidx;
                bool any_prev = ex;
                int r = 0;
                for (; r < m; ++r) {
                    double lk;
                    int li, le;
                    best_after<false>(ch, cp, ci, nullptr, tid, kPkBlock, n, by_prom, any_prev, wpk, wpi, lk, li, le);
                    double bk;
                    int bi, be;
                    if (!wave_best(lk, li, le, bk, bi, be)) break;    // (wave-uniform)
                    if (lane == 0) s.wtop[wave * kTop + r] = be;
                    wpk = bk;
                    wpi = bi;
                    any_prev = true;
                }
                for (int q = r + lane; q < kTop; q += 64) s.wtop[wave * kTop + q] = -1;
            }
            __syncthreads();
            bool any_prev = ex;
            for (int round = 0; round < m; ++round) {
                double lk;
                int li, le;
                best_after<true>(ch, cp, ci, s.wtop, lane, 64, (kPkBlock / 64) * kTop, by_prom, any_prev, pk, pidx, lk, li, le);
                double bk;
                int bi, be;
                if (!wave_best(lk, li, le, bk, bi, be)) break;        // (the same in every wave)
                if (tid == 0) {
                    s.win_key[round] = bk;
                    s.win_idx[round] = bi;
                    s.win_h[round] = ch[be];
                    s.win_p[round] = cp[be];
                }
                pk = bk;
                pidx = bi;
                any_prev = true;
                ++found;
            }
        }
        __syncthreads();
        for (int e = tid; e < found; e += kPkBlock) {
            ci[e] = (int)s.win_idx[e];
            ch[e] = s.win_h[e];
            cp[e] = s.win_p[e];
        }
        if (tid == 0) s.ncand = found;
        __syncthreads();
        return found;
    };
    // One sweep over the row in chunks of 1024 bins straight from global memory.  FIRST: every maximum is counted (in
    // `mine`); those with height >= s.thr are collected, and whenever the list is half full it is cut down to the m
    // highest (s.thr = the m-th); kPkAhead chunks are in flight ahead of the one examined, and with 256-bin blocks the
    // block extrema are taken on the way.  Otherwise (by prominence, second sweep): the maxima with
    // height - row_min >= s.thr are collected (s.thr = tau), walked and ranked when the list fills up (tau rises to
    // the m-th prominence); chunks whose block maxima rule out a candidate are not read.
    long long mine = 0;
    double row_min = inf;
    auto sweep = [&](auto first_tag, int m) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const double sub = FIRST ? 0.0 : row_min;
        const double nan = __builtin_nan("");
        // A wave reads a stretch of 256 consecutive bins + the bin before and after; all loads of a chunk are in
        // flight together.  Lane L owns the kPer CONSECUTIVE bins w0 + kPer L .. + kPer - 1 (two 16-byte loads on the
        // fast path): three of four neighbours are the lane's own registers, the other two one DPP wave shift away.
        constexpr int kPer = kPkPer;
        static_assert(kPer == 4, "the fast path loads two pairs of doubles");
        typedef double pair_t __attribute__((ext_vector_type(2), aligned(8)));
        auto load = [&](int64_t c0, double (&v)[kPer], double &halo_lo, double &halo_hi) __attribute__((always_inline)) {
            const int64_t w0 = c0 + (int64_t)wave * (64 * kPer);
            const int64_t i0 = w0 + (int64_t)lane * kPer;
            if (w0 + 64 * kPer <= nf) {   // (wave-uniform) the whole stretch lies inside the row
                const pair_t a01 = *reinterpret_cast<const pair_t *>(x + i0);
                const pair_t a23 = *reinterpret_cast<const pair_t *>(x + i0 + 2);
                v[0] = a01.x;
                v[1] = a01.y;
                v[2] = a23.x;
                v[3] = a23.y;
            } else {
#pragma unroll
                for (int j = 0; j < kPer; ++j) v[j] = i0 + j < nf ? x[i0 + j] : nan;
            }
            halo_lo = (w0 >= 1 && w0 <= nf) ? x[w0 - 1] : nan;
            halo_hi = w0 + 64 * kPer < nf ? x[w0 + 64 * kPer] : nan;
        };
        static_assert(kPkAhead == 2, "the chunk examined and two in flight: v, vn, vnn");
        double v[kPer], halo_lo, halo_hi, vn[kPer], next_lo = nan, next_hi = nan;
        double vnn[kPer], nn_lo = nan, nn_hi = nan;
        if (FIRST) load(0, v, halo_lo, halo_hi);
        if (FIRST) load(kPkChunk, vn, next_lo, next_hi);
        // Second sweep: tau only rises, so a chunk whose block maxima rule a candidate out at the INITIAL tau
        // never needs a look - found for all chunks at once, and those chunks cost neither a barrier nor an
        // LDS scan below (of 49 chunks of a C3 row a handful remain)
        const int64_t nchunks = (nf + kPkChunk - 1) / kPkChunk;
        const bool masked = !FIRST && nchunks <= 32 * 32;
        if (masked) {
            if (tid < 32) s.need[tid] = 0u;
            __syncthreads();
            const double thr0 = s.thr;
            for (int64_t c = tid; c < nchunks; c += kPkBlock) {
                const int64_t e0 = c * kPkChunk, e1 = e0 + kPkChunk < nf ? e0 + kPkChunk : nf;
                if (chunk_max(bmax, e0, e1, sh) - sub >= thr0) atomicOr(&s.need[c >> 5], 1u << (c & 31));
            }
            __syncthreads();
        }
        for (int64_t c0 = 0; c0 < nf; c0 += kPkChunk) {
            const int64_t c1 = c0 + kPkChunk < nf ? c0 + kPkChunk : nf;
            if (masked && !((s.need[(c0 / kPkChunk) >> 5] >> ((c0 / kPkChunk) & 31)) & 1u)) continue;   // (workgroup-uniform)
            if (FIRST) load(c0 + kPkAhead * kPkChunk, vnn, nn_lo, nn_hi);
            __syncthreads();   // everyone is done with the previous chunk (and sees s.thr / s.ncand)
            if (s.ncand > kPkCap / 2) {   // (workgroup-uniform) a chunk adds at most kPkChunk / 2 maxima
                if (!FIRST) walk_candidates(l, s, r);
                const int got = rank_candidates(m, !FIRST);
                if (tid == 0 && got == m) s.thr = s.win_key[m - 1];
                __syncthreads();
            }
            const double thr = s.thr;
            if (!FIRST) {   // (workgroup-uniform) no block of this chunk reaches the threshold
                if (!(chunk_max(bmax, c0, c1, sh) - sub >= thr)) continue;
            }
            if (!FIRST) load(c0, v, halo_lo, halo_hi);
            const int64_t w0 = c0 + (int64_t)wave * (64 * kPer);
            if (FIRST && sh == kPkFusedShift && w0 < nf) {   // (wave-uniform) this wave's stretch is one block
                double mn = inf, mx = -inf;
                bool isnan = false;
#pragma unroll
                for (int j = 0; j < kPer; ++j) {
                    const double q = v[j];
                    isnan = isnan || (w0 + lane * kPer + j < nf && q != q);
                    mn = q < mn ? q : mn;
                    mx = q > mx ? q : mx;
                }
                wave_extrema(mn, mx, isnan);
                if (lane == 63) {
                    bmin[w0 >> kPkFusedShift] = mn;
                    bmax[w0 >> kPkFusedShift] = mx;
                }
            }
            // x of the lane below / above (lane 0 / 63: the halo): wave_shr:1 / wave_shl:1
            const double below = dpp_double<0x138>(halo_lo, v[kPer - 1]), above = dpp_double<0x130>(halo_hi, v[0]);
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int64_t i = w0 + (int64_t)lane * kPer + j;
                const double prev = j == 0 ? below : v[j > 0 ? j - 1 : 0];
                const double next = j == kPer - 1 ? above : v[j < kPer - 1 ? j + 1 : j];
                // a maximum: strict rise, flat tops -> midpoint, edges and NaN never peaks (scipy's rule, typed out as in
                // highest_peak_kernel: see there)
                const double vv = v[j];
                if (!(i >= 1 && i < nf - 1 && prev < vv)) continue;
                if (!FIRST && !(vv - sub >= thr)) continue;
                int64_t ahead = i + 1;
                if (!(next < vv)) {
                    if (!(next == vv)) continue;
                    while (ahead < nf - 1 && x[ahead] == vv) ++ahead;   // a flat top: global reads from here on
                    if (!(x[ahead] < vv)) continue;
                }
                if (FIRST) ++mine;
                if (FIRST && !(vv >= thr)) continue;
                const int slot = atomicAdd(&s.ncand, 1);
                const int64_t mid = (i + ahead - 1) / 2;
                ci[slot] = (int)mid;
                ch[slot] = mid == i ? vv : x[mid];   // (a flat top of zeros may mix +0.0 and -0.0: the reported
                                                     // height is the midpoint's own bits, as scipy's x[peaks])
                cp[slot] = nan;
            }
            if (FIRST) {
#pragma unroll
                for (int j = 0; j < kPer; ++j) v[j] = vn[j];
                halo_lo = next_lo;
                halo_hi = next_hi;
#pragma unroll
                for (int j = 0; j < kPer; ++j) vn[j] = vnn[j];
                next_lo = nn_lo;
                next_hi = nn_hi;
            }
        }
        __syncthreads();
    };

    const int K = a.k < kPkMaxK ? a.k : kPkMaxK;
    // by prominence: the first walks go to the `pre` highest maxima - in a later launch (seeds below h_cut, see
    // rank_candidates) to twice as many: tau is then the K-th of 2 K + 4 prominences instead of the K-th of K + 4
    const int pre = SORT && a.k_off > 0 && 2 * K + 4 <= kPkPre ? 2 * K + 4 : K + 4;
    const int64_t ob = (int64_t)blockIdx.x * a.k_total + a.k_off;
    if (excl) {
        prev_key = (a.by_prominence ? a.prom : a.height)[ob - 1];
        prev_idx = a.idx[ob - 1];
        if (a.by_prominence) {   // lowest height among the winners of the launches before (their bins are in idx[])
            double lowest = inf;
            for (int j = tid; j < a.k_off; j += kPkBlock) {
                const long long b = a.idx[ob - a.k_off + j];
                if (b >= 0) {
                    const double hb = x[b];
                    lowest = hb < lowest ? hb : lowest;
                }
            }
            h_cut = block_min(lowest, s.red_k, lane, wave);
        }
        if (prev_idx < 0) {   // (workgroup-uniform) the launch before already ran out of peaks
            if (tid < a.k) {
                if (a.idx) a.idx[ob + tid] = -1;
                if (a.height) a.height[ob + tid] = __builtin_nan("");
                if (a.prom) a.prom[ob + tid] = __builtin_nan("");
                if (a.half_lo) a.half_lo[ob + tid] = -1;
                if (a.half_hi) a.half_hi[ob + tid] = -1;
            }
            return;
        }
    }
    static_assert(kPkMaxK + 4 <= kPkPre && kPkPre <= kPkCap / 4, "win_* and the candidate list hold the first walks");
    PK_STAMP(0)
    sweep(std::true_type{}, a.by_prominence ? pre : K);
    PK_STAMP(1)
    // lowest sample of the row (NaN aside): prominence <= height - row_min
    for (int64_t b = tid; b < a.nblk; b += kPkBlock) row_min = bmin[b] < row_min ? bmin[b] : row_min;
    row_min = block_min(row_min, s.red_k, lane, wave);

    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if (lane == 0) s.count[wave] = mine;
    int nwin;
    if (!a.by_prominence) {
        nwin = rank_candidates(K, false);
        PK_STAMP(2)
        walk_candidates(l, s, r);                       // the winners' prominences
        PK_STAMP(3)
        if (tid < nwin) s.win_p[tid] = cp[tid];
    } else {
        rank_candidates(pre, false);
        PK_STAMP(2)
        walk_candidates(l, s, r);                       // the highest maxima
        PK_STAMP(3)
        nwin = rank_candidates(K, true);
        PK_STAMP(4)
        if (tid == 0) s.thr = nwin == K ? s.win_key[K - 1] : -inf;   // tau
        sweep(std::false_type{}, K);
        PK_STAMP(5)
        walk_candidates(l, s, r);
        PK_STAMP(6)
        nwin = rank_candidates(K, true);
        PK_STAMP(7)
    }
    __syncthreads();
    if (tid == 0) {
        long long total = 0;
        for (int w = 0; w < kPkBlock / 64; ++w) total += s.count[w];
        if (a.count) a.count[blockIdx.x] = total;
    }
    if (tid < a.k) {
        const bool ok = tid < nwin;
        if (a.idx) a.idx[ob + tid] = ok ? s.win_idx[tid] : -1;
        if (a.height) a.height[ob + tid] = ok ? s.win_h[tid] : __builtin_nan("");
        if (a.prom) a.prom[ob + tid] = ok ? s.win_p[tid] : __builtin_nan("");
    }

    // ---- D: half-maximum crossings of every ranked peak (periods_at_half_max) -------------------
    // One wave per ranked peak (the k searches run side by side, no workgroup barriers): 256 bins per step
    // outwards from the peak, four loads per lane in flight, the nearest sign change by ballot.
    PK_STAMP(8)
    if (!a.half_lo && !a.half_hi) return;
    if (SORT && a.k > 16) half_max<16>(x, nf, lane, wave, s.win_idx, s.win_key, a, nwin, ob);
    else half_max<64>(x, nf, lane, wave, s.win_idx, s.win_key, a, nwin, ob);
    PK_STAMP(9)
}

}  // namespace

#ifdef PDC_PK_DBG
extern "C" int pdc_debug_peaks_stamps(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(pk_dbg), sizeof(pk_dbg)) == hipSuccess ? 0 : 1;
}
#endif

extern "C" {

int pdc_highest_peak_dev(int device, void *stream, const double *d_power, int64_t n_curves,
                         int64_t nf, int64_t *d_idx, double *d_val) {
    PDC_REQUIRE(d_power || n_curves * nf == 0, "highest_peak: power is NULL");
    PDC_REQUIRE(d_idx || d_val, "highest_peak: no output requested");
    PDC_REQUIRE(n_curves >= 0 && nf >= 0 && n_curves < ((int64_t)1 << 31), "highest_peak: bad size");
    if (n_curves == 0) return PDC_OK;
    PDC_TRY(use_device(device));
    hipStream_t st = (hipStream_t)stream;
    // few long rows: several workgroups per row (shares of >= 16384 bins, ~2048 workgroups in all) + a merge
    int64_t segs = 2048 / n_curves;
    segs = segs < nf / 16384 ? segs : nf / 16384;
    if (segs > 1) {
        void *sp = nullptr;
        ScratchPin pin;
        PDC_TRY(pin.take(device, st, n_curves * segs * 16, &sp));
        double *part_v = static_cast<double *>(sp);
        long long *part_i = reinterpret_cast<long long *>(part_v + n_curves * segs);
        hipLaunchKernelGGL(highest_peak_kernel, dim3((unsigned)(n_curves * segs)), dim3(kBlock), 0, st, d_power, nf, (int)segs,
                           d_idx, d_val, part_v, part_i);
        hipLaunchKernelGGL(highest_peak_merge_kernel, dim3((unsigned)n_curves), dim3(64), 0, st, part_v, part_i, (int)segs, d_idx, d_val);
    } else {
        hipLaunchKernelGGL(highest_peak_kernel, dim3((unsigned)n_curves), dim3(kBlock), 0, st, d_power, nf, 1, d_idx, d_val,
                           static_cast<double *>(nullptr), static_cast<long long *>(nullptr));
    }
    PDC_HIP(hipGetLastError());
    return PDC_OK;
}

int pdc_highest_peak(const double *power, int64_t n_curves, int64_t nf, int64_t *idx_out,
                     double *val_out, int device) {
    PDC_REQUIRE(power || n_curves * nf == 0, "highest_peak: power is NULL");
    PDC_REQUIRE(idx_out || val_out, "highest_peak: no output requested");
    PDC_REQUIRE(n_curves >= 0 && nf >= 0, "highest_peak: negative size");
    if (n_curves == 0) return PDC_OK;
    HostCall hc(device);
    double *d_p = hc.in(SLOT_OUT0, power, n_curves * nf * 8);
    int64_t *d_i = hc.out<int64_t>(SLOT_OUT1, n_curves * 8);
    double *d_v = hc.out<double>(SLOT_OUT2, n_curves * 8);
    PDC_TRY(hc.status);
    PDC_TRY(pdc_highest_peak_dev(device, hc.stream(), d_p, n_curves, nf, d_i, d_v));
    hc.back(idx_out, d_i, n_curves * 8);
    hc.back(val_out, d_v, n_curves * 8);
    return hc.finish();
}

namespace {

int launch_topk(hipStream_t st, PeakArgs a, int64_t n_curves) {
    PDC_REQUIRE(a.nf < ((int64_t)1 << 31), "peaks_topk: at most 2^31-1 bins per spectrum");
    int sh = kPkFusedShift;
    while (((a.nf + ((int64_t)1 << sh) - 1) >> sh) > kPkMaxBlocks) ++sh;
    a.blk_shift = sh;
    a.nblk = (a.nf + ((int64_t)1 << sh) - 1) >> sh;
    // LDS: 20 KB of candidate slots + 3 KB of block extrema at 5e4 bins
    const size_t lds = TopkLds::bytes(a.nblk);
    PDC_REQUIRE(lds <= 150 * 1024, "peaks_topk: %lld bins per spectrum need %zu bytes of LDS", (long long)a.nf, lds);
    auto launch = [&](auto sort) -> int {
        constexpr bool SORT = decltype(sort)::value;
        PDC_TRY(allow_dynamic_lds((const void *)peaks_topk_kernel<SORT>, 150 * 1024));
        hipLaunchKernelGGL(peaks_topk_kernel<SORT>, dim3((unsigned)n_curves), dim3(kPkBlock), lds, st, a);
        PDC_HIP(hipGetLastError());
        return PDC_OK;
    };
    // (the later launches of a call rank after the launch before: that logic lives in the SORT instance only, so the
    // few-ranks instance keeps the 80 registers of six workgroups per CU)
    return a.k > kPkSortFrom || a.k_off > 0 ? launch(std::true_type{}) : launch(std::false_type{});
}

// the checks the three top-k entries share
int topk_validate(const char *who, int k, bool any_output) {
    PDC_REQUIRE(k >= 1 && k <= kPkMaxKTotal, "%s: k must be 1..%d", who, kPkMaxKTotal);
    PDC_REQUIRE(any_output, "%s: no output requested", who);
    return PDC_OK;
}

}  // namespace

int pdc_peaks_topk_dev(int device, void *stream, const double *d_power, int64_t n_curves, int64_t nf,
                       int k, int by_prominence, int64_t *d_count, int64_t *d_idx, double *d_height,
                       double *d_prominence, int64_t *d_half_lo, int64_t *d_half_hi) {
    PDC_REQUIRE(d_power || n_curves * nf == 0, "peaks_topk: power is NULL");
    PDC_TRY(topk_validate("peaks_topk", k, d_count || d_idx || d_height || d_prominence || d_half_lo || d_half_hi));
    PDC_REQUIRE(k <= kPkMaxK || (d_idx && (by_prominence ? d_prominence != nullptr : d_height != nullptr)),
                "peaks_topk: k > %d is ranked in chunks of %d, each after the chunk before: the indices and the ranking key's "
                "output (heights, or prominences) must be requested", kPkMaxK, kPkMaxK);
    PDC_REQUIRE(n_curves >= 0 && nf >= 0 && n_curves < ((int64_t)1 << 31), "peaks_topk: bad size");
    if (n_curves == 0) return PDC_OK;
    PDC_TRY(use_device(device));
    PeakArgs a;
    a.power = d_power;
    a.nf = nf;
    a.k = k;
    a.by_prominence = by_prominence ? 1 : 0;
    a.count = (long long *)d_count;
    a.idx = (long long *)d_idx;
    a.half_lo = (long long *)d_half_lo;
    a.half_hi = (long long *)d_half_hi;
    a.height = d_height;
    a.prom = d_prominence;
    a.k_total = k;
    // k > 128: one launch per 128 ranks; launch c ranks what comes after column 128 c - 1 of the outputs (every launch
    // sweeps the spectra again: ~1.2 ms per 64 ranks by height for the 1.64 GB of a C3 batch, 2-3 ms by prominence)
    for (int off = 0; off < k; off += kPkMaxK) {
        a.k = k - off < kPkMaxK ? k - off : kPkMaxK;
        a.k_off = off;
        a.count = off == 0 ? (long long *)d_count : nullptr;
        PDC_TRY(launch_topk((hipStream_t)stream, a, n_curves));
    }
    return PDC_OK;
}

namespace {

// device slots of the k-wide outputs + D2H + the wait; shared by the two host entry points
int topk_outputs(HostCall &hc, const double *d_pow, int64_t n_curves, int64_t nf, int k, int by_prominence, int64_t *count,
                 int64_t *idx, double *height, double *prom, int64_t *half_lo, int64_t *half_hi) {
    const int64_t nk = n_curves * k;
    // one cached block: count | idx | lo | hi | height | prom
    int64_t *d_count = hc.out<int64_t>(SLOT_OUT1, (n_curves + 5 * nk) * 8);
    PDC_TRY(hc.status);
    int64_t *d_idx = d_count + n_curves, *d_lo = d_idx + nk, *d_hi = d_lo + nk;
    double *d_h = (double *)(d_hi + nk), *d_p = d_h + nk;
    PDC_TRY(pdc_peaks_topk_dev(hc.device, hc.stream(), d_pow, n_curves, nf, k, by_prominence, d_count, d_idx, d_h, d_p,
                               (half_lo || half_hi) ? d_lo : nullptr, (half_lo || half_hi) ? d_hi : nullptr));
    hc.back(count, d_count, n_curves * 8);
    hc.back(idx, d_idx, nk * 8);
    hc.back(height, d_h, nk * 8);
    hc.back(prom, d_p, nk * 8);
    hc.back(half_lo, d_lo, nk * 8);
    hc.back(half_hi, d_hi, nk * 8);
    return hc.finish();
}

}  // namespace

int pdc_peaks_topk(const double *power, int64_t n_curves, int64_t nf, int k, int by_prominence,
                   int64_t *count_out, int64_t *idx_out, double *height_out, double *prominence_out,
                   int64_t *half_lo_out, int64_t *half_hi_out, int device) {
    PDC_REQUIRE(power || n_curves * nf == 0, "peaks_topk: power is NULL");
    PDC_TRY(topk_validate("peaks_topk", k, count_out || idx_out || height_out || prominence_out || half_lo_out || half_hi_out));
    PDC_REQUIRE(n_curves >= 0 && nf >= 0, "peaks_topk: negative size");
    if (n_curves == 0) return PDC_OK;
    HostCall hc(device);
    double *d_p = hc.in(SLOT_OUT0, power, n_curves * nf * 8);
    return topk_outputs(hc, d_p, n_curves, nf, k, by_prominence, count_out, idx_out, height_out, prominence_out, half_lo_out,
                        half_hi_out);
}

// Batched periodograms reduced on the device to their k highest (or most prominent) peaks with
// prominences and half-maximum crossings: 4096 x 5e4 spectra stay in HBM, O(B k) values come back.
int pdc_gls_batch_peaks(const double *t, const double *y, const double *dy, const int64_t *offsets,
                        int64_t n_curves, int shared_t, double f0, double delta, int64_t nf, int fit_mean,
                        int psd, int k, int by_prominence, int64_t *count_out, int64_t *idx_out,
                        double *height_out, double *prominence_out, int64_t *half_lo_out,
                        int64_t *half_hi_out, int device) {
    PDC_REQUIRE(t && y && offsets, "gls_batch_peaks: NULL argument");
    PDC_REQUIRE(n_curves >= 1 && nf >= 0, "gls_batch_peaks: bad size");
    PDC_TRY(topk_validate("gls_batch_peaks", k, true));   // (it asks pdc_peaks_topk_dev for every table itself)
    GlsBatchIn in;
    PDC_TRY(in.check("gls", offsets, n_curves, shared_t));
    HostCall hc(device);
    const int64_t wb = pdc_gls_work_bytes(in.n_total, n_curves, nf);
    in.upload(hc, t, y, dy, offsets, n_curves);
    double *d_pow = hc.out<double>(SLOT_OUT0, n_curves * nf * 8);
    void *d_work = hc.reserve(SLOT_WORK, wb);
    PDC_TRY(hc.status);
    PDC_TRY(pdc_gls_scan_dev(device, hc.stream(), in.d_t, in.d_y, in.d_dy, in.d_off, in.n_total, n_curves, shared_t, f0, delta,
                             0, nf, fit_mean, psd, d_pow, nullptr, nullptr, d_work, wb));
    return topk_outputs(hc, d_pow, n_curves, nf, k, by_prominence, count_out, idx_out, height_out, prominence_out, half_lo_out,
                        half_hi_out);
}

// Batched periodograms reduced on the device to the highest peak of each (index into the grid and
// power there): the spectra never leave HBM.
int pdc_gls_batch_highest_peak(const double *t, const double *y, const double *dy,
                               const int64_t *offsets, int64_t n_curves, int shared_t, double f0,
                               double delta, int64_t nf, int fit_mean, int psd, int64_t *idx_out,
                               double *val_out, int device) {
    PDC_REQUIRE(t && y && offsets && (idx_out || val_out), "gls_batch_highest_peak: NULL argument");
    PDC_REQUIRE(n_curves >= 1 && nf >= 0, "gls_batch_highest_peak: bad size");
    GlsBatchIn in;
    PDC_TRY(in.check("gls", offsets, n_curves, shared_t));
    HostCall hc(device);
    const int64_t wb = pdc_gls_work_bytes(in.n_total, n_curves, nf);
    in.upload(hc, t, y, dy, offsets, n_curves);
    double *d_pow = hc.out<double>(SLOT_OUT0, n_curves * nf * 8);
    int64_t *d_i = hc.out<int64_t>(SLOT_OUT1, n_curves * 8);
    double *d_v = hc.out<double>(SLOT_OUT2, n_curves * 8);
    void *d_work = hc.reserve(SLOT_WORK, wb);
    PDC_TRY(hc.status);
    PDC_TRY(pdc_gls_scan_dev(device, hc.stream(), in.d_t, in.d_y, in.d_dy, in.d_off, in.n_total, n_curves, shared_t, f0, delta,
                             0, nf, fit_mean, psd, d_pow, nullptr, nullptr, d_work, wb));
    PDC_TRY(pdc_highest_peak_dev(device, hc.stream(), d_pow, n_curves, nf, d_i, d_v));
    hc.back(idx_out, d_i, n_curves * 8);
    hc.back(val_out, d_v, n_curves * 8);
    return hc.finish();
}

}  // extern "C"
