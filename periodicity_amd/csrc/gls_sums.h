// The device-side skeleton of the GLS direct sums, one copy: the prologue arithmetic (weights, weighted mean, the
// 48-byte sample record and the two spare ones), the XCD order of the tiles, a chunk row of the rotation
// tables, the two-set scalar pipeline over a chunk's samples, the walk of a thread's K grid frequencies, the loop that
// runs these over a stretch of samples chunk by chunk, and the NaN-aware (max, lowest index) fold.  Everything here is
// inlined into its caller: the kernels, their launch shapes and their registers are the callers' own.
//
// Each piece encodes a rule that every caller must keep in the same way:
//   - sums are taken in one fixed order (per-thread stride loop, wave tree, waves in order): bitwise reproducible;
//   - phases are reduced in cycles with the exact product (frac_product) before any sincos;
//   - maxima follow np.nanargmax: NaN never wins, the first of equal maxima does;
//   - the pipeline reads one record and one table row past the stretch it accumulates.
//
// Who uses what.  The scan of gls_ragged.hip and the four harmonic-sum scans (mhgls.hip, mbgls.hip, htest.hip,
// htest_fdot.hip, with harmonic_sums.h on top) are scan_stretch with their own table fill and their own sums: mhgls and
// htest one stretch per workgroup, mbgls one per band, htest_fdot with the spin-down offset in its fill.  mhgls and
// mbgls take xcd_tile; their prologues and the H-test one take put_record and put_spare_records.  bls.hip and
// glsfft.hip take inv_var.
// The standing rule: a piece that raises the registers of an instance across an occupancy step, makes it spill, or
// slows it beyond the run-to-run spread is not used by that instance, and the piece is not bent to fit it.  Three cases:
//   - every scan kernel writes its tile preamble out: a shared frame for it cost the <12, 4, 256> H-test instances
//     their second wave per SIMD;
//   - mbgls.hip types its Chebyshev ladder out inside scan_stretch: through add_fourier_sums (harmonic_sums.h) the
//     sample loop of mbgls_scan_kernel<1, 4> came out in another order and ran over its bound;
//   - gls.hip takes rot2, walk_grid and inv_var (the wide prologue) only: gls_scan_kernel keeps its own table fill
//     (with the TIGHT / PAIR variants), pipeline, prologue and maxima, because the register allocation of that kernel -
//     the headline number - moves with the smallest change of the source around it (a local pointer to a table row
//     re-allocates 38 of its 60 instances), and its device assembly is required to stay byte-identical across a
//     refactor.  Each of those four pieces, called from here, changed it.
#pragma once
#include "pdc_device.h"

#include <type_traits>

namespace pdc {

// ---- prologue: spectral.py:99-108, 120 ---------------------------------------------------------------------------------
// w = err**-2, unit errors where dy is NULL
__device__ __forceinline__ double inv_var(const double *dy, int64_t i) {
    const double e = dy ? dy[i] : 1.0;
    return 1.0 / (e * e);
}

// W = w.sum() and, with fit_mean, ybar = np.dot(w / w.sum(), values) (0 without), by one BLOCK-thread workgroup.
template <int BLOCK>
__device__ __forceinline__ void weights_and_mean(const double *y, const double *dy, int64_t n, int fit_mean, double *red,
                                                 double &W, double &ybar) {
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += BLOCK) acc += inv_var(dy, i);
    W = block_sum<BLOCK>(acc, red);
    ybar = 0.0;
    if (fit_mean) {
        acc = 0.0;
        for (int64_t i = tid; i < n; i += BLOCK) acc += inv_var(dy, i) / W * y[i];
        ybar = block_sum<BLOCK>(acc, red);
    }
}

// One sample's record {wy, w, cos, sin, 2 cos (2 pi delta t'), t'}; wy and w as the scan wants them (scaled by
// sqrt(w) where it carries sqrt(w) sin / sqrt(w) cos).
__device__ __forceinline__ void put_record(double *rec_i, double wy, double w, double delta, double tp) {
    double sd, cd;
    sincos_cycles(frac_product(delta, tp), sd, cd);
    double2 *r = reinterpret_cast<double2 *>(rec_i);
    r[0] = make_double2(wy, w);
    r[1] = make_double2(cd, sd);
    r[2] = make_double2(cd + cd, tp);
}

// The two spare records behind the n real ones, which the pipeline's read-ahead may load: finite, never accumulated.
__device__ __forceinline__ void put_spare_records(double *rec, int64_t n, int tid) {
    if (tid < 2) {
        double2 *r = reinterpret_cast<double2 *>(rec + (n + tid) * 6);
        r[0] = r[1] = r[2] = make_double2(0.0, 0.0);
    }
}

// ---- a workgroup's tile of the frequency grid ---------------------------------------------------------------------------
// Workgroup p runs on XCD p % 8 (observed dispatch rule, used for speed only): a contiguous run of tiles per XCD.  The
// launch rounds the tiles up to a multiple of 8; a result >= tiles has no tile.
__device__ __forceinline__ int64_t xcd_tile(unsigned block, int64_t tiles) {
    const int64_t per_xcd = (tiles + 7) / 8;
    return (int64_t)(block % 8) * per_xcd + block / 8;
}

// ---- rotation tables ---------------------------------------------------------------------------------------------------
// plane rotation of {sin, cos} pairs: angle(x) + angle(y)
__device__ __forceinline__ double2 rot2(const double2 x, const double2 y) {
    return make_double2(__builtin_fma(x.x, y.y, x.y * y.x), __builtin_fma(x.y, y.y, -(x.x * y.x)));
}

// One sample's row of a chunk's tables, made by two neighbouring threads of a wave (`odd` tells them apart).
// Thread (col, lane) of the scan starts at phase theta_tile + (64 col + 8 a + b) Theta with a = lane / 8, b = lane % 8
// and Theta = 2 pi kdelta t', kdelta = K delta: its seed is row[8 col + a] rotated by row[8 COLS + b] instead of a
// sincos.  The even thread makes {sin, cos}(b Theta), b < 8 (one sincos, a chain of 6 rotations) and the tile's base
// phase f_tile t' (one sincos), times `scale` (sqrt(w) where the sums want it carried, else 1); the odd thread walks
// that base in steps of 8 Theta (one sincos, 8 COLS - 1 rotations).  Three software sincos per SAMPLE, whatever the
// tile holds.  `offset()`, where one is given, moves the tile's base phase by that many cycles (any finite value:
// sincos_cycles reduces it), base = frac(f_tile t') + offset(), added before the one sincos - for phases that are not
// linear in the frequency alone, such as the spin-down term of htest_fdot.hip.  Without one nothing is added.
struct NoOffset {};
template <int COLS, class Offset = NoOffset>
__device__ __forceinline__ void fill_rotation_tables(double2 *row, bool odd, double tp, double kdelta, double f_tile,
                                                     double scale, Offset offset = {}) {
    double2 step1, cur = make_double2(0.0, 0.0);
    if (!odd) {
        sincos_cycles(frac_product(kdelta, tp), step1.x, step1.y);
        row[COLS * 8] = make_double2(0.0, 1.0);
        row[COLS * 8 + 1] = step1;
        cur = step1;
#pragma unroll
        for (int q = 2; q < 8; ++q) {
            cur = rot2(cur, step1);
            row[COLS * 8 + q] = cur;
        }
        double base = frac_product(f_tile, tp);
        if constexpr (!std::is_same<Offset, NoOffset>::value) base += offset();
        sincos_cycles(base, cur.x, cur.y);
        cur.x *= scale;
        cur.y *= scale;
    } else {
        sincos_cycles(frac_product(8.0 * kdelta, tp), step1.x, step1.y);
    }
    double2 b0;
    b0.x = __shfl_xor(cur.x, 1, 64);
    b0.y = __shfl_xor(cur.y, 1, 64);
    if (odd) {
        row[0] = b0;
#pragma unroll
        for (int q = 1; q < COLS * 8; ++q) {
            b0 = rot2(b0, step1);
            row[q] = b0;
        }
    }
}

// ---- the two-set scalar pipeline ---------------------------------------------------------------------------------------
// Everything sample i + 1 needs is requested while sample i is accumulated; two samples per trip with two register
// sets (A, B) that swap roles, so the read-ahead costs no register copies.  The record fields are wave-uniform: they
// come through the scalar cache (s_load, constant address space) and feed the fmas as SGPR operands - no LDS or VGPR
// traffic for them; the two table entries are LDS reads.  Scalar loads return out of order, so the wait for set A
// (lgkmcnt(0)) sits right before the request for set B goes out.  What the read-ahead may touch: see scan_stretch.
using d4 = double __attribute__((ext_vector_type(4)));
using cd4 = __attribute__((address_space(4))) const d4;
using cdbl = __attribute__((address_space(4))) const double;

struct Ahead {
    d4 r;  // {wy, w, cos, sin (2 pi delta t')}
    double cd2;
    double2 qa, qt;
};
// sample i of the chunk whose first record is `rec` (wave-uniform) and whose table is `tab`
template <class Tab>
__device__ __forceinline__ Ahead fetch_sample(const Tab &tab, const double *rec, int i, int slot_a, int slot_b) {
    Ahead h;
    h.qa = tab[i][slot_a];
    h.qt = tab[i][slot_b];
    const cdbl *rp = reinterpret_cast<const cdbl *>(reinterpret_cast<uintptr_t>(rec)) + i * 6;
    h.r = reinterpret_cast<const cd4 *>(rp)[0];
    h.cd2 = rp[4];
    return h;
}
template <class Fetch, class Accumulate>
__device__ __forceinline__ void two_set_pipeline(int i_beg, int i_end, Fetch fetch, Accumulate accumulate) {
    Ahead A = fetch(i_beg);
    int i = i_beg;
    for (; i + 1 < i_end; i += 2) {
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): set A has arrived
        Ahead B = fetch(i + 1);
        __builtin_amdgcn_sched_barrier(0);
        accumulate(A);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        A = fetch(i + 2);
        __builtin_amdgcn_sched_barrier(0);
        accumulate(B);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (i < i_end) accumulate(A);
}

// A thread's K consecutive grid frequencies at one sample: per_frequency(k, s, c) for k = 0 .. K - 1, from the seed
// {s, c} of its first.  One plane rotation by the per-sample angle 2 pi delta t' makes the second; the others follow
// by the three-term recurrence x[k+1] = 2 cos(theta) x[k] - x[k-1] (one fma per component; rounding grows like
// K^2 eps, far below the 1e-6 gate for K <= 16).  Linear in the seed, so a seed scaled by sqrt(w) stays scaled.
template <int K, class PerFrequency>
__device__ __forceinline__ void walk_grid(const double2 seed, double cd, double sd, double cd2, PerFrequency per_frequency) {
    double s = seed.x, c = seed.y;
    double sp = 0.0, cp = 0.0;  // previous step of the recurrence
#pragma unroll
    for (int k = 0; k < K; ++k) {
        per_frequency(k, s, c);
        if (k + 1 < K) {
            double sn, cn;
            if (k == 0) {
                cn = __builtin_fma(c, cd, -(s * sd));
                sn = __builtin_fma(s, cd, c * sd);
            } else {
                cn = __builtin_fma(cd2, c, -cp);
                sn = __builtin_fma(cd2, s, -sp);
            }
            cp = c;
            sp = s;
            c = cn;
            s = sn;
        }
    }
}

// ---- a stretch of samples, chunk by chunk --------------------------------------------------------------------------------
// Samples [beg, end) of the records `recs` (n real ones), CHUNK at a time: the chunk's table rows are made by two
// threads per sample, fill(row, i, real) for sample i (`real`: i < n; a row past the curve is never accumulated, it
// only needs finite input), then every thread runs the pipeline over the chunk's samples and walks its K frequencies,
// per_frequency(h, k, s, c) with the sample's record in h.r.  Every thread of the workgroup must call it, with the
// same bounds (barriers).
// What the read-ahead may touch: up to two records past `end` - real ones where the stretch ends inside the curve, else
// the two spare records (put_spare_records) - and the table's padding row CHUNK.  None of it is accumulated.
template <int CHUNK, int K, class Tab, class Fill, class PerFrequency>
__device__ __forceinline__ void scan_stretch(Tab &tab, const double *recs, int64_t n, int64_t beg, int64_t end, int tid,
                                             int slot_a, int slot_b, Fill fill, PerFrequency per_frequency) {
    for (int64_t base = beg; base < end; base += CHUNK) {
        __syncthreads();   // everyone is done with the previous chunk's tables
        if (tid < 2 * CHUNK) {
            const int il = tid >> 1;
            fill(tab[il], base + il, base + il < n);
        }
        __syncthreads();
        const int cnt = (int)((end - base) < CHUNK ? (end - base) : CHUNK);
        const double *rec = recs + base * 6;
        two_set_pipeline(
            0, cnt, [&](const int i) { return fetch_sample(tab, rec, i, slot_a, slot_b); },
            [&](const Ahead &h) {
                walk_grid<K>(rot2(h.qa, h.qt), h.r[2], h.r[3], h.cd2,
                             [&](const int k, const double s, const double c) { per_frequency(h, k, s, c); });
            });
    }
}

// ---- NaN-aware maximum with its lowest index (np.nanargmax) ------------------------------------------------------------
// j < 0: nothing finite seen yet.  Threads, lanes and waves must hold ASCENDING index ranges: take and take_later keep
// the first of equal maxima by never replacing on a tie; wave_fold, where a later lane's range may interleave, compares
// the indices.
struct ArgMax {
    double v = 0.0;
    long long j = -1;
    __device__ __forceinline__ void take(double p, long long jp) {   // a bin
        if (p == p && (j < 0 || p > v)) {
            v = p;
            j = jp;
        }
    }
    __device__ __forceinline__ void take_later(double ov, long long oj) {   // a partial result over later indices
        if (oj >= 0 && (j < 0 || ov > v)) {
            v = ov;
            j = oj;
        }
    }
    __device__ __forceinline__ void wave_fold() {   // result in lane 0
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_down(v, o, 64);
            const long long oj = __shfl_down(j, o, 64);
            if (oj >= 0 && (j < 0 || ov > v || (ov == v && oj < j))) {
                v = ov;
                j = oj;
            }
        }
    }
    // wave_fold, then the WAVES waves in order through LDS: the result is in thread 0 (true there only)
    template <int WAVES>
    __device__ __forceinline__ bool block_fold(double *red_v, long long *red_i, int lane, int wave) {
        wave_fold();
        if (lane == 0) {
            red_v[wave] = v;
            red_i[wave] = j;
        }
        __syncthreads();
        if (threadIdx.x != 0) return false;
        for (int wv = 1; wv < WAVES; ++wv) take_later(red_v[wv], red_i[wv]);
        return true;
    }
};

}  // namespace pdc
