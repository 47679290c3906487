// The per-period body of the two-workgroups-per-CU StringLength kernels (namespace duo): P1 (exact phases, coarse
// histogram), P2 (the permutation, the range table), P3a (sl_ranges.inc), P3b (deferred ranges), P3c (links + the
// closing segment), the workgroup sum and the period's result - included, textually, in sl_duo_kernel and in its
// ragged counterpart sl_duo_ragged_kernel (sl_ragged.inc), so that a period runs the SAME code in both.
// Names expected in scope: a (.t, .m, .periods, .rec, .ell, .todo: this curve's arrays), p (the period's index in
// them), n (samples), t_safe, marked (unsigned *: the counter of periods left to the one-workgroup kernel), rsum /
// rcnt / rlen (this workgroup's range scratch), the LDS views of the kernel (hist, bkeys, bidx, bndb, bnds, defer,
// order, keys_w, fine_w, idx_w, wave_tot, red, s_bad), tid0, lane, wave and the template parameters KMAX, NBL, kB,
// kW, kDCap.
        const double period = a.periods[p];
        const double y = 1.0 / period;
        const bool safe = period_is_safe(period, t_safe);
        double total = 0.0;

        // ---- P1: exact phases, coarse histogram; bucket ids in registers ------------------------------
        // (as in sl_fast_kernel: opaque copy of the thread id, dummy buckets for samples past the end)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        for (int b = tid; b < NBL + 64; b += kB) hist[b] = 0u;
        if (tid < 16) defer[tid] = tid == 15 ? (unsigned)kW : 0u;   // [15]: next range to hand out (P3a)
        __syncthreads();
        unsigned pk[(KMAX + 1) / 2];
#pragma unroll
        for (int k = 0; k < (KMAX + 1) / 2; ++k) pk[k] = 0u;
        double tv[4], tn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = u * kB + tid;
            tn[u] = a.t[i < n ? i : n - 1];
        }
#pragma unroll
        for (int k0 = 0; k0 < KMAX; k0 += 4) {
            if (k0 * kB < n) {   // workgroup-uniform
#pragma unroll
                for (int u = 0; u < 4; ++u) tv[u] = tn[u];
                if (k0 + 4 < KMAX && (k0 + 4) * kB < n) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = (k0 + 4 + u) * kB + tid;
                        tn[u] = a.t[i < n ? i : n - 1];
                    }
                }
                double phi[4];
                phases4(tv, period, y, safe, phi);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (k0 + u < KMAX) {
                        const int i = (k0 + u) * kB + tid;
                        const int b = i < n ? coarse_of<NBL>(phi[u]) : NBL + lane;
                        atomicAdd(&hist[b], 1u);
                        pk[(k0 + u) >> 1] |= (unsigned)b << (((k0 + u) & 1) * 16);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        scan_buckets<NBL, kB>(hist, wave_tot);   // hist[b] = first sorted position of bucket b
        const int slice_n = n;

        // ---- P2: the permutation, grouped by coarse bucket ----------------------------------------
#pragma unroll
        for (int k0 = 0; k0 < KMAX; k0 += 4) {
            if (k0 * kB < n) {   // workgroup-uniform
                unsigned pos[4], bb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (k0 + u < KMAX) {
                        bb[u] = (pk[(k0 + u) >> 1] >> (((k0 + u) & 1) * 16)) & 0xFFFFu;
                        pos[u] = atomicAdd(&hist[bb[u]], 1u);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (k0 + u < KMAX) {
                        const int i = (k0 + u) * kB + tid;
                        order[i < n ? pos[u] : (unsigned)(n + lane)] = (IdxT)i;
                    }
                }
            }
        }
        const int nranges = (slice_n + kFWin - 1) / kFWin;
        __syncthreads();   // hist[b] = END position of bucket b
        // range r starts at the first bucket whose start position is >= r * kFWin
        for (int r = tid; r <= nranges; r += kB) {
            int b = 0, s0 = 0;
            if (r > 0) {
                const unsigned x = (unsigned)r * kFWin;
                int l = 0, h = NBL;   // smallest j in [0, NBL) with end(j) >= x, NBL if none
                while (l < h) {
                    const int mid = (l + h) >> 1;
                    if (hist[mid] >= x) h = mid; else l = mid + 1;
                }
                b = l < NBL ? l + 1 : NBL;
                s0 = l < NBL ? (int)hist[l] : slice_n;
            }
            bndb[r] = (unsigned short)b;
            bnds[r] = (unsigned short)s0;
        }
        __syncthreads();   // (the histogram is dead from here on: its LDS becomes wave scratch)

        // ---- P3a: wave-autonomous ranges (the same code as sl_fast_kernel's, on this workgroup's 8 waves) --
        constexpr int NB = NBL;
        const int r_base = 0;
#define PDC_ORDER_GET(pos) ((unsigned)order[pos])
        constexpr bool kEmitSorted = false;
        rec_t *const emit_row = nullptr;
        const int emit_at = 0;
#include "sl_ranges.inc"
#undef PDC_ORDER_GET
        if (wave < nranges) request(wave);
        for (int r = wave; r < nranges; r = r_next) {
            if (n_cnt > 192) process(r, std::true_type{});
            else process(r, std::false_type{});
        }
        __syncthreads();

        // ---- P3b: deferred ranges, whole workgroup (LDS sort; larger ones mark the period) ----------
        for (int w32 = 0; w32 < (nranges + 31) / 32; ++w32) {
            unsigned bits = defer[w32];
            while (bits) {
                const int r = w32 * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                const int s_lo = bnds[r], cnt = (int)bnds[r + 1] - s_lo;
                if (cnt > kDCap) {      // (workgroup-uniform)
                    if (tid == 0) s_bad = 1u;
                    continue;
                }
                int P = 2;
                while (P < cnt) P <<= 1;
                for (int sI = tid; sI < P; sI += kB) {
                    if (sI < cnt) {
                        const IdxT id = order[s_lo + sI];
                        bkeys[sI] = phase_key(fast_phase(a.t[id], period, y, safe));
                        bidx[sI] = id;
                    } else {
                        bkeys[sI] = ~0ull;
                        bidx[sI] = (IdxT)~0u;
                    }
                }
                __syncthreads();
                bitonic_sort<IdxT>(bkeys, bidx, P);
                total += segment_sum(bkeys, bidx, cnt, a.m);
                if (tid == 0) {
                    rsum[(int64_t)r * 4 + 0] = __longlong_as_double((long long)bkeys[0]);
                    rsum[(int64_t)r * 4 + 1] = a.m[bidx[0]];
                    rsum[(int64_t)r * 4 + 2] = __longlong_as_double((long long)bkeys[cnt - 1]);
                    rsum[(int64_t)r * 4 + 3] = a.m[bidx[cnt - 1]];
                    rcnt[r] = cnt;
                    rlen[r] = 0.0;   // (its segments were added to `total` by the whole workgroup, in a fixed order)
                }
                __syncthreads();
            }
        }
        __syncthreads();  // every summary of this item (global, this workgroup's) is visible

        // ---- P3c: links between consecutive non-empty ranges + the closing segment -----------------------
        for (int r = tid; r < nranges; r += kB) {
            if (rcnt[r] > 0) {
                total += rlen[r];
                int q = r - 1;
                while (q >= 0 && rcnt[q] == 0) --q;
                if (q >= 0)
                    total += hypot(rsum[(int64_t)r * 4 + 1] - rsum[(int64_t)q * 4 + 3],
                                   rsum[(int64_t)r * 4 + 0] - rsum[(int64_t)q * 4 + 2]);
            }
        }
        if (tid == 0 && nranges > 0) {
            int f0 = 0, l0 = nranges - 1;
            while (f0 < nranges && rcnt[f0] == 0) ++f0;
            while (l0 >= 0 && rcnt[l0] == 0) --l0;
            // closing segment of np.roll(-1): first minus last, no phase wrap (phase.py:50)
            if (f0 < nranges && l0 >= 0)
                total += hypot(rsum[(int64_t)f0 * 4 + 1] - rsum[(int64_t)l0 * 4 + 3],
                               rsum[(int64_t)f0 * 4 + 0] - rsum[(int64_t)l0 * 4 + 2]);
        }
        total = wave_sum(total);
        if (lane == 0) red[wave] = total;
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int w = 0; w < kW; ++w) sum += red[w];
            a.todo[p] = s_bad ? 1 : 0;
            if (s_bad) atomicAdd(marked, 1u);
            else a.ell[p] = sum;
        }
