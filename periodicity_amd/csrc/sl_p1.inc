// P1 of a period of sl_fast_kernel's one-slice instances, sl_duo_kernel and sl_duo_ragged_kernel: exact phases, coarse
// histogram, bucket ids packed in registers (two 16-bit ids per word of pk[]), exclusive scan - TEXT, included in the body
// of the three kernels, because the same statements inside a __device__ function compile differently (the bucket of a
// sample past the end becomes a select where the kernel text has a branch around the fold's last steps) and the large
// single-call shapes lose 0.7 - 0.8 % by it: DESIGN.md 4.3c.  Every other phase of a period is a function of sl_period.h.
// It reads: v (the PeriodLds view), p1_t (const double *: the curve's times), n, period, y, safe, tid (the kernel's opaque
// copy of the thread id), lane, wave_tot, the constants KMAX, P1_BLK (block size), P1_NB (coarse buckets), PDC_SL_G1;
// it writes pk[(KMAX + 1) / 2] (declared by the kernel) and, in LDS, hist[b] = first sorted position of bucket b and
// defer[0..15] ([15]: next range to hand out in P3a).
// Samples past the end go to one of 64 dummy buckets behind the histogram.  Groups of PDC_SL_G1 coalesced loads, the next
// group requested before this one is folded; the scheduling barrier keeps the <= 52 loads from being hoisted to the top.
        static_assert(decltype(v)::template holds_histogram<P1_NB>, "aliases must fit: the coarse histogram");
        static_assert(PDC_SL_G1 % 4 == 0, "phases are computed four at a time");
        for (int b = tid; b < P1_NB + 64; b += P1_BLK) v.hist[b] = 0u;
        if (tid < 16) v.defer[tid] = tid == 15 ? (unsigned)(P1_BLK / 64) : 0u;   // [15]: next range to hand out (P3a)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < (KMAX + 1) / 2; ++k) pk[k] = 0u;
        double tv[PDC_SL_G1], tn[PDC_SL_G1];
#pragma unroll
        for (int u = 0; u < PDC_SL_G1; ++u) {
            const int i = u * P1_BLK + tid;
            tn[u] = p1_t[i < n ? i : n - 1];
        }
#pragma unroll
        for (int k0 = 0; k0 < KMAX; k0 += PDC_SL_G1) {
            if (k0 * P1_BLK < n) {   // workgroup-uniform
#pragma unroll
                for (int u = 0; u < PDC_SL_G1; ++u) tv[u] = tn[u];
                if (k0 + PDC_SL_G1 < KMAX && (k0 + PDC_SL_G1) * P1_BLK < n) {
#pragma unroll
                    for (int u = 0; u < PDC_SL_G1; ++u) {
                        const int i = (k0 + PDC_SL_G1 + u) * P1_BLK + tid;
                        if (k0 + PDC_SL_G1 + u < KMAX) tn[u] = p1_t[i < n ? i : n - 1];
                    }
                }
                double phi[PDC_SL_G1];
#pragma unroll
                for (int q = 0; q < PDC_SL_G1; q += 4) {
                    double t4[4] = {tv[q], tv[q + 1], tv[q + 2], tv[q + 3]}, p4[4];
                    phases4(t4, period, y, safe, p4);
#pragma unroll
                    for (int u = 0; u < 4; ++u) phi[q + u] = p4[u];
                }
#pragma unroll
                for (int u = 0; u < PDC_SL_G1; ++u) {
                    if (k0 + u < KMAX) {
                        const int i = (k0 + u) * P1_BLK + tid;
                        const int b = i < n ? coarse_of<P1_NB>(phi[u]) : P1_NB + lane;
                        atomicAdd(&v.hist[b], 1u);
                        pk[(k0 + u) >> 1] |= (unsigned)b << (((k0 + u) & 1) * 16);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        scan_buckets<P1_NB, P1_BLK>(v.hist, wave_tot);
