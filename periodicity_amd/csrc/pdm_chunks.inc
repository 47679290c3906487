// The sample loop of pdm_scan_kernel - included, textually, in its body and in pdm_ragged_scan_kernel's so that
// both bin the samples with the SAME code: stage [s_begin, s_end) of a.t / a.x through LDS, add every sample to
// this thread's private histogram of its trial period, then (SPLIT > 1) fold the parts into part 0 in a fixed
// order.  Names it reads from the including body: a (.t, .x), s_begin, s_end, mean, period, rp, dm0, thr, m0, mag,
// nbins, ncw, stage, hsum, hcnt, edge, tid, part, q_over, q_nan and the template parameters BLOCK, SPLIT, KIND, CE, GL.
    for (int64_t base = s_begin; base < s_end; base += kChunk) {
        __syncthreads();
        for (int i = tid; i < kChunk; i += BLOCK) {
            const int64_t g = base + i;
            double2 v = g < s_end ? make_double2(a.t[g], GL ? 0.0 : (CE ? a.x[g] : a.x[g] - mean)) : make_double2(0.0, 0.0);
            if (KIND == 2 && !(v.y >= 0.0 && v.y < (double)mag)) {
                // the magnitude bin is the caller's double and indexes the cell histogram: anything outside
                // 0 .. mag-1 (NaN included) is staged with a NaN time - its phase is NaN, so it takes the exact
                // path and counts nowhere, exactly as if the sample were absent (the host entries reject such
                // input; `_dev` callers get this).  Checked once per staged sample, not once per pair.
                v = make_double2(__builtin_nan(""), 0.0);
            }
            stage[i] = v;
        }
        __syncthreads();
        const int cnt = (int)((s_end - base) < kChunk ? (s_end - base) : kChunk);
        const int i_end = cnt < (part + 1) * (kChunk / SPLIT) ? cnt : (part + 1) * (kChunk / SPLIT);
        // two samples per trip: two independent read -> bin -> atomic chains in flight per wave.
        // Fast path: 7 VALU ops (v_fract_f64 twice); the histogram update is unconditional.
        auto fast_bin = [&](const double t, int &k) -> bool {
            const double u = __builtin_amdgcn_fract(t * rp) * dm0;
            k = (int)u;
            return __builtin_fabs(__builtin_amdgcn_fract(u) - 0.5) < thr;
        };
        // exact path: numpy's float remainder of the IEEE quotient, explicit edges; a NaN phase
        // belongs to no bin (adds zero to bin 0)
        auto exact_bin = [&](const double2 tx, int &k, double &val, unsigned &inc) {
            const double qe = tx.x / period;
            const double phi = qe - __builtin_floor(qe);  // == fmod-based Python % for divisor 1
            if (phi != phi) {
                q_nan += tx.y * tx.y;
                k = 0;
                val = 0.0;
                inc = 0u;
                return;
            }
            k = (int)(phi * dm0);
            k = k < 0 ? 0 : (k > m0 ? m0 : k);
            while (k > 0 && phi < edge[k]) --k;
            while (k < m0 && phi >= edge[k + 1]) ++k;
            if (k == m0) q_over += tx.y * tx.y;
        };
        auto add = [&](const int k, const double val, const unsigned inc) {
            if (CE) {   // val = the sample's magnitude bin (range-checked when staged); a NaN phase (inc == 0) counts nowhere
                const int cell = k * mag + (int)val;
                atomicAdd(&hcnt[(cell >> 1) * BLOCK + tid], inc << ((cell & 1) * 16));
            } else {
                atomicAdd(&hsum[k * BLOCK + tid], val);
                atomicAdd(&hcnt[k * BLOCK + tid], inc);
            }
        };
        auto update = [&](const double2 tx) {
            int k;
            double val = tx.y;
            unsigned inc = 1u;
            if (!fast_bin(tx.x, k)) exact_bin(tx, k, val, inc);
            add(k, val, inc);
        };
        int i = part * (kChunk / SPLIT);
        // the samples of the next trip are read before this trip's histogram atomics go out (the compiler
        // cannot move an LDS read above a possibly aliasing LDS atomic by itself); the staging area
        // is followed by the histograms, so reading a few entries past the chunk is harmless
        {   // four samples per trip: four independent read -> bin -> atomic chains in flight per wave (two per
            // trip measured 3.5-8 % slower on one box); the next four are read before this trip's atomics go out
            double2 n0 = stage[i], n1 = stage[i + 1], n2 = stage[i + 2], n3 = stage[i + 3];
            for (; i + 3 < i_end; i += 4) {
                const double2 t0 = n0, t1 = n1, t2 = n2, t3 = n3;
                n0 = stage[i + 4];
                n1 = stage[i + 5];
                n2 = stage[i + 6];
                n3 = stage[i + 7];
                int k0, k1, k2, k3;
                double v0 = t0.y, v1 = t1.y, v2 = t2.y, v3 = t3.y;
                unsigned i0 = 1u, i1 = 1u, i2 = 1u, i3 = 1u;
                const bool f0 = fast_bin(t0.x, k0), f1 = fast_bin(t1.x, k1), f2 = fast_bin(t2.x, k2), f3 = fast_bin(t3.x, k3);
                if (!f0) exact_bin(t0, k0, v0, i0);
                add(k0, v0, i0);
                if (!f1) exact_bin(t1, k1, v1, i1);
                add(k1, v1, i1);
                if (!f2) exact_bin(t2, k2, v2, i2);
                add(k2, v2, i2);
                if (!f3) exact_bin(t3, k3, v3, i3);
                add(k3, v3, i3);
            }
        }
        double2 na = stage[i], nb2 = stage[i + 1];
        for (; i + 1 < i_end; i += 2) {
            // both fast bins first: two independent dependency chains back to back
            const double2 ta = na, tb = nb2;
            na = stage[i + 2];
            nb2 = stage[i + 3];
            int ka, kb;
            double va = ta.y, vb = tb.y;
            unsigned ia = 1u, ib = 1u;
            const bool fa = fast_bin(ta.x, ka), fb = fast_bin(tb.x, kb);
            if (!fa) exact_bin(ta, ka, va, ia);
            add(ka, va, ia);
            if (!fb) exact_bin(tb, kb, vb, ib);
            add(kb, vb, ib);
        }
        for (; i < i_end; ++i) update(stage[i]);
    }

    if (SPLIT > 1) {
        // fold the partial histograms of parts 1..SPLIT-1 into part 0 (threads tid + 64*q)
        __syncthreads();
        double *qx = reinterpret_cast<double *>(stage);  // q_over / q_nan exchange, [2][BLOCK]
        qx[tid] = q_over;
        qx[BLOCK + tid] = q_nan;
        __syncthreads();
        if (part == 0) {
            for (int q = 1; q < SPLIT; ++q) {
                const int other = tid + 64 * q;
                for (int k = 0; k < nbins; ++k)
                    if (!CE) hsum[k * BLOCK + tid] += hsum[k * BLOCK + other];
                for (int k = 0; k < ncw; ++k) hcnt[k * BLOCK + tid] += hcnt[k * BLOCK + other];   // (fields cannot carry)
                q_over += qx[other];
                q_nan += qx[BLOCK + other];
            }
        }
    }
