// The host side that the ragged-grid batches share (gls_ragged.hip, pdm_ragged.hip, sl_ragged.inc, bls_ragged.hip;
// declared in pdc_internal.h): the checks of offsets, tiles and pitch, the costliest-first dispatch order, the device
// slots with their shares, budgets, groups and threads, a group's view of the batch with its uploads and copies back,
// its metadata block, the peak-table arguments and each group's peak table: pdc_peaks_topk_dev on a pitched copy of the rows whose pad is NaN (why
// that keeps scipy's answers, and the one half-maximum artefact run_group removes: periodicity_hip.h).
#include "pdc_internal.h"

#include <algorithm>
#include <string>
#include <thread>

namespace pdc {

namespace {

int64_t tiles_of(int64_t rows, int64_t tile) { return (rows + tile - 1) / tile; }

int grow(RaggedSlot &s, int64_t bytes) {   // (on the slot's device) grow-only
    if (bytes < 256) bytes = 256;
    if (s.cap >= bytes) return PDC_OK;
    if (s.buf) PDC_HIP(hipFree(s.buf));
    s.buf = nullptr;
    s.cap = 0;
    PDC_TRY(device_alloc(&s.buf, bytes + bytes / 8));
    s.cap = bytes + bytes / 8;
    return PDC_OK;
}

int free_slots(RaggedSlots &r) {   // (caller holds r.mutex)
    for (RaggedSlot &s : r.slots) {
        PDC_HIP(hipSetDevice(s.device));
        if (s.stream) PDC_HIP(hipStreamDestroy(s.stream));
        if (s.buf) PDC_HIP(hipFree(s.buf));
    }
    r.slots.clear();
    r.devices.clear();
    return PDC_OK;
}

int64_t row_max_of(const RaggedBatch &j, int64_t c0, int64_t c1) {   // (0 without a peak table: no pitched copy)
    int64_t r = 0;
    for (int64_t b = c0; b < c1 && j.k > 0; ++b) r = std::max(r, j.rows_of(b));
    return r;
}

// Contiguous groups of [c0, c1) of at most `cap` bytes each (a curve that alone exceeds it is a group of its own);
// *largest = the bytes of the largest group.
std::vector<int64_t> make_groups(const RaggedBatch &j, int64_t c0, int64_t c1, int64_t cap, int64_t *largest) {
    std::vector<int64_t> cut{c0};
    *largest = 0;
    int64_t g0 = c0, row_max = 0;
    for (int64_t b = c0; b < c1; ++b) {
        const int64_t grown = j.k > 0 ? std::max(row_max, j.rows_of(b)) : 0;
        if (b > g0 && j.group_bytes(g0, b + 1, grown) > cap) {
            *largest = std::max(*largest, j.group_bytes(g0, b, row_max));
            cut.push_back(b);
            g0 = b;
            row_max = j.k > 0 ? j.rows_of(b) : 0;
        } else {
            row_max = grown;
        }
    }
    if (c1 > g0) *largest = std::max(*largest, j.group_bytes(g0, c1, row_max));
    cut.push_back(c1);
    return cut;
}

// One group on one slot, start to finish: the NaN fill of the pitched copy, the kind's launches, the peak table ranked
// and copied back, the stream synchronised, the pad's artefact removed.
int run_group(RaggedSlot &s, const RaggedBatch &j, int64_t c0, int64_t c1) {
    const int64_t B = c1 - c0, row_max = row_max_of(j, c0, c1), bytes = j.group_bytes(c0, c1, row_max);
    const int k = j.k;
    const int64_t nk = B * (int64_t)k;
    PDC_TRY(grow(s, bytes));
    hipStream_t st = s.stream;
    // the table is the buffer's tail: pitched [B][row_max] | count [B] | idx | half_lo | half_hi | height | prominence
    double *pitched = k > 0 ? (double *)((char *)s.buf + bytes - ragged_table_bytes(B, row_max, k)) : nullptr;
    if (k > 0) PDC_HIP(hipMemsetAsync(pitched, 0xff, (size_t)(B * row_max * 8), st));   // all-ones bytes: NaN
    PDC_TRY(j.run_group(s, c0, c1, row_max, pitched));
    if (k > 0) {
        int64_t *count = (int64_t *)((char *)pitched + up256(B * row_max * 8)), *idx = count + B, *lo = idx + nk,
                *hi = lo + nk;
        double *height = (double *)(hi + nk), *prom = height + nk;
        PDC_TRY(pdc_peaks_topk_dev(s.device, st, pitched, B, row_max, k, j.by_prominence, count, idx, height, prom, lo,
                                   hi));
        if (j.count) PDC_HIP(hipMemcpyAsync(j.count + c0, count, B * 8, hipMemcpyDeviceToHost, st));
        if (j.idx) PDC_HIP(hipMemcpyAsync(j.idx + c0 * k, idx, nk * 8, hipMemcpyDeviceToHost, st));
        if (j.height) PDC_HIP(hipMemcpyAsync(j.height + c0 * k, height, nk * 8, hipMemcpyDeviceToHost, st));
        if (j.prom) PDC_HIP(hipMemcpyAsync(j.prom + c0 * k, prom, nk * 8, hipMemcpyDeviceToHost, st));
        if (j.lo) PDC_HIP(hipMemcpyAsync(j.lo + c0 * k, lo, nk * 8, hipMemcpyDeviceToHost, st));
        if (j.hi) PDC_HIP(hipMemcpyAsync(j.hi + c0 * k, hi, nk * 8, hipMemcpyDeviceToHost, st));
    }
    PDC_HIP(hipStreamSynchronize(st));
    if (k > 0 && j.lo)   // the pad's one artefact: a sign flip of the pair (rows_b - 1, rows_b) is no crossing of the row
        for (int64_t b = c0; b < c1; ++b)
            for (int q = 0; q < k; ++q)
                if (j.lo[b * k + q] >= j.rows_of(b) - 1) j.lo[b * k + q] = -1;
    return PDC_OK;
}

}  // namespace

int ragged_validate(const char *what, const int64_t *offsets, const int64_t *rows, const char *rows_name,
                    int64_t n_curves, int64_t tile, const char *too_large, const std::function<int(int64_t)> &curve) {
    PDC_REQUIRE(n_curves >= 1 && n_curves < ((int64_t)1 << 31), "%s: n_curves must be 1 .. 2^31 - 1 (got %lld)", what,
                (long long)n_curves);
    PDC_REQUIRE(offsets[0] == 0 && rows[0] == 0, "%s: offsets[0] and %s[0] must be 0", what, rows_name);
    int64_t tiles = 0;
    for (int64_t b = 0; b < n_curves; ++b) {
        PDC_REQUIRE(offsets[b + 1] >= offsets[b], "%s: offsets must be non-decreasing (curve %lld)", what, (long long)b);
        PDC_REQUIRE(rows[b + 1] >= rows[b], "%s: %s must be non-decreasing (curve %lld)", what, rows_name, (long long)b);
        PDC_TRY(curve(b));
        tiles += tiles_of(rows[b + 1] - rows[b], tile);
    }
    PDC_REQUIRE(tiles < ((int64_t)1 << 31), "%s: %lld tiles of %lld %s", what, (long long)tiles, (long long)tile,
                too_large);
    return PDC_OK;
}

int ragged_check_pitch(const char *what, const int64_t *rows, int64_t n_curves, int64_t pitch, const char *unit) {
    for (int64_t b = 0; b < n_curves; ++b)
        PDC_REQUIRE(rows[b + 1] - rows[b] <= pitch, "%s: curve %lld has more %s than the pitch", what, (long long)b, unit);
    return PDC_OK;
}

int RaggedBatch::want_table(const char *what, int k_, int by_prominence_, int64_t *count_out, int64_t *idx_out,
                            double *height_out, double *prominence_out, int64_t *half_lo_out, int64_t *half_hi_out,
                            bool other_output) {
    PDC_REQUIRE(k_ >= 1 && k_ <= 1024, "%s: k must be 1..1024 (got %d)", what, k_);
    PDC_REQUIRE(count_out || idx_out || height_out || prominence_out || half_lo_out || half_hi_out || other_output,
                "%s: no output requested", what);
    k = k_;
    by_prominence = by_prominence_ ? 1 : 0;
    count = count_out;
    idx = idx_out;
    height = height_out;
    prom = prominence_out;
    lo = half_lo_out;
    hi = half_hi_out;
    return PDC_OK;
}

RaggedGroup::RaggedGroup(const RaggedBatch &j, const RaggedSlot &s, int64_t c0_, int64_t c1)
    : B(c1 - c0_), c0(c0_), s0(j.offsets[c0_]), n(j.offsets[c1] - s0), r0(j.rows[c0_]), nr(j.rows[c1] - r0),
      off((size_t)B + 1), roff((size_t)B + 1), buf(static_cast<char *>(s.buf)), st(s.stream) {
    for (int64_t b = 0; b <= B; ++b) {
        off[(size_t)b] = j.offsets[c0 + b] - s0;
        roff[(size_t)b] = j.rows[c0 + b] - r0;
    }
}

int RaggedGroup::upload(int64_t byte, const double *host) const {
    if (host && n > 0) PDC_HIP(hipMemcpyAsync(buf + byte, host + s0, (size_t)(n * 8), hipMemcpyHostToDevice, st));
    return PDC_OK;
}

int RaggedGroup::back(void *host, int64_t byte, int64_t bytes) const {
    if (host && bytes > 0) PDC_HIP(hipMemcpyAsync(host, buf + byte, (size_t)bytes, hipMemcpyDeviceToHost, st));
    return PDC_OK;
}

RaggedMeta::RaggedMeta(std::vector<int64_t> &host_, int arrays, int64_t n_curves, void *d_meta)
    : host(host_), B1(n_curves + 1), dev(static_cast<int64_t *>(d_meta)) {
    host.assign((size_t)(arrays * B1), 0);
}

void RaggedMeta::fill_offsets(const int64_t *offsets, const int64_t *rows) {
    std::copy(offsets, offsets + B1, i64(0));
    std::copy(rows, rows + B1, i64(1));
}

void RaggedMeta::fill_linspace(int column, const double *start, const double *step, const double *stop) {
    std::copy(start, start + B1 - 1, f64(column));
    std::copy(step, step + B1 - 1, f64(column + 1));
    std::copy(stop, stop + B1 - 1, f64(column + 2));
}

int RaggedMeta::upload(hipStream_t st, bool wait) {
    PDC_HIP(hipMemcpyAsync(dev, host.data(), host.size() * 8, hipMemcpyHostToDevice, st));
    if (wait) PDC_HIP(hipStreamSynchronize(st));
    return PDC_OK;
}

int64_t ragged_order(const int64_t *offsets, const int64_t *rows, int64_t n_curves, int64_t tile, int64_t *order,
                     int64_t *otile) {
    int64_t m = 0;
    for (int64_t b = 0; b < n_curves; ++b)
        if (rows[b + 1] > rows[b]) order[m++] = b;
    std::stable_sort(order, order + m, [&](int64_t x, int64_t y) {
        return offsets[x + 1] - offsets[x] > offsets[y + 1] - offsets[y];
    });
    otile[0] = 0;
    for (int64_t p = 0; p < m; ++p) otile[p + 1] = otile[p] + tiles_of(rows[order[p] + 1] - rows[order[p]], tile);
    return m;
}

int64_t ragged_table_bytes(int64_t n_curves, int64_t pitch, int k) {
    return k > 0 ? up256(n_curves * pitch * 8) + up256((n_curves + 5 * n_curves * (int64_t)k) * 8) : 0;
}

int RaggedSlots::release() {
    std::lock_guard<std::mutex> lk(mutex);
    return free_slots(*this);
}

int ragged_run(const char *what, RaggedSlots &r, const RaggedBatch &j, int64_t n_curves, const int *devices,
               int n_devices) {
    PDC_REQUIRE(devices && n_devices >= 1 && n_devices <= 64, "%s: 1 .. 64 device slots (got %d)", what, n_devices);
    for (int i = 0; i < n_devices; ++i) PDC_TRY(use_device(devices[i]));
    std::lock_guard<std::mutex> lk(r.mutex);
    if (r.devices != std::vector<int>(devices, devices + n_devices)) {
        PDC_TRY(free_slots(r));
        r.slots.resize((size_t)n_devices);
        for (int i = 0; i < n_devices; ++i) r.slots[(size_t)i].device = devices[i];
        r.devices.assign(devices, devices + n_devices);
    }
    // contiguous shares balanced by sum n_b rows_b (+ n_b + rows_b: the per-sample and per-row work)
    std::vector<double> pre((size_t)n_curves + 1, 0.0);
    for (int64_t b = 0; b < n_curves; ++b) {
        const double nb = (double)(j.offsets[b + 1] - j.offsets[b]), rb = (double)j.rows_of(b);
        pre[(size_t)b + 1] = pre[(size_t)b] + nb * rb + nb + rb;
    }
    std::vector<int64_t> share((size_t)n_devices + 1, n_curves);
    share[0] = 0;
    for (int i = 1; i < n_devices; ++i)
        share[(size_t)i] = std::lower_bound(pre.begin(), pre.end(), pre.back() * i / n_devices) - pre.begin();
    // each slot's groups: the largest group shrinks by powers of two (WorkScale) until it fits the slot's budget,
    // PDC_WORK_BUDGET_GB and its share of what the device has free (plus what the slots on it already hold)
    std::vector<std::vector<int64_t>> cuts((size_t)n_devices);
    for (int i = 0; i < n_devices; ++i) {
        RaggedSlot &s = r.slots[(size_t)i];
        PDC_TRY(use_device(s.device));
        if (!s.stream) PDC_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        const int64_t c0 = share[(size_t)i], c1 = share[(size_t)i + 1];
        if (c1 <= c0) continue;
        int same = 0;
        int64_t held = 0;
        for (const RaggedSlot &o : r.slots)
            if (o.device == s.device) {
                ++same;
                held += o.cap;
            }
        int64_t budget = work_budget();
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const int64_t avail = (int64_t)((double)((int64_t)free_b + held) * 0.9 / same);
            if (avail > 0 && (budget == 0 || avail < budget)) budget = avail;
        } else {
            (void)hipGetLastError();
        }
        const int64_t whole = j.group_bytes(c0, c1, row_max_of(j, c0, c1));
        WorkScale ws(budget, [&] {
            int64_t largest;
            (void)make_groups(j, c0, c1, (int64_t)((double)whole * work_scale()), &largest);
            return largest;
        });
        PDC_REQUIRE_FITS(ws, what);
        int64_t largest;
        cuts[(size_t)i] = make_groups(j, c0, c1, (int64_t)((double)whole * work_scale()), &largest);
    }
    r.groups = 0;
    for (const std::vector<int64_t> &cut : cuts) r.groups += cut.empty() ? 0 : (int64_t)cut.size() - 1;
    std::vector<int> rc((size_t)n_devices, PDC_OK);
    std::vector<std::string> why((size_t)n_devices);
    auto run_slot = [&](int i) {
        RaggedSlot &s = r.slots[(size_t)i];
        const std::vector<int64_t> &cut = cuts[(size_t)i];
        int e = use_device(s.device);
        for (size_t q = 0; e == PDC_OK && q + 1 < cut.size(); ++q) e = run_group(s, j, cut[q], cut[q + 1]);
        if (e != PDC_OK) {
            rc[(size_t)i] = e;
            why[(size_t)i] = pdc_last_error();
            (void)hipStreamSynchronize(s.stream);
        }
    };
    if (n_devices == 1) {
        run_slot(0);
    } else {
        std::vector<std::thread> th;
        for (int i = 0; i < n_devices; ++i) th.emplace_back(run_slot, i);
        for (std::thread &x : th) x.join();
    }
    for (int i = 0; i < n_devices; ++i)
        if (rc[(size_t)i] != PDC_OK) {
            set_error("%s", why[(size_t)i].c_str());
            return rc[(size_t)i];
        }
    if (j.negate_heights && j.k > 0 && j.height)   // the table ranked -statistic: heights back to the statistic itself
        for (int64_t i = 0; i < n_curves * j.k; ++i) j.height[i] = -j.height[i];
    return PDC_OK;
}

}  // namespace pdc
