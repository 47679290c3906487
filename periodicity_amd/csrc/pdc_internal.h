// Internal helpers shared by the translation units of libperiodicity_hip.so (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/periodicity_hip.h"

namespace pdc {

// Per-thread message returned by pdc_last_error().
void set_error(const char *fmt, ...);

// Grow-only device scratch cached per (device, slot); released by pdc_release().
// Slots keep the buffers of one host-level call apart.
enum Slot { SLOT_IN0 = 0, SLOT_IN1, SLOT_IN2, SLOT_IN3, SLOT_OUT0, SLOT_OUT1, SLOT_OUT2, SLOT_WORK,
            SLOT_COUNT };
int cached(int device, Slot slot, int64_t bytes, void **dptr);

// Frees the multi-GPU plans the one-shot `_multi` entry points cache (multi.hip).
void release_multi();
// Frees the per-slot buffers and streams the ragged-grid GLS host entries keep between calls (gls_ragged.hip).
int release_ragged();
// ... and those of the ragged-grid PDM / AoV / conditional-entropy host entries (pdm_ragged.hip).
int release_phase_ragged();
// ... and those of the ragged-grid StringLength host entries (sl_ragged.inc, in stringlength.hip).
int release_sl_ragged();
// ... and those of the ragged-grid BLS host entries (bls_ragged.hip).
int release_bls_ragged();

// ---- ragged-grid batches: the host side the kinds share (ragged.hip) ---------------------------------------------
// A ragged batch is a catalogue of light curves that each keep their own grid: curve b owns samples
// [offsets[b], offsets[b+1]) and rows [rows[b], rows[b+1]) - GLS's frequency bins (gls_ragged.hip) or the phase
// folds' trial periods (pdm_ragged.hip, sl_ragged.inc, bls_ragged.hip).  Each kind keeps its kernels, its workspace
// layout and its launches; the frame around them - slots, groups, a group's uploads and copies back, the metadata
// upload, the peak-table arguments, the pitch check - is here, once.
inline int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct Carve {   // byte offsets of the parts of a buffer, in order: each part starts on a multiple of 256
    int64_t at = 0;
    int64_t take(int64_t bytes) {   // the part's offset; the next one starts up256(bytes) later
        const int64_t here = at;
        at += up256(bytes);
        return here;
    }
};

// The checks every ragged entry shares, with their texts: n_curves, offsets and `rows_name` starting at 0 and never
// decreasing, fewer than 2^31 tiles of `tile` rows (`too_large` ends that message); curve(b) adds the kind's own.
int ragged_validate(const char *what, const int64_t *offsets, const int64_t *rows, const char *rows_name,
                    int64_t n_curves, int64_t tile, const char *too_large, const std::function<int(int64_t)> &curve);

// A `_dev` entry's pitched copy: no curve has more rows (`unit`: "bins" or "periods") than the pitch.
int ragged_check_pitch(const char *what, const int64_t *rows, int64_t n_curves, int64_t pitch, const char *unit);

// Dispatch order of a ragged scan: order[0, m) = the curves with at least one row, most samples first (ties in curve
// order), otile[0, m] = their prefix of tiles of `tile` rows; returns m.
int64_t ragged_order(const int64_t *offsets, const int64_t *rows, int64_t n_curves, int64_t tile, int64_t *order,
                     int64_t *otile);

// Bytes of a group's peak table, the tail of its buffer (0 for k == 0): the pitched [B][pitch] copy of the rows, whose
// pad [rows_b, pitch) is NaN, then count [B] | idx | half_lo | half_hi | height | prominence [B][k].
int64_t ragged_table_bytes(int64_t n_curves, int64_t pitch, int k);

struct RaggedSlot {   // one device slot: its stream, its grow-only buffer, the host copy of a group's metadata
    int device = 0;
    hipStream_t stream = nullptr;
    void *buf = nullptr;
    int64_t cap = 0;
    std::vector<int64_t> meta;   // (uploaded asynchronously: lives until the stream is synchronised)
};

struct RaggedSlots {   // one kind's slots, kept between host calls for the same device list
    std::mutex mutex;
    std::vector<int> devices;
    std::vector<RaggedSlot> slots;
    int64_t groups = 0;   // groups the last call ran, over all slots
    int release();        // frees every slot's stream and buffer (pdc_release())
};

// One host call of a kind: where its peak table goes (caller's host arrays, any may be NULL) and its two group hooks.
struct RaggedBatch {
    const int64_t *offsets = nullptr, *rows = nullptr;   // [B + 1]
    int k = 0, by_prominence = 0;                        // k > 0: a [B][k] peak table of the rows (pdc_peaks_topk_dev)
    int64_t *count = nullptr, *idx = nullptr, *lo = nullptr, *hi = nullptr;
    double *height = nullptr, *prom = nullptr;
    bool negate_heights = false;   // the pitched copy holds -statistic (dips): ragged_run turns `height` back
    int64_t rows_of(int64_t b) const { return rows[b + 1] - rows[b]; }
    // The table arguments of a `*_ragged_peaks` entry, in the ABI's order, after the kind's validate: k in 1 .. 1024,
    // at least one output (`other_output`: the entry has one besides the table), then the fields above.
    int want_table(const char *what, int k, int by_prominence, int64_t *count_out, int64_t *idx_out, double *height_out,
                   double *prominence_out, int64_t *half_lo_out, int64_t *half_hi_out, bool other_output);
    // Slot-buffer bytes of the group [c0, c1) whose longest grid has row_max rows (0 without a table); the buffer
    // ends with the ragged_table_bytes(c1 - c0, row_max, k) of the peak table.
    virtual int64_t group_bytes(int64_t c0, int64_t c1, int64_t row_max) const = 0;
    // Enqueues the group on s.stream: uploads, launches (rows also into `pitched` when not NULL), copies of the kind's
    // own outputs to the host.  ragged_run ranks the table and synchronises.
    virtual int run_group(RaggedSlot &s, int64_t c0, int64_t c1, int64_t row_max, double *pitched) const = 0;
};

// The group [c0, c1) of a batch on its slot, as a run_group sees it: B curves, n samples from s0, nr rows from r0, the
// batch's offsets and rows rebased to the group (what a kind's `*_dev` function takes), and the copies between the
// caller's host arrays and byte offsets of the slot buffer, enqueued on the slot's stream.
struct RaggedGroup {
    RaggedGroup(const RaggedBatch &batch, const RaggedSlot &slot, int64_t c0, int64_t c1);
    int64_t B, c0, s0, n, r0, nr;
    std::vector<int64_t> off, roff;   // [B + 1]
    char *buf;
    hipStream_t st;
    template <typename T>
    T *at(int64_t byte) const { return reinterpret_cast<T *>(buf + byte); }
    template <typename T>
    T *at_if(const void *wanted, int64_t byte) const { return wanted ? at<T>(byte) : nullptr; }
    int upload(int64_t byte, const double *host) const;   // the group's n samples of a [n_total] array (NULL: none)
    template <typename T>
    int rows_back(T *host, int64_t byte) const { return back(host ? host + r0 : nullptr, byte, nr * (int64_t)sizeof(T)); }
    template <typename T>
    int curves_back(T *host, int64_t byte) const { return back(host ? host + c0 : nullptr, byte, B * (int64_t)sizeof(T)); }
    int back(void *host, int64_t byte, int64_t bytes) const;   // (NULL or nothing to copy: no call)
};

// A group's metadata: `arrays` columns of B + 1 entries each, int64 or double, filled in the slot's host vector,
// uploaded in one copy to `d_meta`; the same object gives the columns' device addresses for the kernel arguments.
struct RaggedMeta {
    RaggedMeta(std::vector<int64_t> &host, int arrays, int64_t n_curves, void *d_meta);   // (all zeros)
    std::vector<int64_t> &host;
    int64_t B1, *dev;
    int64_t *i64(int column) { return host.data() + column * B1; }
    double *f64(int column) { return reinterpret_cast<double *>(i64(column)); }
    const int64_t *d_i64(int column) const { return dev + column * B1; }
    const double *d_f64(int column) const { return reinterpret_cast<const double *>(d_i64(column)); }
    void fill_offsets(const int64_t *offsets, const int64_t *rows);   // columns 0 and 1, [B + 1]
    // columns column .. column + 2 [B]: the linspace description of every curve's grid
    void fill_linspace(int column, const double *start, const double *step, const double *stop);
    int upload(hipStream_t st, bool wait);   // wait: the host vector goes when the caller returns
};

// A host call: curves dealt to device slots in contiguous shares balanced by sum n_b rows_b + n_b + rows_b (a device
// may repeat), each share cut into contiguous groups that fit the slot's budget, one thread per slot; a slot's error
// is the call's.  With batch.negate_heights the table's heights change sign once every group has run.
int ragged_run(const char *what, RaggedSlots &slots, const RaggedBatch &batch, int64_t n_curves, const int *devices,
               int n_devices);

// Every device / pinned-host allocation of the library goes through these two, so that
// pdc_alloc_counts() can show a caller (and the tests) that a cached path allocates nothing on
// its second call.
int device_alloc(void **dptr, int64_t bytes);
int pinned_alloc(void **hptr, int64_t bytes);

// Grow-only device scratch cached per (device, stream) for the `_dev` entry points that need a
// workspace the ABI does not pass in: work enqueued on one stream is ordered, so reuse is safe, and two
// streams never share a buffer.  (Stream-ordered pool memory - hipMallocAsync - is NOT used: on ROCm 7.2 a
// block handed out again by the pool gave kernels of the next call stale partial results unless the block
// was memset first)  Released by pdc_release(); the entry of a stream handed to
// pdc_stream_destroy() goes with it, and a device's entries are capped (kScratchPerDevice, true LRU) so that
// a caller cycling through raw HIP streams cannot grow the table without bound - but only entries that are
// not pinned and whose stream has run dry are ever evicted.  stream_scratch() returns the block PINNED; the
// caller unpins it (stream_scratch_done, or the ScratchPin guard) once all launches that use it are enqueued:
// from then on the stream itself is busy until they have run.  Entry points that take an
// explicit workspace (pdc_phase_scan_dev, pdc_gls_scan_dev, pdc_stringlength_scan_dev) never come here.
// RULE: no nested pin on one (device, stream) - a caller that takes stream_scratch() twice before stream_scratch_done()
// waits for itself.  Every `_dev` entry takes the block once, enqueues, unpins (ScratchPin::take).
int host_stream(int device, hipStream_t *st);   // the device's stream for host entry points (caller holds DeviceLock); destroyed by pdc_release()
int stream_scratch(int device, hipStream_t stream, int64_t bytes, void **dptr);
void stream_scratch_done(int device, hipStream_t stream);
int drop_stream_scratch(int device, hipStream_t stream);
struct ScratchPin {   // unpins on scope exit (also on the error returns of PDC_TRY / PDC_HIP)
    int device = -1;
    hipStream_t stream = nullptr;
    bool held = false;
    ScratchPin() = default;
    ScratchPin(const ScratchPin &) = delete;
    int take(int device_, hipStream_t stream_, int64_t bytes, void **dptr) {   // stream_scratch(), and the pin is this guard's
        const int status = stream_scratch(device_, stream_, bytes, dptr);
        device = device_;
        stream = stream_;
        held = status == PDC_OK;
        return status;
    }
    ~ScratchPin() {
        if (held) stream_scratch_done(device, stream);
    }
};

// The phase-fold statistics with an explicit workspace (pdm.hip): kind 0 = PDM theta, 1 = AoV,
// 2 = conditional entropy.  work == NULL falls back to stream_scratch().
int64_t phase_stat_work_bytes(int kind, int64_t n, int64_t n_periods, int nb, int nc);
int phase_stat_dev(int kind, int device, hipStream_t st, const double *d_t, const double *d_x, int64_t n,
                   const double *d_periods, int64_t n_periods, int nb, int nc, double sigma, double *d_out,
                   void *work, int64_t work_bytes);

// StringLength (kind 3) / Supersmoother (kind 5) for callers that hold the host arrays too (stringlength.hip): whether
// the streamed kernels will need their bin lists (hints bit 0) and whether t is in order (bit 1: no time sort to
// launch), the workspace for those hints, the scan.  hints = 1 is what a caller that has not looked passes.
int sorted_scan_hints(int kind, const double *t, int64_t n, const double *periods, int64_t n_periods);
int64_t sorted_scan_work_bytes(int kind, int64_t n, int64_t n_periods, int hints);
int sorted_scan_dev(int kind, int device, void *stream, const double *d_t, const double *d_v, int64_t n, const double *d_periods,
                    int64_t n_periods, double alpha, double *d_out, void *work, int64_t work_bytes, int hints);

// ---- workspace budget (round 6) -------------------------------------------------------------------------------
// The StringLength / Supersmoother workspaces are sized by built-in caps (12 GB of bin lists, 2 GB of sorted curves,
// 1 GB pools, 1024 workgroups' scratch ...) chosen for a 288 GB device that the caller owns.  On a shared device, or
// with eight loopback slots on one GPU, those caps are what made hipMalloc fail.  A budget - PDC_WORK_BUDGET_GB for
// every entry point, and for the HOST entry points also 0.9 x (free device memory + the cached workspace they would
// replace) from hipMemGetInfo - scales ALL of those caps by the largest power of two <= 1 for which the workspace
// fits: smaller batches, fewer resident workgroups, same results.  The scale is a thread-local set for the duration
// of one entry point (WorkScale; an inner entry keeps the outer one's), and every size function reads it, so
// `pdc_*_work_bytes` and the launch that follows agree as long as PDC_WORK_BUDGET_GB does not change in between.
int64_t work_budget();                          // PDC_WORK_BUDGET_GB in bytes (0: none)
int64_t host_work_budget(int device);           // min(work_budget(), 0.9 x (free + cached SLOT_WORK)) - caller holds the DeviceLock
double work_scale();                            // 1 outside a WorkScale scope
double *work_scale_slot(int **depth);           // (the thread-local pair behind WorkScale)
struct WorkScale {
    int64_t budget, need;
    template <typename Total>
    WorkScale(int64_t budget_, Total total) : budget(budget_), need(0) {
        int *depth;
        double *scale = work_scale_slot(&depth);
        if ((*depth)++ == 0) {
            *scale = 1.0;
            if (budget > 0)
                while (total() > budget && *scale > 1.0 / 65536.0) *scale *= 0.5;
        }
        need = total();
    }
    ~WorkScale() {
        int *depth;
        double *scale = work_scale_slot(&depth);
        if (--(*depth) == 0) *scale = 1.0;
    }
    bool fits() const { return budget <= 0 || need <= budget; }
};
#define PDC_REQUIRE_FITS(ws, what)                                                                                      \
    PDC_REQUIRE((ws).fits(), "%s: even the smallest batch needs %lld bytes of workspace, over the budget of %.3f GB "     \
                             "(PDC_WORK_BUDGET_GB / free device memory)", what, (long long)(ws).need, (double)(ws).budget / (double)(1 << 30))

// hipSetDevice + range check; every entry point starts here.
int use_device(int device);

// Compute units of a device (cached per device; 256 where the runtime does not say).
int cu_count(int device);

// Raises a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) on the CURRENT device,
// once per (device, kernel): the attribute belongs to the device's copy of the kernel, so a process that
// drives several GPUs has to set it on each of them.
int allow_dynamic_lds(const void *kernel, int bytes);

// GLS.bootstrap through the FFT path with the replicates given by index (glsfft.hip; host buffers, one device).
int gls_bootstrap_fft(const double *t, const double *y, const double *dy, int64_t n, const int32_t *picks,
                      int64_t n_boot, double fmin, double df, int64_t nf, int fit_mean, int psd,
                      double *amax_out, int64_t *argmax_out, int device);

// Serialises the host-level entry points that share the cached workspace of one device.
struct DeviceLock {
    explicit DeviceLock(int device);
    ~DeviceLock();
    int device;
};

// ---- single-call host entries: the frame they share (runtime.hip) -------------------------------------------------
// A host entry (numpy in, numpy out) checks its arguments, then opens a HostCall: use_device (it builds the device
// table), the DeviceLock, the device's host stream, in that order.  Inputs go up through in(), outputs and SLOT_WORK are
// reserved, the entry enqueues its own `_dev` call or launches on stream(), outputs come back through back(), finish()
// waits.  Slots, sizes, checks and launches stay the entry's; nothing here knows a kind.
// The status is STICKY: after the first failure (of the opening, a cached() block, a copy) every later call does
// nothing and returns NULL, and the error text stays the first one's - so an entry checks `status` once, before it
// enqueues.  An entry that returns before finish() with work enqueued (a late PDC_REQUIRE in a `_dev` call, a failed
// launch) leaves copies from and into the caller's arrays in the stream: the destructor waits for them, status
// ignored, before the lock goes.
struct HostCall {
    explicit HostCall(int device);
    ~HostCall();
    HostCall(const HostCall &) = delete;
    int status;
    const int device;
    hipStream_t stream() {   // for the entry's own enqueues: from here on the destructor has something to wait for
        busy = true;
        return st;
    }
    void *reserve(Slot slot, int64_t bytes);                  // the slot's cached() block, nothing copied
    void put(void *dev, const void *host, int64_t bytes);     // H2D into a reserved block (NULL host: no call)
    void back(void *host, const void *dev, int64_t bytes);    // D2H (NULL host: no call)
    int finish();                                             // the one hipStreamSynchronize; the call's status
    template <typename T>
    T *out(Slot slot, int64_t bytes) { return static_cast<T *>(reserve(slot, bytes)); }
    template <typename T>
    T *in(Slot slot, const T *host, int64_t bytes) {          // block + H2D copy (NULL host: NULL, no call)
        T *dev = host ? out<T>(slot, bytes) : nullptr;
        put(dev, host, bytes);
        return dev;
    }

private:
    DeviceLock lock;   // (taken after use_device, released after the destructor's wait)
    hipStream_t st = nullptr;
    bool busy = false;
};

// The inputs every GLS batch entry takes: check() before any device - offsets never decrease, under shared_t every curve
// is as long as the first, offsets[0] == 0, each with `what` in front, in that order - and it fills the sizes; upload()
// on the open call: t [n_t] in SLOT_IN0, y and dy (NULL: none) in SLOT_IN1 / SLOT_IN2 - n_total values, or the one
// curve's n_t that a bootstrap resamples by index (one_curve) -, offsets [n_curves + 1] in SLOT_IN3.
struct GlsBatchIn {
    int64_t n_total = 0, n_t = 0, n_max = 0;   // samples of y, of t (one curve's when shared), of the longest curve
    double *d_t = nullptr, *d_y = nullptr, *d_dy = nullptr;
    int64_t *d_off = nullptr;
    int check(const char *what, const int64_t *offsets, int64_t n_curves, int shared_t);
    void upload(HostCall &hc, const double *t, const double *y, const double *dy, const int64_t *offsets, int64_t n_curves,
                bool one_curve = false) {
        const int64_t n_y = one_curve ? n_t : n_total;
        d_t = hc.in(SLOT_IN0, t, n_t * 8);
        d_y = hc.in(SLOT_IN1, y, n_y * 8);
        d_dy = hc.in(SLOT_IN2, dy, n_y * 8);
        d_off = hc.in(SLOT_IN3, offsets, (n_curves + 1) * 8);
    }
};

}  // namespace pdc

#define PDC_HIP(call)                                                                     \
    do {                                                                                  \
        hipError_t _e = (call);                                                           \
        if (_e != hipSuccess) {                                                           \
            pdc::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, \
                           __LINE__);                                                     \
            return _e == hipErrorOutOfMemory ? PDC_ERR_NOMEM : PDC_ERR_HIP;               \
        }                                                                                 \
    } while (0)

#define PDC_TRY(call)          \
    do {                       \
        int _s = (call);       \
        if (_s != PDC_OK) return _s; \
    } while (0)

#define PDC_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            pdc::set_error(__VA_ARGS__); \
            return PDC_ERR_INVALID;     \
        }                               \
    } while (0)

inline int pdc::GlsBatchIn::check(const char *what, const int64_t *offsets, int64_t n_curves, int shared_t) {
    for (int64_t b = 0; b < n_curves; ++b) {
        const int64_t nb = offsets[b + 1] - offsets[b];
        PDC_REQUIRE(nb >= 0, "%s: offsets must be non-decreasing", what);
        PDC_REQUIRE(!shared_t || nb == offsets[1] - offsets[0],
                    "%s: with a shared time axis every curve must have the same length", what);
        n_max = nb > n_max ? nb : n_max;
    }
    PDC_REQUIRE(offsets[0] == 0, "%s: offsets[0] must be 0", what);
    n_total = offsets[n_curves];
    n_t = shared_t ? offsets[1] : n_total;
    return PDC_OK;
}

#include "pdc_device.h"
