/*
 * periodicity_hip.h — C ABI of libperiodicity_hip.so: MI355X (gfx950) trial-frequency scans.
 *
 * The reference (dioph/periodicity) is pure Python and has no FFI of its own; the boundary a
 * native replacement slots into is its callable API plus three private seams.
 * Each entry point below names the reference interface it replaces
 * (paths relative to /root/reference/src/periodicity/).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - fp64 only; every array is C-contiguous; sizes are int64_t.
 *   - Functions return 0 on success, a negative pdc_status otherwise; the message of the last
 *     failure on the calling thread is available from pdc_last_error().
 *   - "host" entry points take host pointers: the caller owns every buffer, the library copies
 *     H2D/D2H itself, keeps no host pointer after return and caches its device workspace per
 *     device (freed by pdc_release()).
 *   - "_dev" entry points take device pointers on `device` and enqueue on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream).  They do not synchronise.
 *   - NaN/Inf in the data are not errors: IEEE results propagate exactly as in numpy
 *     (spectral.py:113-128 has no guards).
 *   - No C++ exception crosses this boundary.
 */
#ifndef PERIODICITY_HIP_H
#define PERIODICITY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pdc_status {
    PDC_OK = 0,
    PDC_ERR_INVALID = -1,   /* bad argument (NULL, negative size, incompatible lengths) -> ValueError */
    PDC_ERR_NODEVICE = -2,  /* no usable gfx950 device                                 -> RuntimeError */
    PDC_ERR_HIP = -3,       /* a HIP runtime call failed                               -> RuntimeError */
    PDC_ERR_RCCL = -4,      /* an RCCL call failed                                     -> RuntimeError */
    PDC_ERR_NOMEM = -5      /* device or host allocation failed                        -> MemoryError  */
} pdc_status;

/* ---- runtime ------------------------------------------------------------------------------- */
const char *pdc_last_error(void);
int pdc_version(void);                                   /* 100*major + minor */
int pdc_device_count(int *count);
int pdc_device_info(int device, char *name, int name_len, int *cu_count, int64_t *hbm_bytes,
                    int *clock_khz);
int pdc_release(void);                                   /* free all cached device workspaces */
/* How many device (hipMalloc) and page-locked host (hipHostMalloc) allocations the library has made in
 * this process so far: a cached path (plans, the one-shot `_multi` entry points, the per-device
 * workspaces) shows no increase on its second call with the same sizes. */
int pdc_alloc_counts(int64_t *device_allocs, int64_t *pinned_allocs);
/* TEST HOOKS (not for callers): pin / unpin the scratch block the library keeps per (device, stream) for the `_dev`
 * entry points that take no workspace.  Rule they let the tests drive: ONE holder at a time per (device, stream) -
 * a second pdc_test_scratch_pin on the same stream WAITS until the first is unpinned (so never pin twice from one
 * thread without unpinning: it would wait for itself). */
int pdc_test_scratch_pin(int device, void *stream, int64_t bytes, void **dptr);
int pdc_test_scratch_unpin(int device, void *stream);

/* device memory + events for callers that keep data resident (bench.py, tests) */
int pdc_malloc(int device, int64_t bytes, void **dptr);
int pdc_free(int device, void *dptr);
int pdc_memcpy_h2d(int device, void *dst, const void *src, int64_t bytes);
int pdc_memcpy_d2h(int device, void *dst, const void *src, int64_t bytes);
int pdc_memset(int device, void *dst, int value, int64_t bytes);
int pdc_stream_create(int device, void **stream);
int pdc_stream_destroy(int device, void *stream);
int pdc_stream_sync(int device, void *stream);
int pdc_device_sync(int device);
int pdc_event_create(int device, void **event);
int pdc_event_destroy(int device, void *event);
int pdc_event_record(int device, void *event, void *stream);
int pdc_event_elapsed_ms(int device, void *start, void *stop, float *ms);  /* syncs on stop */
/* Measurement aid (no counterpart upstream): a fixed count of fp64 fmas, 16 independent chains per lane, 4 waves on
 * every SIMD of the device, timed with HIP events on `stream`.  *wave_instr_per_simd x 4 cycles / *ms = the clock the
 * chip sustains under fp64 load right now (it is power-limited there), the figure bench.py prints beside the
 * headline so that a box-to-box difference of the same kernel can be attributed; *memtime_ratio = s_memtime ticks
 * per s_memrealtime tick (100 MHz) over one wave's loop.  iters ~ 10 000 runs about 10 ms. */
int pdc_clock_probe(int device, void *stream, int iters, float *ms, double *wave_instr_per_simd, double *memtime_ratio);

/* ---- generalized Lomb-Scargle --------------------------------------------------------------
 * Replaces GLS.__call__ from the weights onward (spectral.py:99-132): w = dy^-2 / sum(dy^-2)
 * (dy == NULL -> ones, :99-103), y centred by the weighted mean when fit_mean (:105-108), the
 * three _trig_sum calls (:109-112) evaluated as exact direct sums, and the fused epilogue
 * (:113-132).  The grid is the one np.arange(fmin, fmax + df, df) produced on the host (:97):
 * frequency[j] = f0 + j*delta with f0 = frequency[0], delta = frequency[1] - frequency[0]
 * (numpy's own fill rule), j = j_begin .. j_begin + nf - 1; power_out[0..nf) receives that slab.
 */
int pdc_gls_scan(const double *t, const double *y, const double *dy, int64_t n,
                 double f0, double delta, int64_t j_begin, int64_t nf,
                 int fit_mean, int psd, double *power_out, int device);

/* Batch of independent light curves on one shared grid (the shape of GLS.bootstrap,
 * spectral.py:140-152, when shared_t != 0: one time axis, B resampled (y, dy) rows).
 * Curve b occupies [offsets[b], offsets[b+1]) of y/dy (and of t unless shared_t, in which case
 * t has offsets[1]-offsets[0] entries and every curve must have that length).
 * power_out is [B][nf] or NULL; amax_out / argmax_out are [B] or NULL and receive the NaN-aware
 * maximum and its index (Signal.amax / argmax, core.py:202-215), computed on the device. */
int pdc_gls_scan_batch(const double *t, const double *y, const double *dy,
                       const int64_t *offsets, int64_t n_curves, int shared_t,
                       double f0, double delta, int64_t j_begin, int64_t nf,
                       int fit_mean, int psd,
                       double *power_out, double *amax_out, int64_t *argmax_out, int device);

/* A batch of curves dealt to `n_devices` GPU slots in contiguous groups of ceil(n_curves / n_devices)
 * curves (batches shard over curves, no exchange); arguments and outputs as
 * pdc_gls_scan_batch.  With shared_t != 0 this is GLS.bootstrap (spectral.py:140-152) over several GPUs.
 * A device may be listed more than once; per-slot buffers are kept between calls. */
int pdc_gls_scan_batch_multi(const double *t, const double *y, const double *dy,
                             const int64_t *offsets, int64_t n_curves, int shared_t,
                             double f0, double delta, int64_t nf, int fit_mean, int psd,
                             double *power_out, double *amax_out, int64_t *argmax_out,
                             const int *devices, int n_devices);

/* One periodogram with the grid split into contiguous equal slabs over `n_devices` GPUs of this
 * node (one process, one stream per device), gathered with one RCCL all-gather over xGMI. */
int pdc_gls_scan_multi(const double *t, const double *y, const double *dy, int64_t n,
                       double f0, double delta, int64_t nf, int fit_mean, int psd,
                       double *power_out, const int *devices, int n_devices);

/* GLS.bootstrap (spectral.py:140-152) with the replicates given BY INDEX.  Upstream draws
 * `bs = rng.integers(0, ndata, ndata)` per replicate (:146) and runs a full periodogram of
 * (values[bs], err[bs]) on the unchanged time axis, keeping only `.amax()` (:147-150).  Here the caller
 * draws the same integers and passes them as picks[n_boot][n] (int32, row b = replicate b); only the ONE
 * curve (t, y, dy|NULL) and the indices are uploaded, the device prologue gathers y[picks], dy[picks]
 * while it builds the weight table of the shared-time-axis kernel.  Outputs: the NaN-aware maximum of
 * every replicate's spectrum (amax_out[n_boot]) and/or its bin (argmax_out[n_boot]).
 * method 0: exact direct sums on the grid f0 + j*delta; method 1: the reference's FFT/extirpolation
 * path with fmin = f0, df = delta (first listed device only).  Replicates are dealt to the listed device
 * slots in contiguous groups, no exchange.  Any pick outside 0 .. n-1 is PDC_ERR_INVALID. */
int pdc_gls_bootstrap(const double *t, const double *y, const double *dy, int64_t n, const int32_t *picks,
                      int64_t n_boot, double f0, double delta, int64_t nf, int fit_mean, int psd, int method,
                      double *amax_out, int64_t *argmax_out, const int *devices, int n_devices);
/* Device-resident form: inputs, picks and outputs in HBM, no synchronisation; `work` of at least
 * pdc_gls_bootstrap_work_bytes(n, n_boot, nf) bytes on the same device. */
int64_t pdc_gls_bootstrap_work_bytes(int64_t n, int64_t n_boot, int64_t nf);
int pdc_gls_bootstrap_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy,
                          int64_t n, const int32_t *d_picks, int64_t n_boot, double f0, double delta, int64_t nf,
                          int fit_mean, int psd, double *d_amax, int64_t *d_argmax, void *work,
                          int64_t work_bytes);

/* The same shard + all-gather as a persistent plan for callers that scan repeatedly (bench.py, a
 * survey loop over many light curves): per-device sample/power/work buffers, two streams and the
 * events per device and the RCCL communicators (ncclCommInitAll, one process, N devices) are created
 * ONCE by pdc_gls_plan_create and reused by every scan; this is also what pdc_gls_scan_multi keeps
 * cached between calls.  Replaces the per-call process fan-out of phase.py:69-70,185-186 for the
 * spectral path.  `devices` are distinct ordinals below pdc_device_count() (else PDC_ERR_INVALID).
 *   upload   replicate (t, y, dy|NULL) of n <= n_max samples on every device (async, compute streams)
 *   scan     enqueue: device i scans slab i of the nf <= nf_max grid into generation g of its power
 *            buffer, then the grouped ncclAllGather of generation g runs on the communication streams
 *            while the next scan (generation g^1) may already compute; returns without waiting
 *   wait     drain every stream of the plan
 *   download wait, then copy the latest complete power[nf] from device slot `which` (every device
 *            holds the whole array after the gather)
 *   kernel_ms  HIP-event time of the latest slab scan on devices[0]
 *   slot_ms    the same for every slot (ms_out[n_slots]; the slowest slot bounds a sharded scan) */
int pdc_gls_plan_create(const int *devices, int n_devices, int64_t n_max, int64_t nf_max, void **plan);
/* The same plan with `n_slots` LOGICAL slots on ONE physical device ("loopback"): every slot has its own
 * buffers, streams and events, scans its own slab, and the all-gather is replaced by the equivalent
 * device-to-device copies on the communication streams (RCCL refuses two ranks on one device).  The slab
 * arithmetic, padded tails (nf % n_slots != 0, nf < n_slots), generation reuse and event ordering are
 * those of the N-GPU plan, so they can be tested on a 1-GPU box.  PDC_PLAN_EXCHANGE=copy makes
 * pdc_gls_plan_create use the copy exchange between distinct devices too (hipMemcpyPeerAsync). */
int pdc_gls_plan_create_loopback(int device, int n_slots, int64_t n_max, int64_t nf_max, void **plan);
/* n_slots; the size RCCL reports for the plan's communicator (ncclCommCount; 0 = no communicator);
 * exchange: 0 none (one slot), 1 RCCL all-gather, 2 device-to-device copies.  Any pointer may be NULL. */
int pdc_gls_plan_info(void *plan, int *n_slots, int *rccl_ranks, int *exchange);
/* If ncclCommInitAll failed when the plan was built, the plan does NOT fail: it warns on stderr and exchanges the
 * slabs by device-to-device copies (peer access enabled where the devices allow it) - exchange == 2 above - and the
 * reason is kept here (empty string: the communicators were built, or never needed).  PDC_FORCE_RCCL_FAIL=1 injects
 * the failure (tests, `bench.py --loopback`). */
int pdc_gls_plan_init_error(void *plan, char *buf, int buf_len);
int pdc_gls_plan_upload(void *plan, const double *t, const double *y, const double *dy, int64_t n);
int pdc_gls_plan_scan(void *plan, double f0, double delta, int64_t nf, int fit_mean, int psd);
int pdc_gls_plan_wait(void *plan);
int pdc_gls_plan_download(void *plan, double *power_out, int64_t nf, int which);
int pdc_gls_plan_kernel_ms(void *plan, float *ms);
int pdc_gls_plan_slot_ms(void *plan, float *ms_out, int n_slots);
int pdc_gls_plan_destroy(void *plan);

/* Seam-level: replaces _trig_sum(t, w, df, nf, fmin) (spectral.py:11-40) by what its docstring
 * defines (:13-15): S_j = sum_i w_i sin(2 pi f_j t_i), C_j = sum_i w_i cos(2 pi f_j t_i),
 * f_j = f0 + j*delta. */
int pdc_trig_sums(const double *t, const double *w, int64_t n,
                  double f0, double delta, int64_t nf,
                  double *S_out, double *C_out, int device);

/* ---- BGLST: Bayesian generalised Lomb-Scargle with linear trend -----------------------------------------------
 * The reference exports the name (spectral.py:7 `__all__ = ["GLS", "BGLST"]`) for an empty class (:207-208, README:
 * "Bayesian Lomb-Scargle with linear Trend (soon)"); there is nothing upstream to replace or to pin against -
 * PARITY UNPINNED BY THE REFERENCE.  What is computed is the published statistic (Olspert, Pelt, Kapyla & Lehtinen
 * 2018, A&A 615, A111): per trial frequency f_j = f0 + (j_begin + j) delta the log marginal likelihood of
 *     y_i = A cos(2 pi f t_i) + B sin(2 pi f t_i) + alpha tau_i + beta + eps_i,   eps_i ~ N(0, dy_i^2),
 * with independent zero-mean Gaussian priors on A, B (one sigma_A), alpha, beta integrated out analytically;
 * tau = (t - t_ref) / span.  Same kernel skeleton as pdc_gls_scan (eight running sums per pair instead of six).
 * scalars[12] = {W = sum dy^-2, then over the normalised weights w = dy^-2 / W: sum w y^2, sum w y, sum w tau y,
 * sum w tau^2, sum w tau; (t[0] - t_ref) / span; 1 / span; 1 / sigma_A^2, 1 / sigma_alpha^2 (alpha per span),
 * 1 / sigma_beta^2; sum log(2 pi dy_i^2) + log(sigma_A^4 sigma_alpha^2 sigma_beta^2)} - O(N) host work in fp64
 * (periodicity_amd/spectral.py:BGLST).  dy == NULL: unit uncertainties.  Workspace: pdc_gls_work_bytes(n, 1, nf). */
int pdc_bglst_scan(const double *t, const double *y, const double *dy, int64_t n,
                   double f0, double delta, int64_t j_begin, int64_t nf, const double *scalars,
                   double *loglik_out, int device);
int pdc_bglst_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                       double f0, double delta, int64_t j_begin, int64_t nf, const double *scalars,
                       double *d_loglik, void *work, int64_t work_bytes);

/* ---- multi-harmonic generalised Lomb-Scargle (Schwarzenberg-Czerny 1996, ApJ 460, L107; Palmer 2009, ApJ 695, 496) -----
 * The reference has no such class - PARITY UNPINNED BY THE REFERENCE.  Per trial frequency f_j = f0 + (j_begin + j) delta
 * the weighted least-squares fit of a Fourier series of `nterms` (1 .. 4) harmonics, theta_i = 2 pi f (t_i - t_0):
 * design columns cos(h theta), sin(h theta), h = 1 .. nterms, and a constant when fit_mean; weights, centring of y
 * (fit_mean) and the grid rule as pdc_gls_scan.  With M = Phi^T diag(w) Phi, b = Phi^T diag(w) y, YY = sum w y^2:
 *     power_out[j] = b^T M^-1 b / YY        (psd: b^T M^-1 b * 0.5 * sum dy^-2),
 * for nterms = 1 the GLS power.  A bin whose M is not positive definite to rounding (a Cholesky pivot that is not > 0
 * or not finite) is NaN.  n must be at least the number of columns + 1; delta finite and > 0.  dy == NULL: unit
 * uncertainties.  The `_dev` form enqueues on `stream` and keeps its own workspace per (device, stream). */
int pdc_mhgls_scan(const double *t, const double *y, const double *dy, int64_t n,
                   double f0, double delta, int64_t j_begin, int64_t nf, int nterms, int fit_mean, int psd,
                   double *power_out, int device);
int pdc_mhgls_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                       double f0, double delta, int64_t j_begin, int64_t nf, int nterms, int fit_mean, int psd,
                       double *d_power);

/* ---- shared-phase multiband generalised Lomb-Scargle (VanderPlas & Ivezic 2015, ApJ 812, 18: Nbase = nterms, Nband = 0) ----
 * The reference has no such class - PARITY UNPINNED BY THE REFERENCE.  One light curve whose samples carry a band label
 * band[i] in 0 .. n_bands - 1 (n_bands 1 .. 32; filters, instruments): per trial frequency the weighted least-squares fit
 * of ONE Fourier series of `nterms` (1 .. 3) harmonics common to all bands plus, with fit_mean, one floating offset PER
 * BAND.  w_i = dy_i^-2 / sum dy^-2 over all samples, theta_i = 2 pi f (t_i - t_min), grid rule as pdc_gls_scan; y is
 * centred per band on the band's weighted mean (for conditioning: the offsets still float).  With the design
 * 1[band_i = b] (b < n_bands), cos(h theta), sin(h theta) (h = 1 .. nterms), M = Phi^T diag(w) Phi, b = Phi^T diag(w) yc,
 * YY = sum w yc^2:
 *     power_out[j] = b^T M^-1 b / YY        (psd: b^T M^-1 b * 0.5 * sum dy^-2),
 * with one band the value of pdc_mhgls_scan.  Without fit_mean there are no offsets and no centring, the labels do not
 * enter, and the value is that of pdc_mhgls_scan with fit_mean = 0 on the merged curve.  A bin whose reduced normal
 * matrix is not positive definite to rounding (a Cholesky pivot that is not > 0 or not finite) is NaN.
 * Checked before any device is looked for: NULL arguments (band too), negative sizes, nterms, n_bands, delta finite and
 * > 0, n >= n_bands + 2 nterms + 1 (2 nterms + 1 without fit_mean), and in the host form every label in range and every
 * band with at least one sample.  The `_dev` form cannot look at the labels: they are its caller's precondition, a label
 * out of range never indexes memory and makes EVERY bin NaN, a band without samples is skipped.  No atomics: the same
 * bits from call to call.  The `_dev` form enqueues on `stream` and keeps its own workspace per (device, stream). */
int pdc_mbgls_scan(const double *t, const double *y, const double *dy, const int32_t *band, int64_t n, int n_bands,
                   double f0, double delta, int64_t j_begin, int64_t nf, int nterms, int fit_mean, int psd,
                   double *power_out, int device);
int pdc_mbgls_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy,
                       const int32_t *d_band, int64_t n, int n_bands, double f0, double delta, int64_t j_begin, int64_t nf,
                       int nterms, int fit_mean, int psd, double *d_power);
/* Frequencies per tile of the kernel instance `nterms` runs; -1 when nterms is out of range.  No GPU needed. */
int pdc_mbgls_tile_bins(int nterms);

/* ---- Z^2_m and the H-test for event lists (Buccheri et al. 1983, A&A 128, 245; de Jager, Raubenheimer & Swanepoel 1989,
 * A&A 221, 180; photon weights as Kerr 2011, ApJ 732, 38) ------------------------------------------------------------------
 * The reference has no such class - PARITY UNPINNED BY THE REFERENCE.  Arrival times t[n] in ascending order, weights
 * w[n] (NULL: 1), theta_i = 2 pi f (t_i - t[0]); per trial frequency f_j = f0 + (j_begin + j) delta (numpy's arange fill):
 *     C_k = sum w_i cos(k theta_i), S_k = sum w_i sin(k theta_i), Z^2_m = (2 / sum w_i^2) sum_{k <= m} (C_k^2 + S_k^2),
 *     h_out[j] = max_{1 <= m <= nharm} (Z^2_m - 4 m + 4), m_out[j] = the lowest m that reaches it, z2_out[j] = Z^2_nharm.
 * Any output may be NULL, not all.  n >= 1; nf, j_begin >= 0; 1 <= nharm <= 20; delta finite and > 0.  Non-finite input
 * gives IEEE values, never an error.  parts: workgroups that share one tile's events (0: chosen from n, nf, nharm and the
 * device's CU count; with parts > 1 partial sums go through the workspace and are added in a fixed order, so a given
 * count gives the same bits at every call; PDC_WORK_BUDGET_GB lowers the count, never fails).  The `_dev` form enqueues
 * on `stream` and keeps its own workspace per (device, stream). */
int pdc_htest_scan(const double *t, const double *w, int64_t n, double f0, double delta, int64_t j_begin, int64_t nf,
                   int nharm, int parts, double *h_out, int32_t *m_out, double *z2_out, int device);
int pdc_htest_scan_dev(int device, void *stream, const double *d_t, const double *d_w, int64_t n, double f0, double delta,
                       int64_t j_begin, int64_t nf, int nharm, int parts, double *d_h, int32_t *d_m, double *d_z2);
/* Bins per tile of the kernel instance `nharm` runs; -1 when nharm is out of range.  No GPU needed. */
int64_t pdc_htest_tile_bins(int nharm);
/* What the CALLING THREAD's last H-test scan launched (recorded on the host just before the launches, per host thread
 * like pdc_test_gls_last_dispatch; zeros before the first): harmonics of the kernel instance, frequencies per thread,
 * sample parts.  Any pointer may be NULL. */
int pdc_htest_last_dispatch(int *ht, int *k, int *parts);

/* ---- the H-test and Z^2_m over the (frequency, spin-down) plane ---------------------------------------------------------
 * The statistic of pdc_htest_scan with the phase f tau_i + fdot tau_i^2 / 2 cycles, tau_i = t_i - epoch, for every
 * frequency f_j of the grid (as pdc_htest_scan) and every fdot[r], r < nfd (any finite values, any order), reduced on
 * the device.  stat 0: the value of a cell is H (and its m the lowest number of harmonics that reaches it); stat 1: the
 * value is Z^2_nharm, there is no m, and m_plane_out and ridge_m_out must be NULL.  A row with fdot = 0 holds the bits
 * pdc_htest_scan gives with the same `parts`, whatever the epoch.  Outputs, any of them NULL, not all:
 *     plane_out[nfd][nf], m_plane_out[nfd][nf]   the value and m of every cell;
 *     ridge_out[nf], ridge_row_out[nf], ridge_m_out[nf]   per frequency the largest value over the rows, its row and m
 *         as np.nanargmax(plane, axis=0) finds it: NaN never wins, the lowest row of equal maxima wins; a bin with no
 *         finite value has value NaN, row -1 and m -1;
 *     best_out[1], best_at_out[3] = (bin, row, m)   the largest ridge value as np.nanargmax(ridge) finds it (the lowest
 *         bin of equal maxima; m is nharm with stat 1); NaN and (-1, -1, -1) where nothing is finite.
 * Checked before any device is looked for: what pdc_htest_scan checks, nfd >= 1, a finite epoch, stat, and in the host
 * form finite fdot entries (the `_dev` form cannot look at them: a non-finite entry gives a NaN row there).
 * parts: as pdc_htest_scan, 0 chooses from n, nf, nfd, nharm and the CU count with the rows of a launch counted as
 * workgroups.  A launch takes min(nfd, 65535) rows; the workspace holds, per row of a launch, the partial sums
 * (parts > 1) or the values and m the caller does not take (parts == 1).  PDC_WORK_BUDGET_GB lowers the rows per launch
 * first, then the parts, never fails, and changes no bit of the plane, the ridge or the best cell as long as the
 * parts stay.  No atomics: the same bits from call to call.  The `_dev` form takes device pointers (fdot too), enqueues
 * on `stream` and keeps its own workspace per (device, stream). */
int pdc_htest_fdot_scan(const double *t, const double *w, int64_t n, double f0, double delta, int64_t j_begin, int64_t nf,
                        const double *fdot, int64_t nfd, double epoch, int nharm, int stat, int parts, double *plane_out,
                        int32_t *m_plane_out, double *ridge_out, int32_t *ridge_row_out, int32_t *ridge_m_out,
                        double *best_out, int64_t *best_at_out, int device);
int pdc_htest_fdot_scan_dev(int device, void *stream, const double *d_t, const double *d_w, int64_t n, double f0,
                            double delta, int64_t j_begin, int64_t nf, const double *d_fdot, int64_t nfd, double epoch,
                            int nharm, int stat, int parts, double *d_plane, int32_t *d_m_plane, double *d_ridge,
                            int32_t *d_ridge_row, int32_t *d_ridge_m, double *d_best, int64_t *d_best_at);
/* What the CALLING THREAD's last plane scan launched (as pdc_htest_last_dispatch), with the rows of a launch and the
 * number of launches.  Any pointer may be NULL. */
int pdc_htest_fdot_last_dispatch(int *ht, int *k, int *parts, int *rows_per_launch, int64_t *launches);
/* Workspace bytes of a plane scan under the current PDC_WORK_BUDGET_GB, for the H-test with (want_plane != 0) or without
 * both planes; a device of 256 CUs is assumed for parts == 0.  -1 for sizes out of range.  No GPU needed. */
int64_t pdc_htest_fdot_work_bytes(int64_t n, int64_t nf, int64_t nfd, int nharm, int parts, int want_plane);

/* ---- WWZ: the weighted wavelet Z-transform (Foster 1996, AJ 112, 1709) -------------------------------------------------
 * The reference has no such statistic (its timefrequency.WPS needs an evenly sampled series) - PARITY UNPINNED BY THE
 * REFERENCE.  Time-frequency analysis of an unevenly sampled curve: at every time shift tau[r], r < ntau, and every trial
 * frequency f_j = f0 + j delta (numpy's arange fill, f0 >= 0, delta > 0) the weighted least-squares fit of a constant plus
 * a sinusoid under a Gaussian window whose width scales with the period.  Times t[n] never decrease; s_i = dy_i^-2
 * (dy == NULL: 1); omega = 2 pi f; decay c > 0 (Foster: 1 / (8 pi^2)):
 *     w_i = s_i exp(-c omega^2 (t_i - tau)^2),   W = sum w_i,   Neff = W^2 / sum w_i^2,   <a, b> = sum w_i a_i b_i / W,
 *     phi = (1, cos omega (t - t[0]), sin omega (t - t[0])),   S = <phi phi^T>,   b = <phi y>,   a = S^-1 b,
 *     Vx = <y, y> - <1, y>^2,   Vy = a^T b - <1, y>^2,
 *     WWZ = (Neff - 3) Vy / (2 (Vx - Vy)),   WWA = sqrt(a_2^2 + a_3^2)
 * (neither depends on the phase origin; y is centred on its global weighted mean first, which the constant absorbs).  A
 * cell with W not > 0, or with a Cholesky pivot of S not > 0 or not finite, is NaN in WWZ and WWA; Neff is 0 where W is
 * not > 0.  Samples whose exponent c (2 pi f_lo)^2 (t_i - tau)^2 at the LOWEST frequency f_lo of a tile of
 * pdc_wwz_tile_bins() bins exceeds 746 are skipped for that (tile, tau): their weight is exactly 0 in fp64 at every
 * frequency of the tile.  Outputs, any of them NULL, not all:
 *     wwz_out[ntau][nf], amp_out[ntau][nf], neff_out[ntau][nf]   WWZ, WWA and Neff of every cell;
 *     ridge_bin_out[ntau], ridge_wwz_out[ntau], ridge_amp_out[ntau]   per tau the bin of the largest WWZ among the cells
 *         with Neff >= min_neff, as np.nanargmax(np.where(neff >= min_neff, wwz, nan), axis=1) finds it (NaN never wins,
 *         the lowest bin of equal maxima wins), with its WWZ and WWA; bin -1 and NaN where no cell is eligible;
 *     best_out[1], best_at_out[2] = (row, bin)   the largest ridge value as np.nanargmax finds it in ascending row order;
 *         NaN and (-1, -1) where no row has a bin;
 *     visited_out[1]   the samples that were not skipped, summed over all (tile, tau).
 * min_neff applies to the reductions only, never to the planes.  Checked before any device is looked for: f0 finite and
 * >= 0, delta finite and > 0, nf >= 1, n >= 4, ntau >= 1, decay finite and > 0, min_neff finite, not every output NULL,
 * and in the host form finite t that never decrease and finite tau (the `_dev` form cannot look at them: they are its
 * caller's precondition, and no value of them indexes memory out of bounds).  A launch takes at most 65535 rows; no bit
 * depends on the rows per launch.  No atomics: the same bits from call to call.  The `_dev` form takes device pointers
 * (tau too), enqueues on `stream` and keeps its own workspace per (device, stream). */
int pdc_wwz_scan(const double *t, const double *y, const double *dy, int64_t n, double f0, double delta, int64_t nf,
                 const double *tau, int64_t ntau, double decay, double min_neff, double *wwz_out, double *amp_out,
                 double *neff_out, int64_t *ridge_bin_out, double *ridge_wwz_out, double *ridge_amp_out, double *best_out,
                 int64_t *best_at_out, int64_t *visited_out, int device);
int pdc_wwz_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                     double f0, double delta, int64_t nf, const double *d_tau, int64_t ntau, double decay,
                     double min_neff, double *d_wwz, double *d_amp, double *d_neff, int64_t *d_ridge_bin,
                     double *d_ridge_wwz, double *d_ridge_amp, double *d_best, int64_t *d_best_at, int64_t *d_visited);
/* Bins per tile of the scan (the unit of the support cut).  No GPU needed. */
int64_t pdc_wwz_tile_bins(void);
/* Workspace bytes of a scan; -1 for sizes out of range (n < 4, nf < 1, ntau < 1, a plane too large).  No GPU needed. */
int64_t pdc_wwz_work_bytes(int64_t n, int64_t nf, int64_t ntau);
/* What the CALLING THREAD's last WWZ scan launched (as pdc_htest_last_dispatch; zeros before the first): frequencies per
 * thread, rows per launch, launches of the scan kernel.  Any pointer may be NULL. */
int pdc_wwz_last_dispatch(int *k, int *rows_per_launch, int64_t *launches);

/* ---- WPS: the Morlet wavelet power spectrum of an evenly sampled curve -------------------------------------------------
 * The reference's timefrequency.WPS calls PyWavelets, cwt(values - mean, scales, "cmor2.0-1.0", dt), squares and divides
 * by the scale.  PyWavelets is not a dependency: its published algorithm is restated here - PARITY UNPINNED BY THE
 * REFERENCE.  The caller tabulates the integrated wavelet, table[1024] complex (re, im interleaved), on 1024 points `step`
 * apart over a support `span` wide (cmor2.0-1.0: np.linspace(-8, 8, 1024), conj(cumsum(psi) step), span 16).  With x the
 * centred samples (x[N], the caller subtracts the mean), zero outside [0, N), and per scale s (samples per period):
 *     j[m] = trunc(m / (s step)), m = 0 .. ceil(s span + 1) - 1, kept while j[m] < 1024: L entries (L >= 2);
 *     h[k] = table[j[L-1-k]], h[-1] = h[L] = 0;
 *     coef[n] = -sqrt(s) sum_{k = 0 .. L} (h[k] - h[k-1]) x[n + floor(L / 2) - k];   spectrum[n] = |coef[n]|^2 / s
 * - np.convolve(x, h), np.diff, times -sqrt(s), the centred cut to N, as one sum.  The positions where h changes are those
 * of numpy's rule bit for bit (every operation above rounds once, the division included).  h changes at no more than 1025
 * positions whatever the scale (the TAPS), so a cell costs at most 1025 complex-by-real multiply-adds, summed in ascending
 * filter position.  Cone of influence: cell (i, n) is inside where corr * periods[i] < min(t[n] - t_min, t_max - t[n])
 * (each operation rounded once, as numpy's; corr = exp2(0.5) in the reference).  Outputs, any of them NULL, not all:
 *     spectrum_out[n_scales][N], coefs_out[n_scales][N] complex (re, im interleaved)   the planes;
 *     gwps_out[n_scales]   mean over time;   sav_out[N]   mean over the scales;
 *     masked_gwps_out[n_scales], gwps_count_out[n_scales], masked_sav_out[N], sav_count_out[N]   the means over the cells
 *         inside the cone, as np.nanmean of the masked plane gives them, NaN where the count is 0.
 * Without the two planes no [n_scales][N] array exists anywhere.  The rows sum tiles of pdc_wps_tile() time indices in
 * ascending order, the columns sum chunks of scales in ascending order (8 scales; more where PDC_WORK_BUDGET_GB or the
 * 65535 chunks of a launch ask for fewer partials).  No atomics: the same bits from call to call, and a scale's row does
 * not depend on the other scales.  Checked before any device is looked for: N >= 1, n_scales >= 1, step and span finite
 * and > 0, not every output NULL, and in the host form finite x, t, periods, table and corr, and every scale with
 * 2 <= L and s <= 2^24 (the `_dev` form cannot look: a scale it cannot serve gives NaN rows, and no value indexes memory
 * out of bounds).  The `_dev` form takes device pointers and t_min, t_max, enqueues on `stream` and keeps its own
 * workspace per (device, stream). */
int pdc_wps_scan(const double *x, const double *t, int64_t n, const double *periods, const double *scales,
                 int64_t n_scales, const double *table, double step, double span, double corr, double *spectrum_out,
                 double *coefs_out, double *gwps_out, double *sav_out, double *masked_gwps_out, int64_t *gwps_count_out,
                 double *masked_sav_out, int64_t *sav_count_out, int device);
int pdc_wps_scan_dev(int device, void *stream, const double *d_x, const double *d_t, int64_t n, const double *d_periods,
                     const double *d_scales, int64_t n_scales, const double *d_table, double step, double span,
                     double corr, double t_min, double t_max, double *d_spectrum, double *d_coefs, double *d_gwps,
                     double *d_sav, double *d_masked_gwps, int64_t *d_gwps_count, double *d_masked_sav,
                     int64_t *d_sav_count);
/* The taps of one scale as the device builds them, on the host (the same function): position_out[<= 1025] ascending,
 * before_out / after_out the table entries on either side (-1: outside the filter), length_out[1] = L.  Returns the
 * number of taps, or a negative status.  Any pointer may be NULL.  No GPU needed. */
int64_t pdc_wps_taps(double scale, double step, double span, int64_t *position_out, int32_t *before_out,
                     int32_t *after_out, int64_t *length_out);
/* Time indices per workgroup of the scan.  No GPU needed. */
int64_t pdc_wps_tile(void);
/* Workspace bytes of a scan under the current PDC_WORK_BUDGET_GB; -1 for sizes out of range.  No GPU needed. */
int64_t pdc_wps_work_bytes(int64_t n, int64_t n_scales);
/* What the CALLING THREAD's last WPS scan launched (zeros before the first): tiles, chunks of scales, scales per chunk,
 * and - host form only, -1 after a `_dev` call - the scales whose every filter position is a tap (L + 1 <= 1025) and those
 * served from change points.  Any pointer may be NULL. */
int pdc_wps_last_dispatch(int64_t *tiles, int64_t *chunks, int64_t *scales_per_chunk, int64_t *dense_scales,
                          int64_t *sparse_scales);

/* ---- EMD and CEEMDAN: empirical mode decomposition --------------------------------------------------------------------
 * The reference's decomposition.EMD (Rilling et al. 2003) and the ensemble stage of its CEEMDAN, restated from its calls
 * (scipy.signal.find_peaks, np.pad, splrep / splev); its TSeries needs xarray, which is not a dependency: PARITY UNPINNED
 * BY THE REFERENCE.  A row x[N] on the strictly increasing times t[N]; one sift evaluation of the working mode v:
 *     M, D        interior maxima / minima as find_peaks(prominence=0) lists them (a flat top once, at (left + right) / 2;
 *                 a plateau that touches an edge is none); n_zero = #{i : signbit(v[i]) != signbit(v[i + 1])};
 *     monotonic   if |M| < p or |D| < p or |M| + 2 p < 4 or |D| + 2 p < 4 (p = pad_width);
 *     knots       p extrema reflected about t[0] (time 2 t[0] - t[M[p-1-j]], value v[M[p-1-j]]), M itself, p reflected
 *                 about t[N-1]; the envelope is the not-a-knot cubic spline through them, evaluated at every t[i];
 *     mu = (U + L) / 2, amp = (U - L) / 2, sigma = |mu / amp|;
 *     is_imf = count(sigma > theta_1) / N < alpha and all(sigma < theta_2) and |n_zero - (|M| + |D|)| <= 1 (ordered
 *                 comparisons: a NaN sigma is neither);  if not, v -= mu, at most max_iter times.
 * residue = x; while the residue is not monotonic and fewer than max_modes modes exist, the next mode is sifted from it
 * and subtracted.  One workgroup per row, the sift loop inside the kernel; rows of at most pdc_emd_lds_samples() samples
 * with pad_width <= 8 keep the mode in LDS, longer ones in a slab of the workspace - the same code, the same bits, and a
 * row's bytes depend neither on its place in the batch nor on the call.  PDC_EMD_FORCE_GLOBAL=1 sends every row through
 * the workspace route.  Outputs: modes_out[B][max_modes][N] (the host form writes a row's first n_modes, the `_dev` form
 * too, the rest is left as it was), residue_out[B][N], n_modes_out[B], sifts_out[B][max_modes] (updates applied to mode k;
 * the host form zeroes the rest), flags_out[B]: bit 0 a mode ran into max_iter, bit 1 max_modes reached with the residue
 * not monotonic.  Checked before any device is looked for: 1 <= N <= 2^24, pad_width 0 .. 2^20, max_modes 1 .. 64,
 * max_iter 1 .. 10^6, the thresholds finite, and - host forms - finite samples and strictly increasing finite times. */
int pdc_emd_batch(const double *t, const double *x, int64_t n, int64_t n_rows, int64_t max_iter, int pad_width,
                  double theta_1, double theta_2, double alpha, int max_modes, double *modes_out, double *residue_out,
                  int64_t *n_modes_out, int64_t *sifts_out, int64_t *flags_out, int device);
int pdc_emd_batch_dev(int device, void *stream, const double *d_t, const double *d_x, int64_t n, int64_t n_rows,
                      int64_t max_iter, int pad_width, double theta_1, double theta_2, double alpha, int max_modes,
                      double *d_modes, double *d_residue, int64_t *d_n_modes, int64_t *d_sifts, int64_t *d_flags);
/* One sift evaluation of one row with the batch kernel's own device functions: upper_out[N], lower_out[N] (untouched,
 * zero, when monotonic), idx_max_out / idx_min_out[N / 2 + 1] (the lists, zero beyond their counts), counts_out[4] =
 * maxima, minima, n_zero, 1 if monotonic. */
int pdc_emd_sift(const double *t, const double *x, int64_t n, int pad_width, double *upper_out, double *lower_out,
                 int32_t *idx_max_out, int32_t *idx_min_out, int64_t *counts_out, int device);
/* One stage of CEEMDAN on the device: noisy[e] = residue + beta[e] * noise_modes[e][k] where n_noise_modes[e] > k (the
 * residue itself where not), the first mode of each noisy row, mu[N] = sum over e ascending of (noisy[e] - mode[e]) / E,
 * a realisation whose noisy row is monotonic adding zero.  noise_modes[E][noise_max_modes][N] and n_noise_modes[E] are
 * what pdc_emd_batch_dev left on the device; n_modes[E], sifts[E], flags[E] describe the stage's own decompositions.
 * Nothing of size E N leaves the device. */
int pdc_ceemdan_stage_dev(int device, void *stream, const double *d_t, const double *d_residue, int64_t n,
                          const double *d_noise_modes, const int64_t *d_noise_n_modes, int64_t ensemble,
                          int noise_max_modes, int k, const double *d_beta, int64_t max_iter, int pad_width,
                          double theta_1, double theta_2, double alpha, double *d_mu, int64_t *d_n_modes,
                          int64_t *d_sifts, int64_t *d_flags);
/* Longest row the LDS route serves.  No GPU needed. */
int64_t pdc_emd_lds_samples(void);
/* Workspace bytes of a batch (the global route sized for 256 compute units); -1 for sizes out of range.  No GPU needed. */
int64_t pdc_emd_work_bytes(int64_t n, int64_t n_rows, int pad_width);
/* What the CALLING THREAD's last EMD call launched (zeros before the first): route (1 LDS, 2 workspace), threads per
 * workgroup, rows, and - host batch form only, -1 otherwise - the sift evaluations of all rows.  Any pointer may be NULL. */
int pdc_emd_last_dispatch(int64_t *route, int64_t *threads, int64_t *rows, int64_t *sift_evaluations);

/* ---- the Keplerian periodogram (Zechmeister & Kurster 2009, A&A 496, 577, section 4) -----------------------------------
 * The reference has no such class - PARITY UNPINNED BY THE REFERENCE.  Per trial frequency the best weighted least-squares
 * fit of a Keplerian orbit over a grid of eccentricities ecc[ne], each in [0, 0.95], and mean anomalies at t[0] m0[nm],
 * each in [0, 1) cycles.  Inputs, weights w_i = dy_i^-2 / sum dy^-2 (dy == NULL: unit uncertainties), centring of y on
 * its weighted mean (fit_mean) and the grid rule f_j = f0 + j delta (numpy's arange fill) as pdc_mhgls_scan;
 * t' = t - t[0].  Cell c = k nm + l of bin j:
 *     phi_i = frac(f_j t'_i), reduced exactly;   M_i = 2 pi (phi_i - m0_l);   E_i solves E - e_k sin E = M_i;
 *     cos nu = (cos E - e) / (1 - e cos E),   sin nu = sqrt(1 - e^2) sin E / (1 - e cos E);
 *     cube[j][k][l] = b^T M^-1 b / YY        (psd: b^T M^-1 b * 0.5 * sum dy^-2)
 * with design columns cos nu, sin nu and a constant when fit_mean, M = Phi^T diag(w) Phi, b = Phi^T diag(w) y,
 * YY = sum w y^2.  A cell whose M has a Cholesky pivot that is not > 0, or not finite, is NaN.  At e = 0 the cell is the
 * GLS power for every m0.  Outputs, any of them NULL, not all:
 *     power_out[nf]   the largest cell of the bin, as np.nanmax gives it;
 *     cell_out[nf]    the index of that cell as np.nanargmax over the row-major [ne][nm] cells finds it: NaN never wins,
 *         the lowest index of equal maxima wins; index -1 and power NaN where every cell is NaN;
 *     cube_out[nf][ne][nm]   every cell (for tests and small problems);
 *     best_out[1], best_at_out[2] = (bin, cell)   the largest power_out in ascending bin order; NaN and (-1, -1) if no
 *         bin has a value.
 * Checked before any device is looked for: f0 finite and >= 0, delta finite and > 0, nf >= 1, n >= 4, 1 <= ne, 1 <= nm,
 * ne nm <= 65535, every ecc finite and in [0, 0.95], every m0 finite and in [0, 1), not every output NULL, and in the
 * host form finite t.  The `_dev` form takes device pointers (ecc and m0 too) and cannot look at the lists: a cell whose
 * e or m0 is out of range indexes nothing and is NaN.  The Kepler solve has a fixed trip count (Markley 1995): cos nu and
 * sin nu are within 1e-12 of their values over the whole range, which is what the cap of 0.95 on e buys (d nu / d M
 * reaches 125 there).  PDC_WORK_BUDGET_GB cuts the grid into slabs of whole tiles, at least one, scanned one after the
 * other.  No atomics: the same bits from call to call, and no bit of a cell depends on its place in the lists, on the
 * other cells of the call or on the slabs.  The `_dev` form enqueues on `stream` and keeps its own workspace per
 * (device, stream). */
int pdc_kepler_scan(const double *t, const double *y, const double *dy, int64_t n, double f0, double delta, int64_t nf,
                    const double *ecc, int64_t ne, const double *m0, int64_t nm, int fit_mean, int psd, double *power_out,
                    int32_t *cell_out, double *cube_out, double *best_out, int64_t *best_at_out, int device);
int pdc_kepler_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                        double f0, double delta, int64_t nf, const double *d_ecc, int64_t ne, const double *d_m0,
                        int64_t nm, int fit_mean, int psd, double *d_power, int32_t *d_cell, double *d_cube,
                        double *d_best, int64_t *d_best_at);
/* cos nu and sin nu of `count` pairs (phase[i] in cycles, any finite value; e[i] in [0, 0.95]) by the device function
 * the scan runs.  Host arrays. */
int pdc_kepler_anomaly(const double *phase, const double *e, int64_t count, double *cos_out, double *sin_out, int device);
/* Cells per thread of the scan (a workgroup takes one tile of bins and this many cells).  No GPU needed. */
int pdc_kepler_cell_group(void);
/* Bins per tile of the scan: 256.  No GPU needed. */
int64_t pdc_kepler_tile_bins(void);
/* Workspace bytes of a scan under the current PDC_WORK_BUDGET_GB; -1 for sizes out of range (what the scan refuses, the
 * cube counted when want_cube).  No GPU needed. */
int64_t pdc_kepler_work_bytes(int64_t n, int64_t nf, int64_t ne, int64_t nm, int want_cube);
/* What the CALLING THREAD's last Keplerian scan launched (as pdc_htest_last_dispatch; zeros before the first): cells per
 * thread, cell groups, launches of the scan kernel (slabs).  Any pointer may be NULL. */
int pdc_kepler_last_dispatch(int *kc, int *groups, int64_t *launches);

/* ---- DCF: the discrete correlation function (Edelson & Krolik 1988, ApJ 333, 646) --------------------------------------
 * The reference has an autocorrelation for evenly sampled series only (an inverse FFT on median_dt, core.py:578-608) and
 * no cross-correlation - PARITY UNPINNED BY THE REFERENCE.  Auto- and cross-correlation of unevenly sampled curves: every
 * ordered pair of a sample i of (ta[na], a[na]) and a sample j of (tb[nb], b[nb]) is binned by its lag; nothing is
 * interpolated.  Times are finite and never decrease; a and b are taken as they come (centring is the caller's);
 * edges[nlag + 1] is finite and strictly increasing.  THE DEFINITION: pair (i, j) has lag d = fl(tb[j] - ta[i]), one IEEE
 * double subtraction, and belongs to bin k iff edges[k] <= d < edges[k+1], compared in double - no other form of the
 * comparison is evaluated anywhere, so a pair with edges[0] <= d < edges[nlag] is in exactly one bin.  With
 * skip_same_index the pairs i == j are left out (autocorrelation: na == nb, the same arrays twice).  Per bin:
 *     pairs_out[k]            the count;
 *     sums_out[6][nlag]       Sa = sum a_i, Sb = sum b_j, Saa = sum a_i^2, Sbb = sum b_j^2, Sab = sum a_i b_j,
 *                             Sabab = sum (a_i b_j)^2 over the bin's pairs, in this order;
 * an empty bin has count 0 and six sums of exactly 0.0.  A NaN in a or b is no error: it reaches the sums of the bins
 * its pairs fall in (a_i: Sa, Saa, Sab, Sabab; b_j: Sb, Sbb, Sab, Sabab) and no others.  To first order in 2^-53 each
 * sum is within (pairs[k] + 8) 2^-53 sum |term| of its exact value (the bound the tests hold it to).  The i are cut into chunks of `chunk` consecutive samples (0: the
 * library chooses, pdc_dcf_chunk; positive: a test and tuning hook, like `slices` of pdc_bls_scan), each chunk writes a
 * slab of partial sums to the workspace and the slabs are summed in chunk order: no atomics, the same bits from call to
 * call (another chunk: other roundings, the same counts).  PDC_WORK_BUDGET_GB enlarges the chunk until the slabs fit; a
 * budget that not even one chunk of all samples fits in is an error.  Checked before any device is looked for: 0 <= na,
 * nb <= 2^31 - 64 (0 is valid: all-zero outputs), 1 <= nlag <= 2^22, chunk >= 0 and fewer than 2^24 chunks, skip_same_index only with na == nb, no NULL
 * argument, and in the host form finite times that never decrease and finite, strictly increasing edges (the `_dev` form
 * cannot look at them: they are its caller's precondition, and no value of them indexes memory out of bounds).  The
 * `_dev` form takes device pointers, enqueues on `stream` and keeps its own workspace per (device, stream). */
int pdc_dcf_scan(const double *ta, const double *a, int64_t na, const double *tb, const double *b, int64_t nb,
                 const double *edges, int64_t nlag, int skip_same_index, int64_t chunk, int64_t *pairs_out,
                 double *sums_out, int device);
int pdc_dcf_scan_dev(int device, void *stream, const double *d_ta, const double *d_a, int64_t na, const double *d_tb,
                     const double *d_b, int64_t nb, const double *d_edges, int64_t nlag, int skip_same_index,
                     int64_t chunk, int64_t *d_pairs, double *d_sums);
/* Workspace bytes of a scan under the current PDC_WORK_BUDGET_GB (chunk as for the scan); -1 for sizes the scan
 * refuses.  No GPU needed. */
int64_t pdc_dcf_work_bytes(int64_t na, int64_t nb, int64_t nlag, int64_t chunk);
/* The samples per chunk the library chooses for chunk == 0 under the current PDC_WORK_BUDGET_GB (at least 1); -1 for
 * sizes the scan refuses.  No GPU needed. */
int64_t pdc_dcf_chunk(int64_t na, int64_t nb, int64_t nlag);
/* What the CALLING THREAD's last DCF scan launched (as pdc_htest_last_dispatch; zeros before the first): the chunks
 * (0: a curve was empty) and the samples per chunk.  Any pointer may be NULL. */
int pdc_dcf_last_dispatch(int64_t *chunks, int64_t *chunk);

/* ---- GP: celerite log-likelihoods of one curve under many kernels (Foreman-Mackey et al. 2017, AJ 154, 220) -----------
 * The reference's gp.py evaluates `gp.compute(...); gp.log_likelihood(y)` once per hyper-parameter vector through
 * celerite2; these entries evaluate M vectors ("candidates") in one call.  A candidate is J terms of four coefficients
 * (a, b, c, nu): k(D) = sum_j exp(-c_j |D|) (a_j cos(2 pi nu_j D) + b_j sin(2 pi nu_j |D|)) - nu = d / 2 pi of
 * celerite's d, in CYCLES per time unit, so that phases are reduced before they meet 2 pi; a real term is b = nu = 0 -
 * plus jitter[m] >= 0 added to every var and a mean.  coeff is [M][J][4], jitter [M], mean [M] or NULL (0).
 * t_rel[n] = t - t[0] of the sorted times (never decreasing, t_rel[0] == 0), y[n], var[n] = err^2 >= 0.  The recursion
 * is the celerite2 one (S <- P o (S + D W W^T) o P^T: no overflow), see csrc/gp.hip.
 *     loglike_out[M]   ln L = -1/2 sum_n (z_n^2 / D_n + ln D_n) - n/2 ln 2 pi; -inf for a candidate with a D_n that is not
 *                      a positive finite number (its matrix is not positive definite);
 *     mean_out[M]      the mean used: with fit_mean the profiled one, sum z z1 / D / sum z1^2 / D (z1 the solve of the
 *                      all-ones vector), and ln L is the likelihood at it; else mean[m] (0 without mean); NaN where
 *                      ln L is -inf;
 *     status_out[M]    0, or the 1-based index of the first sample whose D_n is not positive and finite.
 * fit_mean with a mean array is refused.  A candidate's bits depend on its coefficients and the curve alone - not on
 * m, M, its neighbours or the slabs: PDC_WORK_BUDGET_GB cuts M into slabs of whole workgroups (64 candidates) whose
 * repacked coefficients fit the budget beside the fixed part, at least one workgroup.  No atomics.
 * pdc_gp_scan: the candidates are a grid [np][nq], period-major, nq <= 65535 cells of nuisance parameters per trial
 * period; besides the likelihoods (cube_out[np][nq], may be NULL)
 *     profile_out[np]      the largest finite ln L of the period's cells (the first of equal ones); NaN if none;
 *     cell_out[np]         its cell, -1 if none;
 *     marginal_out[np]     ln of the mean likelihood of the cells: logsumexp over the finite cells - ln nq; -inf if none;
 *     period_mean_out[np]  mean_out of that cell; NaN if none;
 *     best_out[1], best_at_out[2]   the largest profile value (of equal ones the first period), its period and cell;
 *                          NaN and (-1, -1) if no cell of the grid is finite.
 * Any output may be NULL, not all.  Checked before any device is looked for: 1 <= n < 2^31, 1 <= J <=
 * pdc_gp_max_terms(), 1 <= M <= 2^40, np nq == M, np <= 2^38, and in the host form finite t_rel that starts at 0 and never
 * decreases, finite y, finite var >= 0, finite coefficients with c >= 0, finite jitter >= 0, finite means (the `_dev`
 * form cannot look: they are its caller's precondition, and no value of them indexes memory).  The `_dev` forms take
 * device pointers, enqueue on `stream` and keep their own workspace per (device, stream). */
int pdc_gp_loglike(const double *t_rel, const double *y, const double *var, int64_t n, const double *coeff, int J,
                   const double *jitter, const double *mean, int64_t M, int fit_mean, double *loglike_out, double *mean_out,
                   int32_t *status_out, int device);
int pdc_gp_loglike_dev(int device, void *stream, const double *d_t_rel, const double *d_y, const double *d_var, int64_t n,
                       const double *d_coeff, int J, const double *d_jitter, const double *d_mean, int64_t M, int fit_mean,
                       double *d_loglike, double *d_mean_out, int32_t *d_status);
int pdc_gp_scan(const double *t_rel, const double *y, const double *var, int64_t n, const double *coeff, int J,
                const double *jitter, const double *mean, int64_t M, int fit_mean, int64_t np, int64_t nq,
                double *profile_out, int32_t *cell_out, double *marginal_out, double *period_mean_out, double *cube_out,
                double *best_out, int64_t *best_at_out, int device);
int pdc_gp_scan_dev(int device, void *stream, const double *d_t_rel, const double *d_y, const double *d_var, int64_t n,
                    const double *d_coeff, int J, const double *d_jitter, const double *d_mean, int64_t M, int fit_mean,
                    int64_t np, int64_t nq, double *d_profile, int32_t *d_cell, double *d_marginal, double *d_period_mean,
                    double *d_cube, double *d_best, int64_t *d_best_at);
/* Workspace bytes of a scan under the current PDC_WORK_BUDGET_GB (want_cube: the caller's cube takes the likelihoods); -1
 * for sizes out of range.  pdc_gp_loglike needs less: the records and the slab's coefficients alone.  No GPU needed. */
int64_t pdc_gp_work_bytes(int64_t n, int64_t M, int J, int want_cube);
/* The largest J the library was built for.  No GPU needed. */
int pdc_gp_max_terms(void);
/* Samples the likelihood kernel stages at a time (the seam its tests straddle).  No GPU needed. */
int pdc_gp_chunk_samples(void);
/* What the CALLING THREAD's last GP call launched (as pdc_htest_last_dispatch; zeros before the first): J, fit_mean,
 * launches of the likelihood kernel (slabs).  Any pointer may be NULL. */
int pdc_gp_last_dispatch(int *J, int *fit_mean, int64_t *launches);

/* ---- BLS: box least squares (Kovacs, Zucker & Mazeh 2002, A&A 391, 369) ----------------------------------------------
 * The reference has no such class - PARITY UNPINNED BY THE REFERENCE.  The search for a box-shaped dip (a transit, a
 * detached eclipse): per trial period the best two-level model of the folded curve.  Weights and centring as
 * pdc_gls_scan: w = dy^-2 / sum dy^-2 (dy == NULL: unit uncertainties), y' = y - sum w y, YY = sum w y'^2.  Phase
 * phi = (t / P) % 1 in n_bins bins [k / n_bins, (k + 1) / n_bins) with numpy's membership (the edges are the doubles
 * k / n_bins, phi == 1.0 joins the last bin).  A box is a start bin i (0 .. n_bins - 1) and a length of L
 * (len_min .. len_max) bins, wrapping past phase 1, with r = sum w, s = sum w y', c = count over its samples; it is
 * admissible when c >= min_points, N_binned - c >= min_points and 0 < r < 1 (dips_only: also s < 0).  Per period
 *     power[j]     = max over admissible boxes of SR / YY,  SR = s^2 / (r (1 - r))   (in [0, 1])
 *     start_bin[j], box_bins[j] = the maximising (i, L); among equal SR the smaller L, then the smaller i
 *     depth[j]     = -s / (r (1 - r)) of that box: out-of-box level minus in-box level, positive for a dip.
 * No admissible box: NaN, NaN, -1, -1.  A non-finite t, y or dy, dy == 0 or YY == 0 anywhere: every output NaN / -1;
 * a period at which a phase is NaN (0, NaN): NaN / -1 at that period only.  Limits, checked before any device work:
 * 2 <= n_bins <= 2048, 1 <= len_min <= len_max <= n_bins - 1, min_points >= 1, 0 <= slices <= 1024, n and n_periods
 * in 0 .. 2^31 - 1.  The sums are 64-bit fixed point (weights scaled by 2^60): exact and independent of order, so
 * every `slices` gives the same bits; a window sum is within n 2^-61 of the real one on a scale where the total
 * weight is 1.  slices: workgroups that share the samples of one trial period (1: one workgroup bins and searches; > 1:
 * through a global histogram of n_periods n_bins 20 bytes in the workspace, an error when that does not fit the
 * workspace budget); 0 chooses from the shape.  depth, start_bin and box_bins may be NULL.  The `_dev` form takes
 * device pointers, enqueues on `stream` and keeps its own workspace per (device, stream). */
int pdc_bls_scan(const double *t, const double *y, const double *dy, int64_t n,
                 const double *periods, int64_t n_periods, int n_bins, int len_min, int len_max, int min_points,
                 int dips_only, int slices,
                 double *power, double *depth, int32_t *start_bin, int32_t *box_bins, int device);
int pdc_bls_scan_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy, int64_t n,
                     const double *d_periods, int64_t n_periods, int n_bins, int len_min, int len_max, int min_points,
                     int dips_only, int slices,
                     double *d_power, double *d_depth, int32_t *d_start_bin, int32_t *d_box_bins);

/* ---- BLS over curves on their OWN period grids (BLS.batch) -------------------------------------------
 * Replaces a survey's loop of BLS()(s, e): curve b owns samples [offsets[b], offsets[b+1]) of t, y and dy (dy == NULL:
 * unit uncertainties for every curve) and the trial periods linspace(start[b], stop[b], P_b),
 * P_b = p_offsets[b+1] - p_offsets[b], rebuilt on the device with numpy's rule as for pdc_phase_scan_ragged (for
 * P_b == 1 pass step = stop - start).  n_bins ... dips_only are those of pdc_bls_scan, shared by all curves, with its
 * limits; there is no `slices`: one workgroup bins and searches one (curve, period).  The rows power, depth,
 * start_bin, box_bins [p_offsets[B]] come back in period order, X[p_offsets[b] + j], and are BIT-IDENTICAL to
 * pdc_bls_scan on that curve and those periods at every curve length and every `slices` (the sums are integers).
 * best_* [B]: index = the first period index of the row's largest power (np.nanargmax), -1 for a row without a
 * finite power (an empty curve, an empty grid, bad input, no admissible box anywhere); power, depth, start, box =
 * the rows' values there, NaN / -1 where index is -1.  Any output may be NULL, but not all of them.
 * Devices, groups and budget as for pdc_phase_scan_ragged: contiguous groups balanced by sum n_b P_b over the
 * `n_devices` listed slots, per-slot buffers kept until pdc_release, groups that fit PDC_WORK_BUDGET_GB and free
 * memory, the same bits for any grouping.
 *
 * pdc_bls_ragged_peaks: also the [B][k] peak table (k <= 1024) of pdc_gls_ragged_peaks on every curve's power row in
 * FSeries order (ascending frequency 1/p: index j' = P_b - 1 - j when stop[b] > start[b], j' = j otherwise).  The
 * rows may all be NULL: they stay in HBM.
 *
 * pdc_bls_ragged_work_bytes / pdc_bls_scan_ragged_dev: ONE launch sequence on `device` / `stream`, no grouping:
 * d_t, d_y, d_dy and every output on the device; offsets ... p_offsets on the HOST (the entry waits for their
 * upload before it returns, not for the launches).  d_pitched [B][pitch]: the power rows in FSeries order (its pad is
 * the caller's).  work_bytes >= pdc_bls_ragged_work_bytes(B, offsets[B], p_offsets[B], 0, 0), which covers the
 * records (24 bytes a sample) and the rows of every NULL output; p_max > 0 and k > 0 add the pitched copy and the
 * [B][k] table of the peak entry's groups. */
int pdc_bls_scan_ragged(const double *t, const double *y, const double *dy, const int64_t *offsets, int64_t n_curves,
                        const double *start, const double *step, const double *stop, const int64_t *p_offsets,
                        int n_bins, int len_min, int len_max, int min_points, int dips_only,
                        double *power, double *depth, int32_t *start_bin, int32_t *box_bins,
                        int64_t *best_index, double *best_power, double *best_depth, int32_t *best_start,
                        int32_t *best_box, const int *devices, int n_devices);
int pdc_bls_ragged_peaks(const double *t, const double *y, const double *dy, const int64_t *offsets, int64_t n_curves,
                         const double *start, const double *step, const double *stop, const int64_t *p_offsets,
                         int n_bins, int len_min, int len_max, int min_points, int dips_only, int k, int by_prominence,
                         int64_t *count_out, int64_t *idx_out, double *height_out, double *prominence_out,
                         int64_t *half_lo_out, int64_t *half_hi_out,
                         double *power, double *depth, int32_t *start_bin, int32_t *box_bins,
                         int64_t *best_index, double *best_power, double *best_depth, int32_t *best_start,
                         int32_t *best_box, const int *devices, int n_devices);
int64_t pdc_bls_ragged_work_bytes(int64_t n_curves, int64_t n_total, int64_t p_total, int64_t p_max, int k);
/* TEST HOOK (not for callers): how many groups of curves the last pdc_bls_scan_ragged / pdc_bls_ragged_peaks call of
 * this process ran, summed over its device slots. */
int pdc_test_bls_ragged_groups(int64_t *groups);
int pdc_bls_scan_ragged_dev(int device, void *stream, const double *d_t, const double *d_y, const double *d_dy,
                            const int64_t *offsets, int64_t n_curves, const double *start, const double *step,
                            const double *stop, const int64_t *p_offsets,
                            int n_bins, int len_min, int len_max, int min_points, int dips_only,
                            double *d_power, double *d_depth, int32_t *d_start_bin, int32_t *d_box_bins,
                            int64_t *d_best_index, double *d_best_power, double *d_best_depth, int32_t *d_best_start,
                            int32_t *d_best_box, double *d_pitched, int64_t pitch, void *work, int64_t work_bytes);

/* Device-resident form used by bench.py: inputs already in HBM, no synchronisation.
 * `work` is scratch of at least pdc_gls_work_bytes(n_total, n_curves, nf) bytes on the same
 * device (non-decreasing in n_total and in nf: a buffer sized for the largest call serves all; for a
 * single curve it includes up to 48 MiB for the partial sums of short grids, whose samples are cut
 * into parts as well; for the mirrored-pair kernel 256 bytes per sample of offset table, 32 bytes per sample of fill
 * steps and 128 bytes per 64 samples and per curve of chunk remainders).  d_offsets may be NULL for a single curve of
 * n_total samples. */
int64_t pdc_gls_work_bytes(int64_t n_total, int64_t n_curves, int64_t nf);
int pdc_gls_scan_dev(int device, void *stream,
                     const double *d_t, const double *d_y, const double *d_dy,
                     const int64_t *d_offsets, int64_t n_total, int64_t n_curves, int shared_t,
                     double f0, double delta, int64_t j_begin, int64_t nf,
                     int fit_mean, int psd,
                     double *d_power, double *d_amax, int64_t *d_argmax,
                     void *work, int64_t work_bytes);
/* TEST HOOK (not for callers): the route the CALLING THREAD's last direct-sum scan took inside the library (every entry
 * above, pdc_gls_bootstrap with method 0 and the plans' enqueueing thread end in the same dispatcher) and its launch
 * shape, recorded on the host just before the launches.  The record is per host thread, so concurrent scans on other
 * threads do not disturb it; all zeros before the thread's first scan.  out[14] = route (1 general, 2 general with
 * sample parts, 3 balanced pieces, 4 shared time axis, 5 shared time axis with two frequencies per lane), K (frequencies
 * per thread; per lane on the shared routes), S (waves per frequency tile; 0 on the shared routes), frequency tiles,
 * final sample part count (1: not cut), 1 when the parts are dealt to the XCDs, workgroup slots of the balanced launch
 * (0: not balanced), 1 when the grid-wide prologue ran, curves per padded row of the shared weight table, its curve
 * groups, samples per part, 128-sample chunks per tile of the balanced launch, 1 when the odd column-waves of the
 * mirrored-pair kernel took every sample's table halves in the opposite order (only with PDC_GLS_LEAD=1 in the
 * environment; always 0 at S = 4 and where the pair kernel did not run), 1 when the mirrored-pair kernel took its
 * chunks' remainders from the array made once per call, 0 when every tile summed them in its table fill
 * (PDC_GLS_CHUNK_SUMS=0 in the environment, a launch whose stretches are not chunk-aligned, no pair kernel). */
int pdc_test_gls_last_dispatch(int64_t *out);
/* TEST HOOK (not for callers): whether the CALLING THREAD's last direct-sum scan ran the mirrored-pair kernel (K = 16 in
 * the two GLS modes; PDC_GLS_PAIR=0 in the environment keeps the plain kernel), per host thread like the record above.
 * out[2] = 1 when it did (0 otherwise), bytes of the per-sample offset table it read from the workspace. */
int pdc_test_gls_last_pair(int64_t *out);

/* ---- generalized Lomb-Scargle by the reference's own algorithm ("Tier F") ------
 * Same inputs/outputs as pdc_gls_scan, but the three _trig_sum calls (spectral.py:109-112) are
 * evaluated the way the reference evaluates them: Press-Rybicki extirpolation onto a grid of
 * nfft = 2^ceil(log2(5 nf)) points + inverse FFT (spectral.py:18-39), all on the device.  It takes
 * the reference's own scalars: fmin and df (spectral.py:88-96), not the np.arange grid.  Result:
 * the reference's `power` including its approximation error (O(N + nfft log nfft) work).
 * pdc_trig_sums_fft is the seam: _trig_sum(t, h, df, nf, fmin) itself. */
int64_t pdc_gls_fft_work_bytes(int64_t n, int64_t nf);
int pdc_gls_scan_fft(const double *t, const double *y, const double *dy, int64_t n,
                     double fmin, double df, int64_t nf, int fit_mean, int psd,
                     double *power_out, int device);
int pdc_gls_scan_fft_dev(int device, void *stream, const double *d_t, const double *d_y,
                         const double *d_dy, int64_t n, double fmin, double df, int64_t nf,
                         int fit_mean, int psd, double *d_power, void *work, int64_t work_bytes);
int pdc_trig_sums_fft(const double *t, const double *h, int64_t n, double df, int64_t nf,
                      double fmin, double *S_out, double *C_out, int device);
/* Batch of curves through the FFT path in one set of launches (layout and outputs as
 * pdc_gls_scan_batch): with shared_t != 0 this is GLS.bootstrap (spectral.py:140-152) evaluated by
 * the reference's own algorithm; the batch is processed in chunks sized to ~8 GiB of grids. */
int pdc_gls_scan_fft_batch(const double *t, const double *y, const double *dy,
                           const int64_t *offsets, int64_t n_curves, int shared_t,
                           double fmin, double df, int64_t nf, int fit_mean, int psd,
                           double *power_out, double *amax_out, int64_t *argmax_out, int device);

/* ---- peak picking on the device --------------------------------------------------
 * Highest local maximum of each of n_curves spectra of nf bins, as
 * FSeries.period_at_highest_peak finds it (core.py:952-955 -> find_peaks :283-317 ->
 * scipy.signal.find_peaks(prominence=0.0) -> NaN-aware max :202-220): strict local maxima, flat
 * tops resolved to their midpoint, first/last bin never a peak, NaN never part of one, ties ->
 * lowest index.  idx_out[b] = -1 (val NaN) when spectrum b has no peak.
 * pdc_gls_batch_highest_peak runs the batched periodogram and the reduction back to back so the
 * spectra never leave HBM (4096 x 5e4 bins = 1.6 GB stay on the device, 64 KB come back). */
int pdc_highest_peak(const double *power, int64_t n_curves, int64_t nf,
                     int64_t *idx_out, double *val_out, int device);
int pdc_highest_peak_dev(int device, void *stream, const double *d_power, int64_t n_curves,
                         int64_t nf, int64_t *d_idx, double *d_val);
int pdc_gls_batch_highest_peak(const double *t, const double *y, const double *dy,
                               const int64_t *offsets, int64_t n_curves, int shared_t,
                               double f0, double delta, int64_t nf, int fit_mean, int psd,
                               int64_t *idx_out, double *val_out, int device);

/* The k <= 1024 highest (by_prominence == 0: FSeries.psort_by_peak, core.py:944-946) or most prominent
 * (psort_by_prominence :948-950, period_at_highest_prominence :957-961) find_peaks() maxima of each
 * spectrum, found and ranked on the device: count[b] = number of maxima scipy.signal.find_peaks(x,
 * prominence=0.0) reports; idx/height/prominence are [n_curves][k], ranked descending, padded with
 * -1 / NaN; prominences follow scipy.signal.peak_prominences (wlen=None).  half_lo / half_hi
 * ([n_curves][k], -1 when absent; may be NULL) are the two sign changes of x - (x[idx] - key/2), key =
 * the ranking quantity, that FSeries.periods_at_half_max (core.py:963-978) looks up for
 * peak_order = rank + 1: half_hi = the last one inside x[:idx], half_lo = the first one of x[idx:]
 * as an absolute bin (np.where(np.diff(np.signbit(..))), core.py:362); the method returns
 * (period[half_lo], period[half_hi]).  Exactly equal keys rank the lower bin first (upstream's argsort()[::-1]
 * leaves ties to numpy's unstable sort: see INTEGRATION.md).
 * k > 128 runs as launches of 128 ranks (round 5: 64), each ranking what comes AFTER the launch before's last winner in that total
 * order (every launch sweeps the spectra again; measured for 4096 spectra of 5e4 bins: 64 / 128 / 256 ranks 1.1 / 1.5 / 3.0 ms by height, 1.8 / 2.7 / 6.7 ms by prominence - profiles/r06_peaks_timing.txt); it needs idx_out
 * and the ranking key's output (height_out, or prominence_out).  The host methods of FSeries serve any k.
 * pdc_gls_batch_peaks runs the batched periodogram first; the spectra never leave HBM. */
int pdc_peaks_topk(const double *power, int64_t n_curves, int64_t nf, int k, int by_prominence,
                   int64_t *count_out, int64_t *idx_out, double *height_out, double *prominence_out,
                   int64_t *half_lo_out, int64_t *half_hi_out, int device);
int pdc_peaks_topk_dev(int device, void *stream, const double *d_power, int64_t n_curves, int64_t nf,
                       int k, int by_prominence, int64_t *d_count, int64_t *d_idx, double *d_height,
                       double *d_prominence, int64_t *d_half_lo, int64_t *d_half_hi);
int pdc_gls_batch_peaks(const double *t, const double *y, const double *dy, const int64_t *offsets,
                        int64_t n_curves, int shared_t, double f0, double delta, int64_t nf,
                        int fit_mean, int psd, int k, int by_prominence,
                        int64_t *count_out, int64_t *idx_out, double *height_out,
                        double *prominence_out, int64_t *half_lo_out, int64_t *half_hi_out, int device);

/* ---- batches of light curves on their OWN grids ("ragged" grids; GLS.batch) ----------------------
 * Replaces a survey's loop of GLS()(s) (spectral.py:88-132, each curve on the grid its own data give:
 * df = 1/(baseline n), fmin = df/2, fmax = 0.5/median_dt, :88-97) followed by period_at_highest_peak /
 * psort_by_* / periods_at_half_max on each result (core.py:944-978).
 * Curve b owns samples [offsets[b], offsets[b+1]) of t, y and dy (dy NULL: unit errors for every curve)
 * and the grid f0[b] + j*delta[b], j < nf_b = f_offsets[b+1] - f_offsets[b] (numpy's arange fill rule,
 * two roundings); its bins are power[f_offsets[b] .. f_offsets[b+1]).  Weights, centring and epilogue are
 * those of pdc_gls_scan per curve (bits may differ from it by rounding: another tile shape).
 * offsets[0] == f_offsets[0] == 0, both non-decreasing; f0, delta finite, delta > 0; the grid in tiles of
 * 1024 bins < 2^31 tiles.  An empty curve gives a NaN row (as pdc_gls_scan), an empty grid no bins
 * (amax NaN, argmax -1).
 * Curves are dealt to the `n_devices` listed device slots in contiguous groups balanced by
 * sum n_b nf_b (a device may be listed more than once); per-slot buffers and streams are kept between
 * calls (pdc_release frees them).  Each slot's share runs in groups of curves whose buffers fit
 * PDC_WORK_BUDGET_GB and the slot's share of free device memory: results are bit-identical whatever the
 * grouping; a budget too small for one curve is PDC_ERR_INVALID and the message names it.
 *
 * pdc_gls_scan_ragged: power_out [f_offsets[B]] and/or amax_out / argmax_out [B] (NaN-aware maximum and
 * its bin within the curve's row: Signal.amax / argmax, core.py:202-215), any of them NULL.
 *
 * pdc_gls_ragged_peaks: the peak table of pdc_gls_batch_peaks on every curve's own row: count[B];
 * idx / height / prominence / half_lo / half_hi [B][k] (k <= 1024), ranked and padded exactly as there,
 * bins relative to the row; power_out as above, or NULL (the spectra then never leave HBM).  The scan
 * writes a pitched copy [B][nf_max] whose tail bins [nf_b, nf_max) are NaN and pdc_peaks_topk_dev runs
 * on it.  The pad keeps scipy's answers for the unpadded row: NaN compares false, so the last real bin
 * still cannot be a peak and a flat top running into the pad is still none; the right-hand prominence
 * walk stops at the pad as at the row's end; heights, counts and ranks are unchanged.  The one
 * artefact is a sign flip of the pair (nf_b - 1, nf_b), which the half-maximum walk may report:
 * half_lo >= nf_b - 1 is therefore returned as -1 (periods_at_half_max, core.py:975-977, looks only at
 * pairs inside the row).
 *
 * pdc_gls_ragged_work_bytes / pdc_gls_scan_ragged_dev: ONE launch sequence on `device` / `stream`, no
 * grouping: t, y, dy on the device; offsets, f0, delta, f_offsets on the HOST (the tile tables are built
 * from them; the entry waits for their upload, and so for the stream's earlier work, before it returns -
 * the launches themselves are not waited for).  d_power [f_offsets[B]], d_pitched [B][pitch] (its pad is
 * the caller's), d_amax / d_argmax [B]: any may be NULL, not all.  work_bytes >=
 * pdc_gls_ragged_work_bytes(offsets[B], B, f_offsets[B], 0, 0); k > 0 and nf_max size the group
 * workspace of the peak entry (+ the pitched copy and the [B][k] table). */
int pdc_gls_scan_ragged(const double *t, const double *y, const double *dy, const int64_t *offsets,
                        int64_t n_curves, const double *f0, const double *delta, const int64_t *f_offsets,
                        int fit_mean, int psd, double *power_out, double *amax_out, int64_t *argmax_out,
                        const int *devices, int n_devices);
int pdc_gls_ragged_peaks(const double *t, const double *y, const double *dy, const int64_t *offsets,
                         int64_t n_curves, const double *f0, const double *delta, const int64_t *f_offsets,
                         int fit_mean, int psd, int k, int by_prominence, int64_t *count_out,
                         int64_t *idx_out, double *height_out, double *prominence_out,
                         int64_t *half_lo_out, int64_t *half_hi_out, double *power_out,
                         const int *devices, int n_devices);
int64_t pdc_gls_ragged_work_bytes(int64_t n_total, int64_t n_curves, int64_t nf_total, int64_t nf_max, int k);
int pdc_gls_scan_ragged_dev(int device, void *stream, const double *d_t, const double *d_y,
                            const double *d_dy, const int64_t *offsets, int64_t n_curves,
                            const double *f0, const double *delta, const int64_t *f_offsets,
                            int fit_mean, int psd, double *d_power, double *d_pitched, int64_t pitch,
                            double *d_amax, int64_t *d_argmax, void *work, int64_t work_bytes);

/* ---- PDM / AoV / conditional entropy over curves on their OWN period grids (PDM.batch ...) ---------
 * Replaces a survey's loop of PDM()(s), AOV()(s) or ConditionalEntropy()(s) (each curve on the grid its own
 * data give: np.linspace(p_min, p_max, count), p_min = 2 median_dt, p_max = oversample baseline,
 * phase.py:167-180) followed by find_dips / find_peaks / periods_at_half_max on each result.
 * kind: 0 PDM theta over nb x nc covers (sigma[b] = np.var(values_b, ddof=1) is required), 1 AoV over nb
 * phase bins (nc ignored), 2 conditional entropy over nb phase x nc magnitude bins (x = the magnitude bin
 * of every sample, 0 .. nc-1; a curve may have at most 65 280 samples: one workgroup bins it in 16-bit cells).
 * Curve b owns samples [offsets[b], offsets[b+1]) of t and x and the trial periods
 * linspace(start[b], stop[b], P_b), P_b = p_offsets[b+1] - p_offsets[b], rebuilt on the device with numpy's
 * rule: j*step[b] + start[b] (two roundings), exactly stop[b] at j = P_b - 1 > 0; for P_b == 1 pass
 * step = stop - start.  significant[b] (or NULL: none) turns on the sub-harmonic averaging of PDM's
 * do_subharmonic with that threshold (1 - 11 / N**0.8, computed by the caller); it needs P_b >= 2.
 * Values come back in period order, out[p_offsets[b] + j].  For a curve of < 8192 samples and < 131 072
 * periods they are bit-identical to pdc_pdm_scan / pdc_aov_scan / pdc_cond_entropy_scan on that curve;
 * longer curves agree to rounding (the single call splits them otherwise).
 * Devices, groups and budget as for pdc_gls_scan_ragged: curves are dealt to the `n_devices` listed slots
 * in contiguous groups balanced by sum n_b P_b, per-slot buffers are kept (pdc_release frees them),
 * groups fit PDC_WORK_BUDGET_GB and free memory, and results are bit-identical for any grouping.
 *
 * pdc_phase_ragged_peaks: the [B][k] peak table (k <= 1024) of pdc_gls_ragged_peaks on every curve's row in
 * FSeries order (ascending frequency 1/p: index j' = P_b - 1 - j when stop[b] > start[b], j' = j otherwise; that is
 * FSeries' order for grids whose periods share one sign and have distinct reciprocals): of its DIPS for PDM and
 * conditional entropy (find_dips, ranked deepest first; height_out holds the statistic itself, the half-maximum
 * crossings are those of the negated row), of its peaks for AoV.  out may be NULL: the rows stay in HBM.
 *
 * pdc_phase_ragged_work_bytes / pdc_phase_scan_ragged_dev: ONE launch sequence on `device` / `stream`, no
 * grouping: t, x on the device; offsets ... significant on the HOST (the entry waits for their upload before
 * it returns, not for the launches).  d_out [p_offsets[B]] and/or d_pitched [B][pitch] (FSeries order, negated
 * for the dip kinds; its pad is the caller's).  work_bytes >= pdc_phase_ragged_work_bytes(B, p_offsets[B], 0, 0);
 * p_max > 0 and k > 0 size the group workspace of the peak entry (+ the pitched copy and the [B][k] table). */
int pdc_phase_scan_ragged(int kind, const double *t, const double *x, const int64_t *offsets,
                          int64_t n_curves, const double *start, const double *step, const double *stop,
                          const int64_t *p_offsets, const double *sigma, const double *significant, int nb,
                          int nc, double *out, const int *devices, int n_devices);
int pdc_phase_ragged_peaks(int kind, const double *t, const double *x, const int64_t *offsets,
                           int64_t n_curves, const double *start, const double *step, const double *stop,
                           const int64_t *p_offsets, const double *sigma, const double *significant, int nb,
                           int nc, int k, int by_prominence, int64_t *count_out, int64_t *idx_out,
                           double *height_out, double *prominence_out, int64_t *half_lo_out,
                           int64_t *half_hi_out, double *out, const int *devices, int n_devices);
int64_t pdc_phase_ragged_work_bytes(int64_t n_curves, int64_t p_total, int64_t p_max, int k);
/* TEST HOOK (not for callers): how many groups of curves the last pdc_phase_scan_ragged / pdc_phase_ragged_peaks call
 * of this process ran, summed over its device slots (1 per busy slot when everything fit the budget). */
int pdc_test_phase_ragged_groups(int64_t *groups);
int pdc_phase_scan_ragged_dev(int kind, int device, void *stream, const double *d_t, const double *d_x,
                              const int64_t *offsets, int64_t n_curves, const double *start,
                              const double *step, const double *stop, const int64_t *p_offsets,
                              const double *sigma, const double *significant, int nb, int nc,
                              double *d_out, double *d_pitched, int64_t pitch, void *work,
                              int64_t work_bytes);

/* ---- StringLength over curves on their OWN period grids (StringLength.batch) ------------------------
 * Replaces a survey's loop of StringLength()(s) (each curve on 1 / np.linspace(n_periods * s, s, n_periods),
 * s = dphi / baseline, phase.py:67-68) followed by find_dips / periods_at_half_max on each result.
 * Curve b owns samples [offsets[b], offsets[b+1]) of t and m (m already scaled to [-0.25, 0.25] by the caller)
 * and the trial periods 1 / linspace(start[b], stop[b], P_b), P_b = p_offsets[b+1] - p_offsets[b]: a FREQUENCY
 * linspace rebuilt on the device with numpy's rule (j*step[b] + start[b], two roundings, exactly stop[b] at
 * j = P_b - 1 > 0; for P_b == 1 pass step = stop - start), then an IEEE reciprocal.  Lengths come back in period
 * order, out[p_offsets[b] + j], bit-identical to pdc_stringlength_scan on that curve and those periods: curves of
 * 1 .. 26 048 samples run the single call's one-cycle pre-pass and two-workgroups-per-CU kernel as ragged
 * launches (the same instance, the same per-period code), the periods that kernel marks and every other curve
 * run the single call's own kernels on the curve's slices.
 * Devices, groups and budget as for pdc_phase_scan_ragged (bit-identical for any grouping).
 *
 * pdc_stringlength_ragged_peaks: the [B][k] peak table (k <= 1024) of the DIPS of every curve's row in FSeries
 * order (ascending frequency: j' = P_b - 1 - j when start[b] > stop[b], j' = j otherwise), as find_dips ranks
 * them; height_out holds the lengths themselves, the half-maximum crossings are those of the negated row.
 * out may be NULL: the rows stay in HBM.
 *
 * pdc_stringlength_ragged_work_bytes / pdc_stringlength_scan_ragged_dev: ONE group on `device` / `stream`: t, m
 * on the device; offsets ... p_offsets on the HOST.  d_out [p_offsets[B]] and/or d_pitched [B][pitch] (FSeries
 * order, negated; its pad is the caller's).  The entry waits for the stream once, to read how many periods the
 * ragged kernel left to the one-workgroup kernel.  work_bytes >= pdc_stringlength_ragged_work_bytes(offsets,
 * p_offsets, B). */
int pdc_stringlength_scan_ragged(const double *t, const double *m, const int64_t *offsets, int64_t n_curves,
                                 const double *start, const double *step, const double *stop,
                                 const int64_t *p_offsets, double *out, const int *devices, int n_devices);
int pdc_stringlength_ragged_peaks(const double *t, const double *m, const int64_t *offsets, int64_t n_curves,
                                  const double *start, const double *step, const double *stop,
                                  const int64_t *p_offsets, int k, int by_prominence, int64_t *count_out,
                                  int64_t *idx_out, double *height_out, double *prominence_out,
                                  int64_t *half_lo_out, int64_t *half_hi_out, double *out, const int *devices,
                                  int n_devices);
int64_t pdc_stringlength_ragged_work_bytes(const int64_t *offsets, const int64_t *p_offsets, int64_t n_curves);
/* TEST HOOK (not for callers): of the last pdc_stringlength_scan_ragged / pdc_stringlength_ragged_peaks call of this
 * process, the groups it ran (summed over its device slots), the (curve, period) pairs the ragged kernel marked for
 * the one-workgroup kernel, and the curves that took the single call's own route (more than 26 048 samples ...). */
int pdc_test_sl_ragged_stats(int64_t *groups, int64_t *marked, int64_t *long_curves);
int pdc_stringlength_scan_ragged_dev(int device, void *stream, const double *d_t, const double *d_m,
                                     const int64_t *offsets, int64_t n_curves, const double *start,
                                     const double *step, const double *stop, const int64_t *p_offsets,
                                     double *d_out, double *d_pitched, int64_t pitch, void *work,
                                     int64_t work_bytes);

/* ---- Phase Dispersion Minimization -----------------------------------------------------------
 * Replaces pool.map(PDM._pdm, periods) (phase.py:128-149, 185-187): theta_out[p] for every trial
 * period, bins phi in [k/m0, (k+nc)/m0) U [0, (k+nc-m0)/m0), m0 = nb*nc, phi = (t/period) % 1
 * with IEEE division and Python modulo; sigma = var(x, ddof=1) is the caller's (phase.py:165). */
int pdc_pdm_scan(const double *t, const double *x, int64_t n,
                 const double *periods, int64_t n_periods, int nb, int nc, double sigma,
                 double *theta_out, int device);
int pdc_pdm_scan_dev(int device, void *stream, const double *d_t, const double *d_x, int64_t n,
                     const double *d_periods, int64_t n_periods, int nb, int nc, double sigma,
                     double *d_theta);

/* The two period searches phase.py:11-15 lists as TODO, on the PDM binning kernel (same phase bins
 * [k/r, (k+1)/r) against the doubles k/r as phase.py:137, same exact phases, one thread per trial
 * period; only the epilogue differs).  The reference has no implementation: parity is pinned to the
 * published formulas, restated in oracle/scan_oracle.py.
 *   Analysis of Variance (Schwarzenberg-Czerny 1989, MNRAS 241, 153, eq. 1-3) over n_bins phase bins:
 *     theta_out[p] = [sum_i n_i (xbar_i - xbar)^2 / (r - 1)] / [sum_i sum_j (x_ij - xbar_i)^2 / (n - r)]
 *   Conditional entropy (Graham et al. 2013, MNRAS 434, 2629, eq. 1) over n_phase x n_mag cells:
 *     entropy_out[p] = sum_ij p(m_j, phi_i) ln(p(phi_i) / p(m_j, phi_i));  mag_bin[i] is the magnitude
 *     bin (0 .. n_mag-1, stored as a double) of sample i, (n_phase + 1) * n_mag <= 191. */
int pdc_aov_scan(const double *t, const double *x, int64_t n, const double *periods, int64_t n_periods,
                 int n_bins, double *theta_out, int device);
int pdc_aov_scan_dev(int device, void *stream, const double *d_t, const double *d_x, int64_t n,
                     const double *d_periods, int64_t n_periods, int n_bins, double *d_theta);
int pdc_cond_entropy_scan(const double *t, const double *mag_bin, int64_t n, const double *periods,
                          int64_t n_periods, int n_phase, int n_mag, double *entropy_out, int device);
int pdc_cond_entropy_scan_dev(int device, void *stream, const double *d_t, const double *d_mag_bin,
                              int64_t n, const double *d_periods, int64_t n_periods, int n_phase,
                              int n_mag, double *d_entropy);

/* The third TODO of phase.py:11-15: the Gregory-Loredo method (Gregory & Loredo 1992, ApJ 398, 146) for
 * ARRIVAL TIMES t (the signal's values are not used): for every trial period the log of
 *     S_m(w) = (1 / 2 pi) Int dphi  m^N n_1! ... n_m! / N!      (their eq. 5.13-5.14 marginalised over the offset;
 * the integrand of the odds ratio O_m1, eq. 5.28), n_j = counts in m phase bins, the offset integral as the
 * mean over n_offsets equally spaced shifts of the bin boundaries; m * n_offsets <= 190.  Counts-only histogram
 * on the PDM binning kernel (same exact phases, same edges f / F).  The reference has no implementation:
 * parity is pinned to the published formula, restated in oracle/scan_oracle.py. */
int pdc_gl_scan(const double *t, int64_t n, const double *periods, int64_t n_periods, int m, int n_offsets,
                double *log_s_out, int device);
int pdc_gl_scan_dev(int device, void *stream, const double *d_t, int64_t n, const double *d_periods,
                    int64_t n_periods, int m, int n_offsets, double *d_log_s);

/* The phase-fold statistics behind one device-resident entry with an EXPLICIT workspace (nothing is
 * cached per stream, nothing is allocated): kind 0 = PDM theta (nb, nc, sigma as pdc_pdm_scan), 1 = AoV
 * (nb = n_bins), 2 = conditional entropy (nb = n_phase, nc = n_mag, v = magnitude bins), 3 = StringLength
 * (v = m; nb, nc, sigma ignored), 4 = Gregory-Loredo (v may be NULL; nb = m * n_offsets, nc = m).  `work` holds at least pdc_phase_work_bytes(kind, n, n_periods, nb, nc)
 * bytes (0 for most PDM shapes: only short period grids over long curves split the samples and need
 * scratch for partial histograms). */
int64_t pdc_phase_work_bytes(int kind, int64_t n, int64_t n_periods, int nb, int nc);
int pdc_phase_scan_dev(int kind, int device, void *stream, const double *d_t, const double *d_v, int64_t n,
                       const double *d_periods, int64_t n_periods, int nb, int nc, double sigma,
                       double *d_out, void *work, int64_t work_bytes);
/* TEST HOOKS (not for callers): the route of the phase-binning scans (kinds 0, 1, 2 and 4; every entry above ends in one
 * dispatcher, and one host function chooses its route).  pdc_test_phase_shape gives the route a scan of that shape would
 * take in this process - PDC_PDM_SPLIT and PDC_PDM_NZ are honoured as the launcher honours them - and touches no device;
 * pdc_test_phase_last_dispatch gives the route of the last launch in this process, written on the host just before the
 * kernels go out (all zeros before the first).  out[11] = kind, 1 in split mode (sample statistics from two launches of
 * their own, the samples cut in slices on grid.y, a finishing launch), threads per workgroup of the scan kernel, waves
 * that share one group of 64 trial periods, trial periods per workgroup, workgroups in x, sample slices (1: not cut),
 * samples per slice (0 when unsplit), partial sums of the sample statistics (0 when unsplit), dynamic LDS bytes of the
 * scan kernel, dynamic LDS bytes of the finishing kernel (0 when unsplit). */
int pdc_test_phase_shape(int kind, int64_t n, int64_t n_periods, int nb, int nc, int64_t *out);
int pdc_test_phase_last_dispatch(int64_t *out);

/* The period grid cut into contiguous slabs over `n_devices` GPUs of this node (one process, one
 * stream per slab; a device may be listed more than once).  Replaces the multiprocessing.Pool
 * fan-out of phase.py:182-186; trial periods are independent, so there is no exchange step.  The
 * per-slot buffers, streams and page-locked staging are kept between calls, keyed by the device list
 * (pdc_release() frees them): a second call of the same size allocates nothing. */
int pdc_pdm_scan_multi(const double *t, const double *x, int64_t n,
                       const double *periods, int64_t n_periods, int nb, int nc, double sigma,
                       double *theta_out, const int *devices, int n_devices);
int pdc_aov_scan_multi(const double *t, const double *x, int64_t n, const double *periods, int64_t n_periods,
                       int n_bins, double *theta_out, const int *devices, int n_devices);
int pdc_cond_entropy_scan_multi(const double *t, const double *mag_bin, int64_t n, const double *periods,
                                int64_t n_periods, int n_phase, int n_mag, double *entropy_out,
                                const int *devices, int n_devices);
int pdc_gl_scan_multi(const double *t, int64_t n, const double *periods, int64_t n_periods, int m, int n_offsets,
                      double *log_s_out, const int *devices, int n_devices);

/* The same fan-out as a persistent plan for callers that scan repeatedly or want the samples resident
 * (bench.py, a survey loop): replaces Pool(cores).map of phase.py:69-70,185-186.
 *   create    streams, events and (for n_max / n_periods_max > 0) buffers per slot; a device may repeat
 *   upload    replicate (t, v) on every slot through page-locked staging (async)
 *   scan      kind as pdc_phase_scan_dev; enqueue per slot: its slab of `periods` H2D, the scan, its slab
 *             of results D2H into page-locked memory; returns without waiting
 *   wait / download   drain; copy the n_periods results of the latest scan to `out`
 *   kernel_ms HIP-event time of the latest scan's kernels, the slowest slot */
int pdc_phase_plan_create(const int *devices, int n_devices, int64_t n_max, int64_t n_periods_max, void **plan);
int pdc_phase_plan_upload(void *plan, const double *t, const double *v, int64_t n);
int pdc_phase_plan_scan(void *plan, int kind, const double *periods, int64_t n_periods, int nb, int nc,
                        double sigma);
int pdc_phase_plan_wait(void *plan);
int pdc_phase_plan_download(void *plan, double *out, int64_t n_periods);
int pdc_phase_plan_kernel_ms(void *plan, float *ms);
int pdc_phase_plan_destroy(void *plan);

/* ---- String Length -----------------------------------------------------------------------------
 * Replaces pool.map(StringLength._stringlength, periods) (phase.py:45-51, 69-70) including the
 * fold ((t - 0)/period) % 1 (core.py:543-544) and the stable sort by phase of the TSeries
 * constructor (core.py:473-477); the closing segment is not phase-wrapped. `m` is the scaled
 * signal of phase.py:65-66.  Samples may come in any order (equal phases keep the order given, as the
 * stable sort does).  Time-ordered samples - what a TSeries holds - are what the kernels are built around: the
 * periods that outlast them need no sort at all (at any size), and from 262 144 samples on a bin's samples are
 * fetched as slices of t / m.  Samples in ANOTHER order, from 262 144 on, are ordered by time on the device first
 * (round 5; a stable radix sort of (t, m), once per call, 0.4 ms at N = 2e6 - csrc/timesort.inc) and take the same
 * kernels: the result is the one for TSeries(t, m), i.e. samples that share a time stamp keep the caller's order, and
 * samples that share a phase at some period without sharing a time stamp are taken in time order there (up to
 * round 4 such samples went through the partition lists and the general kernel - N = 2e6 x 512 periods: 118 ms;
 * now 13.7 against 13.3 ms in order; profiles/r05_sl_shapes.txt).  Non-finite or |t| beyond 1e+-150: no time sort,
 * the lists as before.  Below 262 144 samples the kernels sort any order by phase directly: the periods which outlast
 * the samples are then sorted like any other, and two samples that share a phase WITHOUT sharing a time stamp keep the
 * caller's order there (above: the time order, as the reference's TSeries would have it - core.py:473-477).
 * The `_dev` entry cannot look at the samples from the host: from 262 144 samples on it ALWAYS enqueues the time sort's
 * intake (a 16 n-byte copy of (t, m) and 25 launches that return at once when the device finds the samples in order:
 * 3.19 against 3.15 ms at N = 1e6 x 256 periods) and sizes its workspace for the bin lists; the host entry and the
 * phase plan hold the arrays, check the order and the periods first, and skip both.
 * Workspace (both forms): PDC_WORK_BUDGET_GB=<float> caps it - pdc_stringlength_work_bytes and the scan read the same
 * value -, the host entry also fits it to the device's free memory; smaller batches, same bits; a budget that not
 * even one period fits in is an error whose text names it. */
int pdc_stringlength_scan(const double *t, const double *m, int64_t n,
                          const double *periods, int64_t n_periods,
                          double *ell_out, int device);
int64_t pdc_stringlength_work_bytes(int64_t n, int64_t n_periods);
int pdc_stringlength_scan_dev(int device, void *stream, const double *d_t, const double *d_m,
                              int64_t n, const double *d_periods, int64_t n_periods,
                              double *d_ell, void *work, int64_t work_bytes);

/* As pdc_pdm_scan_multi, for phase.py:69-70. */
int pdc_stringlength_scan_multi(const double *t, const double *m, int64_t n,
                                const double *periods, int64_t n_periods,
                                double *ell_out, const int *devices, int n_devices);

/* Supersmoother period search - the reference names it in one line ("TODO: check out Supersmoother (Reimann
 * 1994)", spectral.py:8) and has no code.  Built from the published algorithm: per trial period the curve is
 * folded and sorted by phase exactly as for StringLength (core.py:543-544, 473-477), Friedman's variable span
 * smoother (Friedman 1984, SLAC PUB-3477: `supsmu` with periodic abscissae, spans 0.05 / 0.2 / 0.5, bass
 * control `alpha` in [0, 10], 0 = off) is fitted to (phase, y), and stat_out[p] = the mean absolute residual
 * about the fit (Reimann 1994): minimal at the period.  Needs n >= 5.  Parity unpinned by the reference; the
 * oracle restates the published Fortran (oracle/scan_oracle.py: supersmoother*) in exact-to-rounding window sums -
 * for phases crowded into a sliver of the cycle (periods thousands of baselines long) the Fortran's own
 * double-precision updating formulas lose the windows' variances; the device follows the oracle there, not them.
 * Samples may come in any order, as for pdc_stringlength_scan (from 262 144 samples on they are ordered by time on the
 * device first).  The device form takes resident inputs and a workspace of pdc_supersmoother_work_bytes(n, n_periods)
 * bytes; PDC_WORK_BUDGET_GB caps it as for pdc_stringlength_scan (smaller sub-batches and pools: the statistic agrees
 * to 1e-12 - the tiles' segment count follows the sub-batch -, a budget nothing fits in is an error that names it). */
int pdc_supersmoother_scan(const double *t, const double *y, int64_t n, const double *periods, int64_t n_periods,
                           double alpha, double *stat_out, int device);
int pdc_supersmoother_scan_multi(const double *t, const double *y, int64_t n, const double *periods, int64_t n_periods,
                                 double alpha, double *stat_out, const int *devices, int n_devices);
int64_t pdc_supersmoother_work_bytes(int64_t n, int64_t n_periods);
int pdc_supersmoother_scan_dev(int device, void *stream, const double *d_t, const double *d_y, int64_t n,
                               const double *d_periods, int64_t n_periods, double alpha, double *d_stat, void *work,
                               int64_t work_bytes);
/* TEST HOOK (not for callers): the launch shape the device entry takes for (n, n_periods) under PDC_WORK_BUDGET_GB and
 * the PDC_SS_* switches; out[10] = periods per batch, per sub-batch of the tiled smoother (0: not tiled), segments of
 * the first two / last two sweeps, workgroups of the generic smoother / of the fallback sort, tiled, streamed sort,
 * LDS sort, workspace bytes.  No device is touched. */
int pdc_test_ss_shape(int64_t n, int64_t n_periods, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* PERIODICITY_HIP_H */
