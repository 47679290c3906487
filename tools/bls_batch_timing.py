"""Timing of BLS.batch (ragged period grids, bls_ragged.hip) on a survey-shaped batch (developer tool).

The batch: the survey of tools/gls_batch_timing.py (4096 curves, N log-uniform in 300 .. 5000, baselines 100 .. 3000
days, jittered cadences, individual errors), searched with BLS's defaults (200 bins, boxes of 2 .. 20 bins, 1000 periods
per curve, min_points = 5).  Reports, with the inputs in HBM, HIP events, the median of 7 runs after 2 warm-ups:
  (a) the batch through pdc_bls_scan_ragged_dev (metadata upload + prologue + binning / search + best box), rows and
      best written, and with the best box only;
  (b) the same curves as a loop of pdc_bls_scan_dev - before the batch, the only way - in the same run, and whether the
      two give the same bits;
  (c) the single call at 1e5 samples x 1000 periods (tools/bls_timing.py's curve) as the rate yardstick;
  (d) wall time of BLS().batch(cat, errs, want_power=False) against a loop of BLS()(s, e) reading .best.
``python tools/bls_batch_timing.py > profiles/<round>_bls_batch_timing.txt``   (--batch-only: one BLS().batch call of the
survey, want_power=False - the run to put under a kernel trace)
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import bls_oracle as bo  # noqa: E402
from gls_batch_timing import survey  # noqa: E402
from periodicity_amd import _cabi  # noqa: E402
from periodicity_amd.phase import BLS, _linspace_steps, _pdm_limits  # noqa: E402

N_BINS, LEN_MIN, LEN_MAX, MIN_POINTS, N_PERIODS = 200, 2, 20, 5, 1000     # the defaults of periodicity_amd.phase.BLS
REPS, WARM = 7, 2


def main():
    lib, dev, DB, ptr = _cabi.lib(), 0, _cabi.DeviceBuffer, _cabi._ptr
    print("device:", _cabi.device_info(dev))
    print(f"# n_bins={N_BINS} boxes of {LEN_MIN}..{LEN_MAX} bins, min_points={MIN_POINTS}, individual weights, both signs, "
          f"{N_PERIODS} periods per curve = linspace(2 median dt, baseline, {N_PERIODS}); device-side time (HIP events), median "
          f"of {REPS} runs after {WARM} warm-up runs, inputs in HBM; MEASURED on this device in this run")
    sigs, errs = survey()
    B = len(sigs)
    sizes = np.array([len(s) for s in sigs], dtype=np.int64)
    offsets = np.zeros(B + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(sizes)
    t = np.concatenate([s.time for s in sigs])
    y = np.concatenate([s.values for s in sigs])
    dy = np.concatenate(errs)
    lim = [_pdm_limits(s, None, None, N_PERIODS, 1) for s in sigs]
    start, stop = np.array([x[0] for x in lim]), np.array([x[1] for x in lim])
    count = np.array([x[2] for x in lim], dtype=np.int64)
    step = _linspace_steps(start, stop, count)
    poff = np.zeros(B + 1, dtype=np.int64)
    poff[1:] = np.cumsum(count)
    P, n_total = int(poff[-1]), int(offsets[-1])
    pairs = float(np.sum(sizes * count))
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(dev, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, dev, sp.value)
    bt, by, be = DB.from_array(t, dev), DB.from_array(y, dev), DB.from_array(dy, dev)
    wb = lib.pdc_bls_ragged_work_bytes(B, n_total, P, 0, 0)
    work = DB(wb, dev)
    rows = [DB(P * 8, dev), DB(P * 8, dev), DB(P * 4, dev), DB(P * 4, dev)]
    best = [DB(B * 8, dev), DB(B * 8, dev), DB(B * 8, dev), DB(B * 4, dev), DB(B * 4, dev)]
    kinds = (np.float64, np.float64, np.int32, np.int32)

    def batch(with_rows):
        outs = [r.ptr if with_rows else None for r in rows] + [b.ptr for b in best]
        _cabi.check(lib.pdc_bls_scan_ragged_dev(dev, sp.value, bt.ptr, by.ptr, be.ptr, ptr(offsets), B, ptr(start), ptr(step),
                                                ptr(stop), ptr(poff), N_BINS, LEN_MIN, LEN_MAX, MIN_POINTS, 0, *outs, None, 0,
                                                work.ptr, wb))

    shape = f"B={B} N={n_total} ({sizes.min()}..{sizes.max()}) P={P} (sample, period) pairs={pairs:.3e}"
    ms_full = tm.ms(lambda: batch(True), reps=REPS, warm=WARM)
    _cabi.check(lib.pdc_stream_sync(dev, sp.value))
    got = [r.to_array(k, P) for r, k in zip(rows, kinds)]
    got_index = best[0].to_array(np.int64, B)
    print(f"(a) batch, pdc_bls_scan_ragged_dev, rows + best box: {shape}: {ms_full:.2f} ms, {pairs / ms_full / 1e6:.2f} "
          f"G(sample, period)/s")
    ms_best = tm.ms(lambda: batch(False), reps=REPS, warm=WARM)
    _cabi.check(lib.pdc_stream_sync(dev, sp.value))
    same_best = np.array_equal(got_index, best[0].to_array(np.int64, B))
    print(f"(a) batch, best box only (rows in the workspace): {ms_best:.2f} ms, {pairs / ms_best / 1e6:.2f} G(sample, period)/s; "
          f"{'same best index' if same_best else 'best index DIFFERS'}")

    # (b) the loop of single calls on the same curves: the period grids uploaded once, outside the timing
    periods = np.concatenate([np.linspace(start[b], stop[b], count[b]) for b in range(B)])
    bp = DB.from_array(periods, dev)
    loop_rows = [DB(P * 8, dev), DB(P * 8, dev), DB(P * 4, dev), DB(P * 4, dev)]
    calls = []
    for b in range(B):
        o, po = int(offsets[b]), int(poff[b])
        calls.append((bt.ptr + 8 * o, by.ptr + 8 * o, be.ptr + 8 * o, int(sizes[b]), bp.ptr + 8 * po, int(count[b]),
                      loop_rows[0].ptr + 8 * po, loop_rows[1].ptr + 8 * po, loop_rows[2].ptr + 4 * po, loop_rows[3].ptr + 4 * po))

    def loop():
        for a_t, a_y, a_e, n, a_p, n_p, o_pow, o_dep, o_st, o_box in calls:
            _cabi.check(lib.pdc_bls_scan_dev(dev, sp.value, a_t, a_y, a_e, n, a_p, n_p, N_BINS, LEN_MIN, LEN_MAX, MIN_POINTS, 0, 0,
                                             o_pow, o_dep, o_st, o_box))

    ms_loop = tm.ms(loop, reps=REPS, warm=WARM)
    _cabi.check(lib.pdc_stream_sync(dev, sp.value))
    same = all(np.array_equal(a, r.to_array(k, P), equal_nan=True) for a, r, k in zip(got, loop_rows, kinds))
    power = got[0]
    want_index = np.array([np.nanargmax(power[poff[b]:poff[b + 1]]) if np.any(~np.isnan(power[poff[b]:poff[b + 1]])) else -1
                           for b in range(B)])
    print(f"(b) loop of {B} pdc_bls_scan_dev calls, device-resident, no result copies, no synchronisation: {ms_loop:.2f} ms, "
          f"{pairs / ms_loop / 1e6:.2f} G(sample, period)/s; batch / loop = {ms_full / ms_loop:.3f} (rows + best), "
          f"{ms_best / ms_loop:.3f} (best only); rows {'bit-identical' if same else 'DIFFER'}; best index "
          f"{'== nanargmax on every curve' if np.array_equal(want_index, got_index) else 'DIFFERS from nanargmax'}")
    for b in rows + best + loop_rows + [bp, bt, by, be, work]:
        b.free()

    # (c) the rate yardstick: the single call at 1e5 samples x 1000 periods
    n, n_periods = 100_000, 1000
    t1, y1, e1 = bo.curve(n, 31)
    p1 = np.linspace(2 * np.median(np.diff(t1)), t1[-1] - t1[0], n_periods)
    b1 = [DB.from_array(a, dev) for a in (t1, y1, e1, p1)]
    o1 = [DB(n_periods * 8, dev), DB(n_periods * 8, dev), DB(n_periods * 4, dev), DB(n_periods * 4, dev)]
    ms1 = tm.ms(lambda: _cabi.check(lib.pdc_bls_scan_dev(dev, sp.value, b1[0].ptr, b1[1].ptr, b1[2].ptr, n, b1[3].ptr, n_periods,
                                                         N_BINS, LEN_MIN, LEN_MAX, MIN_POINTS, 0, 0, *[o.ptr for o in o1])),
                reps=REPS, warm=WARM)
    rate1 = n * n_periods / ms1 / 1e6
    print(f"(c) single call, N={n} x {n_periods} periods (slices chosen from the shape): {ms1:.3f} ms, {rate1:.2f} G(sample, "
          f"period)/s; the batch runs at {pairs / ms_full / 1e6 / rate1:.3f} of that rate, the loop at "
          f"{pairs / ms_loop / 1e6 / rate1:.3f}")
    for b in b1 + o1:
        b.free()
    _cabi.check(lib.pdc_stream_destroy(dev, sp.value))

    # (d) wall clock through the public API
    BLS().batch(sigs[:64], errs[:64], want_power=False)   # (warm: library, slots, LDS attributes)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = BLS().batch(sigs, errs, want_power=False)
        walls.append(time.perf_counter() - t0)
    w_batch = float(np.median(walls))
    scan = BLS()
    scan(sigs[0], errs[0])
    t0 = time.perf_counter()
    loop_best = []
    for s, e in zip(sigs, errs):
        scan(s, e)
        loop_best.append(scan.best["period"])
    w_loop = time.perf_counter() - t0
    same = np.mean(np.asarray(loop_best) == res.best["period"])
    print(f"(d) BLS().batch({B} curves, errs, want_power=False): {w_batch * 1e3:.1f} ms wall (median of 3); loop of BLS()(s, e) "
          f"reading .best: {w_loop * 1e3:.0f} ms; {w_loop / w_batch:.1f}x; same best period on {same * 100:.2f} % of the curves")


if __name__ == "__main__":
    if "--batch-only" in sys.argv:
        cat, cat_errs = survey()
        out = BLS().batch(cat, cat_errs, want_power=False)
        print(f"BLS().batch: {len(out)} curves, best period of curve 0: {out.best['period'][0]:.6g}")
    else:
        main()
