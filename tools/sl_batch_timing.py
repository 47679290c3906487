"""Timing of StringLength.batch (ragged period grids, sl_ragged.inc) on a survey-shaped batch (developer tool).

The batch: the survey of tools/gls_batch_timing.py (4096 curves, N log-uniform in 300 .. 5000, baselines 100 .. 3000
days, jittered cadences), scanned with StringLength's defaults (dphi = 0.1, 1000 periods per curve).  Reports, with the
inputs in HBM:
  (a) the ragged scan (periods, prologue, one-cycle pre-pass, the duo instances, the host read of the marked counts;
      event-timed, median of 5) and its pair rate, next to the single call's (pdc_stringlength_scan_dev) at a matching
      uniform shape, N = 2000 x 1e5 periods (the <16, 256, 512> instance), measured in the same run;
  (c) wall time of StringLength().batch(..., peaks=1, want_power=False) against a loop of StringLength()(s) +
      find_dips, with its host (Python) / library split.
Usage: python tools/sl_batch_timing.py [--scan-only | --batch-only]   (--batch-only: one StringLength().batch call of
the survey, peaks=1, want_power=False - the run to put under a kernel trace)
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from gls_batch_timing import survey  # noqa: E402
from periodicity_amd import _cabi, phase  # noqa: E402
from periodicity_amd.phase import StringLength, _quarter_scaled, _string_grid, _string_periods  # noqa: E402


def main(scan_only):
    lib, dev, DB = _cabi.lib(), 0, _cabi.DeviceBuffer
    sigs, _ = survey()
    B = len(sigs)
    offsets = np.zeros(B + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in sigs])
    t = np.concatenate([s.time for s in sigs])
    m = np.concatenate([_quarter_scaled(np.asarray(s.values, dtype=float)) for s in sigs])
    nb_ = np.diff(offsets)
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(dev, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, dev, sp.value)
    bt, bm = DB.from_array(t, dev), DB.from_array(m, dev)
    ptr = _cabi._ptr
    start, step, stop = _string_grid(np.array([s.baseline for s in sigs]), 0.1, 1000)
    poff = np.arange(B + 1, dtype=np.int64) * 1000
    P = int(poff[-1])
    pairs = float(np.sum(nb_ * np.diff(poff)))
    wb = lib.pdc_stringlength_ragged_work_bytes(ptr(offsets), ptr(poff), B)
    work, out = DB(wb, dev), DB(P * 8, dev)

    def scan():
        _cabi.check(lib.pdc_stringlength_scan_ragged_dev(dev, sp.value, bt.ptr, bm.ptr, ptr(offsets), B, ptr(start),
                                                         ptr(step), ptr(stop), ptr(poff), out.ptr, None, 0, work.ptr,
                                                         wb))

    ms = tm.ms(scan, reps=5, warm=2)
    print(f"(a) StringLength ragged scan, n_periods=1000: B={B} N={offsets[-1]} ({nb_.min()}..{nb_.max()}) P={P} "
          f"pairs={pairs:.3e}: {ms:.2f} ms, {pairs / ms * 1e3:.3e} pair/s (every launch of the group + the metadata "
          f"upload and the read of the marked counts)")
    work.free()
    out.free()

    # the single call at a matching uniform shape: N = 2000 x 1e5 periods, the quad instance (the reference of the
    # target), and at 300 / 1000 / 4000 samples: the spread of the survey's N (the per-period fixed work of the duo
    # kernel - bucket zeroing and scans, barriers - weighs more on short curves)
    rng = np.random.default_rng(1)
    n_per = 100000
    rates = {}
    for n in (2000, 300, 1000, 4000):
        t2 = np.sort(rng.uniform(0.0, 1500.0, n))
        m2 = _quarter_scaled(np.sin(2 * np.pi * t2 / 13.7) + 0.2 * rng.standard_normal(n))
        p2 = _string_periods(t2[-1] - t2[0], 0.1 * 1000 / n_per, n_per)
        wb2 = lib.pdc_stringlength_work_bytes(n, n_per)
        b2t, b2m, b2p, b2o, b2w = (DB.from_array(t2, dev), DB.from_array(m2, dev), DB.from_array(p2, dev),
                                   DB(n_per * 8, dev), DB(wb2, dev))
        ms2 = tm.ms(lambda: _cabi.check(lib.pdc_stringlength_scan_dev(dev, sp.value, b2t.ptr, b2m.ptr, n, b2p.ptr,
                                                                      n_per, b2o.ptr, b2w.ptr, wb2)), reps=5)
        rates[n] = n * n_per / ms2 * 1e3
        print(f"(a) single call (pdc_stringlength_scan_dev, N={n} x {n_per} periods): {ms2:.2f} ms, "
              f"{rates[n]:.3e} pair/s" + (f"; ragged / single = {pairs / ms * 1e3 / rates[n]:.2f}" if n == 2000 else ""))
        for b in (b2t, b2m, b2p, b2o, b2w):
            b.free()
    # what the single call's rates at those N predict for the survey's pairs (per-curve rate interpolated in log N)
    ns = np.array(sorted(rates))
    pred = np.sum(nb_ * 1000.0 / np.interp(np.log(nb_), np.log(ns), [rates[k] for k in ns])) * 1e3
    print(f"(a) the single call's rates at N = 300 .. 4000, interpolated per curve, predict {pred:.2f} ms for the "
          f"survey's pairs (ragged scan: {ms:.2f} ms, {pred / ms:.2f} of that prediction)")
    for b in (bt, bm):
        b.free()
    if scan_only:
        _cabi.check(lib.pdc_stream_destroy(dev, sp.value))
        return

    # (c) wall clock through the public API against the per-curve loop
    StringLength().batch(sigs[:64], peaks=1, want_power=False)   # (warm: library, slots, LDS attributes)
    walls, libs = [], []
    real = _cabi.stringlength_scan_ragged
    for _ in range(3):
        spent = []

        def timed(*a, **k):
            t0 = time.perf_counter()
            r = real(*a, **k)
            spent.append(time.perf_counter() - t0)
            return r

        phase._cabi.stringlength_scan_ragged = timed
        try:
            t0 = time.perf_counter()
            res = StringLength().batch(sigs, peaks=1, want_power=False)
            walls.append(time.perf_counter() - t0)
        finally:
            phase._cabi.stringlength_scan_ragged = real
        libs.append(spent[0])
    i = int(np.argsort(walls)[1])
    w_batch, w_lib = walls[i], libs[i]
    StringLength()(sigs[0])
    t0 = time.perf_counter()
    loop = []
    for s in sigs:
        dips = StringLength()(s).find_dips()
        loop.append(dips.period[np.argmin(dips.values)] if len(dips) else np.nan)
    w_loop = time.perf_counter() - t0
    same = np.mean(np.asarray(loop) == res.peaks.period[:, 0])
    print(f"(c) StringLength().batch(4096 curves, peaks=1, want_power=False): {w_batch * 1e3:.1f} ms wall (median of 3): "
          f"{(w_batch - w_lib) * 1e3:.1f} ms host Python, {w_lib * 1e3:.1f} ms in the library (uploads, launches, "
          f"table); loop of StringLength()(s) + find_dips: {w_loop * 1e3:.0f} ms; {w_loop / w_batch:.1f}x; "
          f"same period on {same * 100:.2f} % of the curves")
    _cabi.check(lib.pdc_stream_destroy(dev, sp.value))


if __name__ == "__main__":
    if "--batch-only" in sys.argv:
        res = StringLength().batch(survey()[0], peaks=1, want_power=False)
        print(f"StringLength().batch: {len(res)} curves, best period of curve 0: {res.peaks.period[0, 0]:.6g}")
    else:
        main("--scan-only" in sys.argv)
