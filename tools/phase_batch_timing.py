"""Timing of PDM.batch (ragged period grids, pdm_ragged.hip) on a survey-shaped batch (developer tool).

The batch: the survey of tools/gls_batch_timing.py (4096 curves, N log-uniform in 300 .. 5000, baselines 100 .. 3000
days, jittered cadences), scanned with PDM's defaults (nb = 5, nc = 2, 1000 periods per curve) and with
n_periods=None (every curve its own count).  Reports, with the inputs in HBM:
  (a) the ragged scan (prologue + scan; event-timed, median of 5) and its pair rate, next to C5 PDM's
      (pdc_pdm_scan_dev, N = 5e4 x 1e5 periods) measured in the same run;
  (c) wall time of PDM().batch(..., peaks=1, want_power=False) against a loop of PDM()(s) + find_dips, with its
      host (Python) / library split.
Usage: python tools/phase_batch_timing.py [--scan-only | --batch-only]   (--batch-only: one PDM().batch call of the
survey, peaks=1, want_power=False - the run to put under a kernel trace)
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
from periodicity_amd.phase import PDM, _linspace_steps, _pdm_limits  # noqa: E402


def description(sigs, n_periods):
    lim = [_pdm_limits(s, None, None, n_periods, 1) for s in sigs]
    start = np.array([x[0] for x in lim])
    stop = np.array([x[1] for x in lim])
    count = np.array([x[2] for x in lim], dtype=np.int64)
    poff = np.zeros(len(sigs) + 1, dtype=np.int64)
    poff[1:] = np.cumsum(count)
    return start, _linspace_steps(start, stop, count), stop, poff


def main(scan_only):
    lib, dev, DB = _cabi.lib(), 0, _cabi.DeviceBuffer
    sigs, _ = survey()
    B = len(sigs)
    offsets = np.zeros(B + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in sigs])
    t = np.concatenate([s.time for s in sigs])
    x = np.concatenate([s.values for s in sigs])
    sigma = np.array([np.var(s.values, ddof=1) for s in sigs])
    nb_ = np.diff(offsets)
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(dev, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, dev, sp.value)
    bt, bx = DB.from_array(t, dev), DB.from_array(x, dev)
    ptr = _cabi._ptr
    for label, n_periods in (("n_periods=1000", 1000), ("n_periods=None", None)):
        start, step, stop, poff = description(sigs, n_periods)
        P = int(poff[-1])
        pairs = float(np.sum(nb_ * np.diff(poff)))
        wb = lib.pdc_phase_ragged_work_bytes(B, P, 0, 0)
        work, out = DB(wb, dev), DB(P * 8, dev)

        def scan():
            _cabi.check(lib.pdc_phase_scan_ragged_dev(0, dev, sp.value, bt.ptr, bx.ptr, ptr(offsets), B, ptr(start),
                                                      ptr(step), ptr(stop), ptr(poff), ptr(sigma), None, 5, 2, out.ptr,
                                                      None, 0, work.ptr, wb))

        ms = tm.ms(scan, reps=5, warm=2)
        print(f"(a) PDM ragged scan, {label}: B={B} N={offsets[-1]} ({nb_.min()}..{nb_.max()}) P={P} "
              f"({np.diff(poff).min()}..{np.diff(poff).max()}) pairs={pairs:.3e}: {ms:.2f} ms, "
              f"{pairs / ms * 1e3:.3e} pair/s (prologue + scan + the metadata upload)")
        work.free()
        out.free()
    if scan_only:
        return

    # C5 PDM (N = 5e4 x 1e5 periods), the single-curve rate this batch is measured against
    t5, y5, _, periods, _ = bench.c5_inputs()
    n, n_per = t5.size, periods.size
    b5t, b5x, b5p, b5o = DB.from_array(t5, dev), DB.from_array(y5, dev), DB.from_array(periods, dev), DB(n_per * 8, dev)
    s5 = float(np.var(y5, ddof=1))
    ms5 = tm.ms(lambda: _cabi.check(lib.pdc_pdm_scan_dev(dev, sp.value, b5t.ptr, b5x.ptr, n, b5p.ptr, n_per, 5, 2, s5,
                                                         b5o.ptr)), reps=5)
    print(f"(a) C5 PDM (pdc_pdm_scan_dev, N={n} x {n_per} periods): {ms5:.2f} ms, {n * n_per / ms5 * 1e3:.3e} pair/s")
    for b in (b5t, b5x, b5p, b5o, bt, bx):
        b.free()

    # (c) wall clock through the public API against the per-curve loop
    PDM().batch(sigs[:64], peaks=1, want_power=False)   # (warm: library, slots, LDS attributes)
    walls, libs = [], []
    real = _cabi.phase_scan_ragged
    for _ in range(3):
        spent = []

        def timed(*a, **k):
            t0 = time.perf_counter()
            r = real(*a, **k)
            spent.append(time.perf_counter() - t0)
            return r

        phase._cabi.phase_scan_ragged = timed
        try:
            t0 = time.perf_counter()
            res = PDM().batch(sigs, peaks=1, want_power=False)
            walls.append(time.perf_counter() - t0)
        finally:
            phase._cabi.phase_scan_ragged = real
        libs.append(spent[0])
    i = int(np.argsort(walls)[1])
    w_batch, w_lib = walls[i], libs[i]
    t0 = time.perf_counter()
    loop = []
    for s in sigs:
        dips = PDM()(s).find_dips()
        loop.append(dips.period[np.argmin(dips.values)] if len(dips) else np.nan)
    w_loop = time.perf_counter() - t0
    same = np.mean(np.asarray(loop) == res.peaks.period[:, 0])
    print(f"(c) PDM().batch(4096 curves, peaks=1, want_power=False): {w_batch * 1e3:.1f} ms wall (median of 3): "
          f"{(w_batch - w_lib) * 1e3:.1f} ms host Python, {w_lib * 1e3:.1f} ms in the library (uploads, launches, "
          f"table); loop of PDM()(s) + find_dips: {w_loop * 1e3:.0f} ms; {w_loop / w_batch:.1f}x; "
          f"same period on {same * 100:.2f} % of the curves")
    _cabi.check(lib.pdc_stream_destroy(dev, sp.value))


if __name__ == "__main__":
    if "--batch-only" in sys.argv:
        res = PDM().batch(survey()[0], peaks=1, want_power=False)
        print(f"PDM().batch: {len(res)} curves, best period of curve 0: {res.peaks.period[0, 0]:.6g}")
    else:
        main("--scan-only" in sys.argv)
