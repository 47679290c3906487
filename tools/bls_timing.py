"""Kernel time of the box-least-squares scan (``pdc_bls_scan_dev``: prologue, binning, search; inputs resident in HBM)
with HIP events over a few shapes, at ``slices`` = 1, 0 (chosen from the shape) and a sweep, and - as the CPU figure - the
test-local oracle's float64 path on a subset of the same periods (developer tool).
``python tools/bls_timing.py > profiles/<round>_bls_timing.txt``"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import bls_oracle as bo  # noqa: E402
from periodicity_amd import _cabi  # noqa: E402

lib = _cabi.lib()
sp = C.c_void_p()
_cabi.check(lib.pdc_stream_create(0, C.byref(sp)))
tm = bench.EventTimer(lib, _cabi, 0, sp.value)
DB = _cabi.DeviceBuffer
N_BINS, LEN_MIN, LEN_MAX, MIN_POINTS = 200, 2, 20, 5     # the defaults of periodicity_amd.phase.BLS
SWEEP = (1, 0, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64)
SHAPES = ((10_000, 10_000, (1, 0, 2)), (100_000, 1000, SWEEP), (100_000, 100, SWEEP + (128, 256)), (1_000_000, 1000, SWEEP),
          (20_000, 1000, SWEEP[:8]), (1000, 1000, (1, 0)))
print("device:", _cabi.device_info(0))
print(f"# n_bins={N_BINS} boxes of {LEN_MIN}..{LEN_MAX} bins, min_points={MIN_POINTS}, individual weights, both signs; device-side time "
      "(HIP events around one call: prologue + memset + binning + search), median of 7 calls after two warm-up calls; periods = "
      "linspace(2 median dt, baseline, n_periods), the grid of the class; slices=0: chosen from the shape by the library")
for n, n_periods, sweep in SHAPES:
    t, y, err = bo.curve(n, 31)
    periods = np.linspace(2 * np.median(np.diff(t)), t[-1] - t[0], n_periods)
    bt, by, be, bp = DB.from_array(t, 0), DB.from_array(y, 0), DB.from_array(err, 0), DB.from_array(periods, 0)
    o_pow, o_dep, o_st, o_box = DB(n_periods * 8, 0), DB(n_periods * 8, 0), DB(n_periods * 4, 0), DB(n_periods * 4, 0)
    first, best = None, None
    for slices in sweep:
        call = lambda: _cabi.check(lib.pdc_bls_scan_dev(0, sp.value, bt.ptr, by.ptr, be.ptr, n, bp.ptr, n_periods, N_BINS, LEN_MIN,
                                                        LEN_MAX, MIN_POINTS, 0, slices, o_pow.ptr, o_dep.ptr, o_st.ptr, o_box.ptr))
        ms = tm.ms(call, reps=7, warm=2)
        _cabi.check(lib.pdc_stream_sync(0, sp.value))
        got = (o_pow.to_array(np.float64, n_periods), o_dep.to_array(np.float64, n_periods), o_st.to_array(np.int32, n_periods),
               o_box.to_array(np.int32, n_periods))
        first = got if first is None else first
        same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, got))
        if slices and (best is None or ms < best[1]):
            best = (slices, ms)
        print(f"N={n:8d} periods={n_periods:6d} slices={slices:4d}: {ms:9.3f} ms  {n * n_periods / ms / 1e6:8.2f} G(sample, period)/s  "
              f"{'same bits as the first row' if same else 'DIFFERS from the first row'}")
    print(f"N={n:8d} periods={n_periods:6d} fastest forced: slices={best[0]} at {best[1]:.3f} ms; peak at period "
          f"{periods[int(np.nanargmax(first[0]))]:.4f} power {np.nanmax(first[0]):.4f}")
    # the CPU figure: the oracle's float64 path on a subset of the same periods, scaled to the grid
    sub = np.linspace(0, n_periods - 1, 8).astype(int)
    t0 = time.perf_counter()
    sc = bo.scan(t, y, err, periods[sub], N_BINS, LEN_MIN, LEN_MAX, MIN_POINTS, dtype=np.float64)
    cpu_ms = (time.perf_counter() - t0) * 1e3 / sub.size
    worst = float(np.nanmax(np.abs(sc.power() - first[0][sub])))
    print(f"N={n:8d} periods={n_periods:6d} CPU oracle (numpy, float64, one core): {cpu_ms:9.3f} ms per period on {sub.size} of the periods = "
          f"{cpu_ms * n_periods:11.1f} ms for the grid; max |device - oracle| on them {worst:.1e}")
    for b in (bt, by, be, bp, o_pow, o_dep, o_st, o_box):
        b.free()
