"""Kernel time of the frequency - spin-down plane scan (``pdc_htest_fdot_scan_dev``: prologue, scans, folds, best cell;
events resident in HBM, ridge and best cell only - no plane leaves the device) with HIP events for nharm = 1, 4, 20 and
nfd = 1, 16, 256 rows at 1e6 events x 1e5 bins, 1e6 x 2e3 and 1e4 x 2.5e4, beside ``pdc_htest_scan_dev`` (automatic
parts) at the same shape in the same process: time per row against the single scan (developer tool).  Every figure is
the median of its launches with the spread (max - min) / median beside it; a configuration whose launch takes seconds
gets fewer launches (the count is printed).
``python tools/htest_fdot_timing.py > profiles/<round>_htest_fdot_timing.txt``"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from periodicity_amd import _cabi  # noqa: E402

lib = _cabi.lib()
sp = C.c_void_p()
_cabi.check(lib.pdc_stream_create(0, C.byref(sp)))
tm = bench.EventTimer(lib, _cabi, 0, sp.value)
DB = _cabi.DeviceBuffer


def timed(fn):
    """(median ms, spread, launches): one warm-up, then 5 launches - 3 if one takes over a second; a launch of over ten
    seconds is measured twice, the first of them in place of a warm-up (its instance has run in the smaller shapes)."""
    first = tm.ms(fn, reps=1, warm=0)
    reps = 5 if first < 1e3 else 3 if first < 1e4 else 2
    runs = [tm.ms(fn, reps=1, warm=0) for _ in range(reps if first < 1e4 else 1)] + ([first] if first >= 1e4 else [])
    med = float(np.median(runs))
    return med, (max(runs) - min(runs)) / med, reps


print("device:", _cabi.device_info(0))
print("# photon weights; parts=0 everywhere: the automatic rule, what it chose is printed; per row = plane time / nfd;")
print("# ratio = per-row time / single scan (below 1: a row of the plane costs less than a scan of its own)")
for n, nf in ((1_000_000, 100_000), (1_000_000, 2_000), (10_000, 25_000)):
    rng = np.random.default_rng(20241008)
    t = np.sort(rng.uniform(0, float(n), n))
    w = rng.uniform(0.2, 1.0, n)
    freq, _, _ = bench.throughput_grid(t, nf)
    f0, delta, _ = _cabi.grid_params(freq)
    epoch = float(0.5 * (t[0] + t[-1]))
    far = float(np.max(np.abs(t - epoch)))
    bt, bw = DB.from_array(t, 0), DB.from_array(w, 0)
    bh, bm, bz = DB(nf * 8, 0), DB(nf * 4, 0), DB(nf * 8, 0)
    br, brr, brm, bb, bba = DB(nf * 8, 0), DB(nf * 4, 0), DB(nf * 4, 0), DB(8, 0), DB(24, 0)
    for nharm in (1, 4, 20):
        one, one_spread, reps = timed(lambda: _cabi.check(lib.pdc_htest_scan_dev(
            0, sp.value, bt.ptr, bw.ptr, n, f0, delta, 0, nf, nharm, 0, bh.ptr, bm.ptr, bz.ptr)))
        ht, k, ran = _cabi.htest_last_dispatch()
        print(f"N={n:8d} nf={nf:7d} nharm={nharm:2d} pdc_htest_scan_dev      <HT={ht:2d}, K={k}> x {ran:3d} parts              : "
              f"{one:11.3f} ms  spread {100 * one_spread:4.1f} %  ({reps} launches)", flush=True)
        for nfd in (1, 16, 256):
            fdot = np.linspace(-2.0, 2.0, nfd) * 2.0 / far ** 2 if nfd > 1 else np.array([2.0 * 2.0 / far ** 2])
            bf = DB.from_array(fdot, 0)
            ms, spread, reps = timed(lambda: _cabi.check(lib.pdc_htest_fdot_scan_dev(
                0, sp.value, bt.ptr, bw.ptr, n, f0, delta, 0, nf, bf.ptr, nfd, epoch, nharm, 0, 0, None, None, br.ptr, brr.ptr,
                brm.ptr, bb.ptr, bba.ptr)))
            ht, k, ran, per_launch, launches = _cabi.htest_fdot_last_dispatch()
            best = bb.to_array(np.float64, 1)[0]
            print(f"N={n:8d} nf={nf:7d} nharm={nharm:2d} pdc_htest_fdot_scan_dev nfd={nfd:3d} x {ran:3d} parts, {per_launch:3d} rows x "
                  f"{launches} launches: {ms:11.3f} ms  spread {100 * spread:4.1f} %  ({reps} launches)  per row {ms / nfd:10.3f} ms  "
                  f"ratio {ms / nfd / one:5.2f}  {(4 * ht - 2) * n * nf * nfd / ms / 1e9:6.2f} Tfma/s  best H {best:.3f}", flush=True)
            bf.free()
    for b in (bt, bw, bh, bm, bz, br, brr, brm, bb, bba):
        b.free()
