"""Kernel time of the H-test scan (``pdc_htest_scan_dev``: prologue + scan + finish, events resident in HBM) with HIP
events for nharm = 1, 2, 4, 8, 20 at 1e6 events x 1e5 bins, 1e6 x 2e3 and 1e4 x 2.5e4, each with the automatic sample
parts and with one part, and of ``pdc_mhgls_scan_dev`` with nterms = 4 at the same shapes in the same process - the
yardstick that existed before the H-test (developer tool).  fma per pair: 4 HT - 2 for the instance HT that nharm runs
(mhgls: 6 fma per sum and harmonic, 8 H - 2 of the recurrence = 46 at H = 4), the grid walk not counted.
``python tools/htest_timing.py > profiles/<round>_htest_timing.txt``"""
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
print("device:", _cabi.device_info(0))
print("# photon weights; median of 5 launches after one warm-up; parts=0: the automatic rule, the count it chose is printed")
for n, nf in ((1_000_000, 100_000), (1_000_000, 2_000), (10_000, 25_000)):
    rng = np.random.default_rng(20241008)
    t = np.sort(rng.uniform(0, float(n), n))
    w = rng.uniform(0.2, 1.0, n)
    y = 1.0 + 0.5 * np.sin(2 * np.pi * t / 37.3)
    freq, _, _ = bench.throughput_grid(t, nf)
    f0, delta, _ = _cabi.grid_params(freq)
    bt, bw, by = DB.from_array(t, 0), DB.from_array(w, 0), DB.from_array(y, 0)
    bh, bm, bz = DB(nf * 8, 0), DB(nf * 4, 0), DB(nf * 8, 0)
    ms = tm.ms(lambda: _cabi.check(lib.pdc_mhgls_scan_dev(0, sp.value, bt.ptr, by.ptr, bw.ptr, n, f0, delta, 0, nf, 4, 1, 0, bh.ptr)),
               reps=5)
    print(f"N={n:8d} nf={nf:7d} pdc_mhgls_scan_dev nterms=4          : {ms:10.3f} ms  {n * nf / ms / 1e6:8.1f} Gpair/s  "
          f"{46 * n * nf / ms / 1e9:7.2f} Tfma/s")
    for nharm in (1, 2, 4, 8, 20):
        for parts in (0, 1):
            ms = tm.ms(lambda: _cabi.check(lib.pdc_htest_scan_dev(0, sp.value, bt.ptr, bw.ptr, n, f0, delta, 0, nf, nharm, parts,
                                                                  bh.ptr, bm.ptr, bz.ptr)), reps=5)
            ht, k, ran = _cabi.htest_last_dispatch()
            h = bh.to_array(np.float64, nf)
            print(f"N={n:8d} nf={nf:7d} pdc_htest_scan_dev nharm={nharm:2d} parts={parts} -> <HT={ht:2d}, K={k}> x {ran:3d} parts: "
                  f"{ms:10.3f} ms  {n * nf / ms / 1e6:8.1f} Gpair/s  {(4 * ht - 2) * n * nf / ms / 1e9:7.2f} Tfma/s  "
                  f"max H {np.max(h):.3f}")
    for b in (bt, bw, by, bh, bm, bz):
        b.free()
