"""Kernel time of the multi-harmonic GLS scan (``pdc_mhgls_scan_dev``: prologue + scan, inputs resident in HBM) with
HIP events for nterms = 1 .. 4 at N = 1e5 x 1e5 frequencies and at 1000 x 2500, and - for nterms = 1 - of
``pdc_gls_scan_dev`` in the same process at both shapes (developer tool).
``python tools/mhgls_timing.py > profiles/<round>_mhgls_timing.txt``"""
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
print("# fit_mean, individual weights; median of 5 launches after one warm-up; the whole curve is streamed by every tile of "
      "1024 frequencies (no sample parts): the short grids fill 98 and 3 workgroups of the chip's 256 CUs")
for n, nf in ((100_000, 100_000), (1000, 2500)):
    t, y, dy = bench.synth_curve(n)
    freq, _, _ = bench.throughput_grid(t, nf)
    f0, delta, _ = _cabi.grid_params(freq)
    bt, by, bdy, bp = DB.from_array(t, 0), DB.from_array(y, 0), DB.from_array(dy, 0), DB(nf * 8, 0)
    wb = lib.pdc_gls_work_bytes(n, 1, nf)
    w = DB(wb, 0)
    ms = tm.ms(lambda: _cabi.check(lib.pdc_gls_scan_dev(0, sp.value, bt.ptr, by.ptr, bdy.ptr, None, n, 1, 0, f0, delta, 0, nf, 1, 0,
                                                        bp.ptr, None, None, w.ptr, wb)), reps=5)
    gls = bp.to_array(np.float64, nf)
    print(f"N={n:7d} nf={nf:7d} pdc_gls_scan_dev           : {ms:9.3f} ms  {n * nf / ms / 1e6:8.1f} Gpair/s")
    for nterms in (1, 2, 3, 4):
        ms = tm.ms(lambda: _cabi.check(lib.pdc_mhgls_scan_dev(0, sp.value, bt.ptr, by.ptr, bdy.ptr, n, f0, delta, 0, nf, nterms, 1, 0,
                                                              bp.ptr)), reps=5)
        p = bp.to_array(np.float64, nf)
        note = f"  max |power - GLS| {np.nanmax(np.abs(p - gls)):.1e}" if nterms == 1 else ""
        print(f"N={n:7d} nf={nf:7d} pdc_mhgls_scan_dev nterms={nterms}: {ms:9.3f} ms  {n * nf / ms / 1e6:8.1f} Gpair/s  "
              f"peak bin {int(np.nanargmax(p))} (GLS {int(np.nanargmax(gls))}){note}")
    for b in (bt, by, bdy, bp, w):
        b.free()
