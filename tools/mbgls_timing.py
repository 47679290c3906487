"""Kernel time of the multiband GLS scan (``pdc_mbgls_scan_dev``: prologue + scan, inputs resident in HBM) with HIP
events for nterms = 1, 2, 3 and 1 and 6 bands at N = 1e5 x 1e5 frequencies and at 1000 x 2500, and of
``pdc_mhgls_scan_dev`` at the same nterms and shapes in the same process (developer tool).
``python tools/mbgls_timing.py > profiles/<round>_mbgls_timing.txt``"""
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
print("# fit_mean, individual weights; median of 5 launches after one warm-up; the whole curve is streamed by every tile "
      "(no sample parts); labels drawn uniformly, each band offset by 0.5; ratio = mbgls / mhgls at the same nterms and shape")
for n, nf in ((100_000, 100_000), (1000, 2500)):
    t, y, dy = bench.synth_curve(n)
    freq, _, _ = bench.throughput_grid(t, nf)
    f0, delta, _ = _cabi.grid_params(freq)
    band = np.random.default_rng(19).integers(0, 6, n).astype(np.int32)
    bt, bdy, bp = DB.from_array(t, 0), DB.from_array(dy, 0), DB(nf * 8, 0)
    by = {1: DB.from_array(y, 0), 6: DB.from_array(y + 0.5 * band, 0)}
    bb = {1: DB.from_array(np.zeros(n, dtype=np.int32), 0), 6: DB.from_array(band, 0)}
    for nterms in (1, 2, 3):
        tile = lib.pdc_mbgls_tile_bins(nterms)
        ms_mh = tm.ms(lambda: _cabi.check(lib.pdc_mhgls_scan_dev(0, sp.value, bt.ptr, by[1].ptr, bdy.ptr, n, f0, delta, 0, nf, nterms,
                                                                 1, 0, bp.ptr)), reps=5)
        mh = bp.to_array(np.float64, nf)
        print(f"N={n:7d} nf={nf:7d} pdc_mhgls_scan_dev nterms={nterms}     : {ms_mh:9.3f} ms  {n * nf / ms_mh / 1e6:8.1f} Gpair/s  "
              f"tile 1024 ({-(-nf // 1024)} workgroups)")
        for B in (1, 6):
            ms = tm.ms(lambda: _cabi.check(lib.pdc_mbgls_scan_dev(0, sp.value, bt.ptr, by[B].ptr, bdy.ptr, bb[B].ptr, n, B, f0, delta,
                                                                  0, nf, nterms, 1, 0, bp.ptr)), reps=5)
            p = bp.to_array(np.float64, nf)
            note = f"  max |power - mhgls| {np.nanmax(np.abs(p - mh)):.1e}" if B == 1 else ""
            print(f"N={n:7d} nf={nf:7d} pdc_mbgls_scan_dev nterms={nterms} B={B} : {ms:9.3f} ms  {n * nf / ms / 1e6:8.1f} Gpair/s  "
                  f"tile {tile} ({-(-nf // tile)} workgroups)  ratio {ms / ms_mh:5.2f}  peak bin {int(np.nanargmax(p))} "
                  f"(mhgls {int(np.nanargmax(mh))}){note}")
    for b in [bt, bdy, bp] + list(by.values()) + list(bb.values()):
        b.free()
