"""Device time of the WPS scan (``pdc_wps_scan_dev``: taps + scan + fold, inputs resident in HBM) with HIP events, with
and without the spectrum plane, end to end through the class (copies included), the fma the scan kernel executes over
that time against the fp64 rate the fixed-count probe ``tools/ubench/fp64_rate`` sustains in the same run, and the
float64 literal recipe (tests/wps_oracle.py: ``np.convolve``, ``np.diff``) on the CPU at the small shape (developer
tool).  The executed fma are counted from the taps as the kernel groups them: two per (tap slot, output), a group's taps
padded to a multiple of four, a whole tile per workgroup, groups whose window misses the curve skipped.
PARITY UNPINNED BY THE REFERENCE.
``python tools/wps_timing.py > profiles/<round>_wps_timing.txt``"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import wps_oracle as wo  # noqa: E402
from kepler_timing import fma_probe  # noqa: E402
from periodicity_amd import _cabi  # noqa: E402
from periodicity_amd.core import TSeries  # noqa: E402
from periodicity_amd.timefrequency import WPS, cmor_table  # noqa: E402

DT = 0.02
EXTRA = 1024   # kExtra of csrc/wps.hip: the filter positions one staged window reaches beyond the tile
SHAPES = ((65536, 512, 0.1, 100.0), (1500, 200, 0.1, 10.0))   # n, n_periods, shortest and longest period


def executed_fma(n, scales, step, span):
    """fma the scan kernel executes, and the (tap, cell) pairs of the definition (taps x n per scale)."""
    tile = _cabi.wps_tile()
    tiles = -(-n // tile)
    n0 = tile * np.arange(tiles)
    executed = useful = 0
    for s in scales:
        position, _, _, length = _cabi.wps_taps(s, step, span)
        useful += position.size * n
        base = n0 - (length + 1) // 2
        a = 0
        while a < position.size:
            b = int(np.searchsorted(position, position[a] + EXTRA, side="right"))
            reach = position[b - 1] - position[a]
            g0 = base + position[a]
            live = np.count_nonzero((g0 + tile + reach > 0) & (g0 < n))
            executed += live * (-(-(b - a) // 4) * 4) * tile * 2
            a = b
    return executed, useful


def main():
    lib = _cabi.lib()
    print("device:", _cabi.device_info(0))
    probe, line = fma_probe()
    print(f"# fma probe, best line: {line}")
    print(f"#   = {probe * 64:.3e} fp64 fma per second on the chip")
    print("# dt = 0.02, log-spaced periods, the curve of tests/wps_oracle.py; median of 5 calls after one warm-up; "
          "one visit's measurement")
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(0, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, 0, sp.value)
    DB = _cabi.DeviceBuffer
    table, step, span = cmor_table()
    for n, n_periods, p_lo, p_hi in SHAPES:
        t, y = wo.curve(n)
        x = y - np.mean(y)
        periods = np.geomspace(p_lo, p_hi, n_periods)
        scales = periods / np.median(np.diff(t))
        ins = [DB.from_array(a, 0) for a in (x, t, periods, scales, table)]
        plane = DB(n * n_periods * 8, 0)
        small = [DB(count * 8, 0) for count in (n_periods, n, n_periods, n_periods, n, n)]

        def call(with_plane):
            _cabi.check(lib.pdc_wps_scan_dev(0, sp.value, ins[0].ptr, ins[1].ptr, n, ins[2].ptr, ins[3].ptr, n_periods,
                                             ins[4].ptr, step, span, float(np.exp2(0.5)), float(t.min()), float(t.max()),
                                             plane.ptr if with_plane else None, None, *[b.ptr for b in small]))
        bare = tm.ms(lambda: call(False), reps=5)
        full = tm.ms(lambda: call(True), reps=5)
        executed, useful = executed_fma(n, scales, step, span)
        wps = WPS(periods)
        signal = TSeries(t, y)
        e2e = {}
        for planes in (False, True):
            wps(signal, want_planes=planes)
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                wps(signal, want_planes=planes)
                walls.append(time.perf_counter() - t0)
            e2e[planes] = 1e3 * float(np.median(walls))
        rate = executed / (bare * 1e-3)
        print(f"wps N={n} periods={n_periods} ({p_lo:g} .. {p_hi:g}, scales {scales[0]:.1f} .. {scales[-1]:.1f}): "
              f"kernels {bare:.3f} ms without planes, {full:.3f} ms with the spectrum plane; end to end {e2e[False]:.2f} ms "
              f"without planes, {e2e[True]:.2f} ms with; {executed:.3e} fma executed ({2 * useful / executed:.3f} of them the "
              f"definition's), {rate:.3e} fma/s = {rate / (probe * 64):.3f} of the probe's rate; workspace "
              f"{_cabi.wps_work_bytes(n, n_periods) / 2 ** 20:.1f} MiB, plane {n * n_periods * 8 / 2 ** 20:.1f} MiB")
        for b in ins + small + [plane]:
            b.free()
        if n <= 2000:
            t0 = time.perf_counter()
            wo.spectrum(x, scales, np.complex128)
            cpu = 1e3 * (time.perf_counter() - t0)
            print(f"cpu N={n} periods={n_periods}: the float64 literal recipe (np.convolve, np.diff, one thread) {cpu:.1f} ms "
                  f"= {cpu / e2e[True]:.1f} x the device's end to end with planes")


if __name__ == "__main__":
    main()
