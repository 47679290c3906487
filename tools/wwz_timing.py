"""Device time of the WWZ scan (``pdc_wwz_scan_dev``: prologue + bounds + scan + fold, inputs resident in HBM, every
output taken) with HIP events at three shapes, and of ``pdc_mhgls_scan_dev`` with nterms = 2 (``mhgls_scan_kernel<2, 4>``,
the same skeleton) at 1e5 x 1e5 in the same process (developer tool).  Median, minimum and maximum of REPS launches after
one warm-up.  PARITY UNPINNED BY THE REFERENCE (the statistic is not in it).
``python tools/wwz_timing.py > profiles/<round>_wwz_timing.txt``"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from periodicity_amd import _cabi  # noqa: E402

REPS = 5
PEAK = 39.3e12        # fp64 vector instructions per second (fma counted once): 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
FOSTER = 1 / (8 * np.pi ** 2)
# fp64 instructions per (sample, frequency) pair, counted from the source: 14 for the ten sums and their
# four products, and per (sample, thread), shared by its K = 8 pairs: 8 (seed rotation, first step of the walk) + 2 (K - 2)
# (walk) + 40 (two software exp and their arguments) + 2 (K - 1) (window recurrence)
WWZ_OPS = 14 + (8 + 2 * 6 + 40 + 2 * 7) / 8
# mhgls_scan_kernel<2, 4>: 6 H sums + 4 H - 2 ladder + 1 (2 cos) and per (sample, thread) 8 + 2 (K - 2), K = 4
MHGLS_OPS = 12 + 6 + 1 + (8 + 2 * 2) / 4

lib = _cabi.lib()
sp = C.c_void_p()
_cabi.check(lib.pdc_stream_create(0, C.byref(sp)))
DB = _cabi.DeviceBuffer


def new_event():
    e = C.c_void_p()
    _cabi.check(lib.pdc_event_create(0, C.byref(e)))
    return e.value


EV = (new_event(), new_event())


def times_ms(fn, reps=REPS):
    fn()
    out = []
    for _ in range(reps):
        _cabi.check(lib.pdc_event_record(0, EV[0], sp.value))
        fn()
        _cabi.check(lib.pdc_event_record(0, EV[1], sp.value))
        ms = C.c_float()
        _cabi.check(lib.pdc_event_elapsed_ms(0, EV[0], EV[1], C.byref(ms)))
        out.append(ms.value)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def curve(n):
    """Unit mean spacing: n uniform times on [0, n), a sinusoid at 0.1 plus noise, individual uncertainties."""
    rng = np.random.default_rng(23)
    t = np.sort(rng.uniform(0, n, n))
    dy = rng.uniform(0.1, 0.3, n)
    return t, np.sin(2 * np.pi * 0.1 * t) + dy * rng.standard_normal(n), dy


print("device:", _cabi.device_info(0))
tile = _cabi.wwz_tile_bins()
print(f"# grid (j + 1) 0.5 / nf, tau on linspace(t[0], t[-1], ntau); median [min .. max] of {REPS} launches after one warm-up;")
print(f"# pairs = visited x {tile} (a workgroup evaluates its whole tile; the last tile of a grid is padded);")
print(f"# fp64 rate = pairs x {WWZ_OPS:.2f} instructions (mhgls<2, 4>: {MHGLS_OPS:.2f}) against {PEAK / 1e12:.1f} T/s")

n, nf = 100_000, 100_000
t, y, dy = curve(n)
delta = 0.5 / nf
bt, by, bdy, bp = DB.from_array(t, 0), DB.from_array(y, 0), DB.from_array(dy, 0), DB(nf * 8, 0)
med, lo, hi = times_ms(lambda: _cabi.check(lib.pdc_mhgls_scan_dev(0, sp.value, bt.ptr, by.ptr, bdy.ptr, n, delta, delta, 0, nf,
                                                                   2, 1, 0, bp.ptr)))
mh_rate = n * nf * MHGLS_OPS / (med * 1e-3)
print(f"mhgls nterms=2 N={n} nf={nf}: {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]  {n * nf / med / 1e6:8.1f} Gpair/s  "
      f"{mh_rate / 1e12:6.2f} T/s = {mh_rate / PEAK:.3f} of peak")
for b in (bt, by, bdy, bp):
    b.free()

for n, nf, ntau, decay in ((10_000, 25_000, 64, FOSTER), (100_000, 10_000, 256, FOSTER), (100_000, 10_000, 256, 1e-12)):
    t, y, dy = curve(n)
    tau = np.linspace(t[0], t[-1], ntau)
    delta = 0.5 / nf
    ins = [DB.from_array(a, 0) for a in (t, y, dy, tau)]
    cells = ntau * nf
    outs = [DB(count * 8, 0) for count in (cells, cells, cells, ntau, ntau, ntau, 1, 2, 1)]
    med, lo, hi = times_ms(lambda: _cabi.check(lib.pdc_wwz_scan_dev(
        0, sp.value, ins[0].ptr, ins[1].ptr, ins[2].ptr, n, delta, delta, nf, ins[3].ptr, ntau, decay, 6.0,
        *[b.ptr for b in outs])))
    visited = int(outs[8].to_array(np.int64, 1)[0])
    tiles = (nf + tile - 1) // tile
    pairs = visited * tile
    rate = pairs * WWZ_OPS / (med * 1e-3)
    best = outs[6].to_array(np.float64, 1)[0]
    at = outs[7].to_array(np.int64, 2)
    print(f"wwz N={n} nf={nf} ntau={ntau} decay={decay:.3g}: {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]  visited {visited} of "
          f"{n * tiles * ntau} ({visited / (n * tiles * ntau):.3f})  {pairs / med / 1e6:8.1f} Gpair/s  {rate / 1e12:6.2f} T/s = "
          f"{rate / PEAK:.3f} of peak, {rate / mh_rate:.2f} of the mhgls rate;  best WWZ {best:.1f} at f = "
          f"{(at[1] + 1) * delta:.4f} (workgroups: {tiles * ntau})")
    for b in ins + outs:
        b.free()
