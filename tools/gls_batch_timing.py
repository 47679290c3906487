"""Timing of GLS.batch (ragged grids, gls_ragged.hip) on a survey-shaped batch (developer tool).

The batch: 4096 curves, N log-uniform in 300 .. 5000, baselines 100 .. 3000 days, jittered cadences, so that every
curve has its own grid (GLS's default rule).  Reports, with the inputs in HBM:
  (a) the ragged scan (prologue + scan + per-curve maximum; event-timed, median of 5) and its pair rate;
  (b) wall time of GLS().batch(..., peaks=1) against a loop of GLS()(s) + period_at_highest_peak;
  (c) the shared-grid batch (pdc_gls_scan_dev, 4096 curves of 2000 samples) at about the same number of pairs;
  (d) what the peak table adds: NaN-padded pitched copy + pdc_peaks_topk_dev (k = 1, by height).
Usage: python tools/gls_batch_timing.py [--scan-only]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from periodicity_amd import _cabi  # noqa: E402
from periodicity_amd.core import TSeries  # noqa: E402
from periodicity_amd.spectral import GLS  # noqa: E402


def survey(count=4096, seed=2026):
    rng = np.random.default_rng(seed)
    sigs, errs = [], []
    for _ in range(count):
        n = int(np.exp(rng.uniform(np.log(300), np.log(5000))))
        span = rng.uniform(100.0, 3000.0)
        t = np.sort((np.arange(n) + rng.uniform(-0.4, 0.4, n)) * (span / n)) + rng.uniform(0, 1e4)
        period = np.exp(rng.uniform(np.log(8 * span / n), np.log(span / 8)))
        dy = rng.uniform(0.05, 0.2, n)
        sigs.append(TSeries(t, 1.0 + np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)))
        errs.append(dy)
    return sigs, errs


def main(scan_only):
    lib, dev, DB = _cabi.lib(), 0, _cabi.DeviceBuffer
    sigs, errs = survey()
    gls = GLS()
    grids, f0, delta, foff = gls._ragged_grids(sigs)
    offsets = np.zeros(len(sigs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in sigs])
    t = np.concatenate([s.time for s in sigs])
    y = np.concatenate([s.values for s in sigs])
    dy = np.concatenate(errs)
    B, n_total, nf_total = len(sigs), int(offsets[-1]), int(foff[-1])
    nfb = np.diff(foff)
    nf_max = int(nfb.max())
    pairs = float(np.sum(np.diff(offsets) * nfb))
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(dev, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, dev, sp.value)
    bt, by, bdy = (DB.from_array(a, dev) for a in (t, y, dy))
    wb = lib.pdc_gls_ragged_work_bytes(n_total, B, nf_total, 0, 0)
    work, power = DB(wb, dev), DB(nf_total * 8, dev)
    amax, arg = DB(B * 8, dev), DB(B * 8, dev)
    pitched = DB(B * nf_max * 8, dev)
    ptr = _cabi._ptr

    def scan(pitch_ptr=None, pw=True):
        _cabi.check(lib.pdc_gls_scan_ragged_dev(dev, sp.value, bt.ptr, by.ptr, bdy.ptr, ptr(offsets), B, ptr(f0),
                                                ptr(delta), ptr(foff), 1, 0, power.ptr if pw else None, pitch_ptr,
                                                nf_max, amax.ptr, arg.ptr, work.ptr, wb))

    ms = tm.ms(scan, reps=5, warm=2)
    print(f"(a) ragged scan: B={B} N={n_total} ({np.diff(offsets).min()}..{np.diff(offsets).max()}) "
          f"nf={nf_total} ({nfb.min()}..{nf_max}) pairs={pairs:.3e}: {ms:.3f} ms, {pairs / ms * 1e3:.3e} pair/s "
          "(prologue + scan + maxima + the 0.2 MB metadata upload)")
    if scan_only:
        return

    # (d) the peak table's share: pitched copy with its NaN pad + top-1 by height on it
    out = DB(B * (1 + 5) * 8, dev)
    o = out.ptr

    def with_peaks():
        _cabi.check(lib.pdc_memset(dev, pitched.ptr, 0xFF, B * nf_max * 8))
        scan(pitched.ptr, pw=False)
        _cabi.check(lib.pdc_peaks_topk_dev(dev, sp.value, pitched.ptr, B, nf_max, 1, 0, o, o + B * 8, o + B * 32,
                                           o + B * 40, o + B * 16, o + B * 24))

    ms_p = tm.ms(with_peaks, reps=5, warm=1)
    ms_t = tm.ms(lambda: _cabi.check(lib.pdc_peaks_topk_dev(dev, sp.value, pitched.ptr, B, nf_max, 1, 0, o, o + B * 8,
                                                            o + B * 32, o + B * 40, o + B * 16, o + B * 24)), reps=5)
    print(f"(d) scan + NaN-padded [B][{nf_max}] copy + top-1 peak table: {ms_p:.2f} ms ({ms_p - ms:+.2f} ms over (a)); "
          f"the top-1 kernel alone {ms_t:.2f} ms")

    # (c) shared grid, same order of pairs: 4096 curves x 2000 samples, nf chosen to match
    n_c = 2000
    nf_c = int(round(pairs / (B * n_c)))
    rng = np.random.default_rng(5)
    tt = np.sort(rng.uniform(0, float(n_c), (B, n_c)), axis=1)
    dd = rng.uniform(0.05, 0.2, (B, n_c))
    yy = 1.0 + 0.5 * np.sin(2 * np.pi * tt / 37.0) + dd * rng.standard_normal((B, n_c))
    off_c = np.arange(B + 1, dtype=np.int64) * n_c
    df = 1.0 / n_c / 5
    ct, cy, cdy, coff = (DB.from_array(a, dev) for a in (tt, yy, dd, off_c))
    wbc = lib.pdc_gls_work_bytes(B * n_c, B, nf_c)
    workc, powc = DB(wbc, dev), DB(B * nf_c * 8, dev)
    ms_c = tm.ms(lambda: _cabi.check(lib.pdc_gls_scan_dev(dev, sp.value, ct.ptr, cy.ptr, cdy.ptr, coff.ptr, B * n_c, B,
                                                          0, 0.5 * df, df, 0, nf_c, 1, 0, powc.ptr, None, None,
                                                          workc.ptr, wbc)), reps=5, warm=1)
    pc = float(B) * n_c * nf_c
    print(f"(c) shared-grid batch B={B} n={n_c} nf={nf_c} pairs={pc:.3e}: {ms_c:.2f} ms, {pc / ms_c * 1e3:.3e} pair/s")
    for b in (workc, powc, ct, cy, cdy, coff, out):
        b.free()

    # (b) wall clock through the public API against the per-curve loop
    GLS().batch(sigs[:64], errs[:64], peaks=1)   # (warm: library, slots, LDS attributes)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = GLS().batch(sigs, errs, peaks=1, want_power=False)
        walls.append(time.perf_counter() - t0)
    w_batch = float(np.median(walls))
    t0 = time.perf_counter()
    loop = [GLS()(s, e).period_at_highest_peak for s, e in zip(sigs, errs)]
    w_loop = time.perf_counter() - t0
    same = np.mean(np.asarray(loop) == res.peaks.period[:, 0])
    print(f"(b) GLS().batch(4096 curves, peaks=1, want_power=False): {w_batch * 1e3:.1f} ms wall (median of 3); "
          f"loop of GLS()(s) + period_at_highest_peak: {w_loop * 1e3:.0f} ms; {w_loop / w_batch:.1f}x; "
          f"same period on {same * 100:.2f} % of the curves")
    for b in (bt, by, bdy, work, power, amax, arg, pitched):
        b.free()
    _cabi.check(lib.pdc_stream_destroy(dev, sp.value))


if __name__ == "__main__":
    main("--scan-only" in sys.argv)
