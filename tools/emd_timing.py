"""Device time of the empirical mode decompositions (developer tool): the batch kernel alone (``pdc_emd_batch_dev``, rows
resident in HBM, HIP events) and end to end through the classes (copies included), as the median of 5 calls after one
warm-up, at three shapes - ``CEEMDAN`` at E = 50 on the two-tone curve of 1000 samples, ``EMD.batch`` of 500 x 4096 noise
rows (LDS route) and of 64 x 65 536 noise rows (workspace route).  Beside each: the literal oracle (tests/emd_oracle.py:
scipy's find_peaks, splrep, splev on one thread) on the same input - on the first rows only where the whole batch would
take minutes, and said so -, sift evaluations per second and barriers per sift evaluation (ceil(N / 256) trips of the
scan + 7).  PARITY UNPINNED BY THE REFERENCE.
``python tools/emd_timing.py > profiles/<round>_emd_timing.txt``"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import emd_oracle as eo  # noqa: E402
from periodicity_amd import _cabi  # noqa: E402
from periodicity_amd.core import TSeries  # noqa: E402
from periodicity_amd.decomposition import CEEMDAN, EMD  # noqa: E402

PARAMS = (2000, 2, 0.05, 0.50, 0.05)
K = _cabi.EMD_MAX_MODES


def wall(fn, reps=5):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(out))


def kernel_ms(lib, tm, sp, t, rows):
    B, n = rows.shape
    DB = _cabi.DeviceBuffer
    bufs = [DB.from_array(t, 0), DB.from_array(rows, 0), DB(B * K * n * 8, 0), DB(B * n * 8, 0), DB(B * 8, 0),
            DB(B * K * 8, 0), DB(B * 8, 0)]
    ms = tm.ms(lambda: _cabi.check(lib.pdc_emd_batch_dev(0, sp, bufs[0].ptr, bufs[1].ptr, n, B, *PARAMS, K,
                                                         *[b.ptr for b in bufs[2:]])), reps=5)
    for b in bufs:
        b.free()
    return ms


def batch(lib, tm, sp, B, n, oracle_rows):
    t = np.arange(n, dtype=np.float64)
    rows = np.random.default_rng(n).standard_normal((B, n))
    kern = kernel_ms(lib, tm, sp, t, rows)
    emd = EMD()
    e2e = wall(lambda: emd.batch(rows))
    route, threads, _, evals = _cabi.emd_last_dispatch()
    t0 = time.perf_counter()
    for b in range(oracle_rows):
        eo.emd(t, rows[b])
    cpu = (time.perf_counter() - t0) / oracle_rows * B
    modes = np.mean([len(m) for m in emd.batch_modes])
    print(f"emd.batch {B} x {n} noise rows ({route} route, {threads} threads per row): kernel {kern:.1f} ms, end to end "
          f"{e2e:.1f} ms; {evals} sift evaluations ({modes:.1f} modes per row) = {evals / (kern * 1e-3):.3e} per second; "
          f"{-(-n // 256) + 7} barriers per sift evaluation; literal oracle, one thread: {cpu:.1f} s for the batch "
          f"(measured on its first {oracle_rows} rows) = {1e3 * cpu / e2e:.0f} x the device's end to end")


def main():
    lib = _cabi.lib()
    print("device:", _cabi.device_info(0))
    print("# median of 5 calls after one warm-up; one visit to one machine")
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(0, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, 0, sp.value)

    t, x = eo.tones(1000)
    rng = np.random.default_rng(42)
    noise = np.stack([rng.standard_normal(1000) for _ in range(50)])
    kern = kernel_ms(lib, tm, sp.value, t, noise)
    e2e = wall(lambda: CEEMDAN(ensemble_size=50, random_seed=42)(TSeries(values=x)))
    t0 = time.perf_counter()
    want = eo.ceemdan(t, x, ensemble_size=50, random_seed=42)
    cpu = time.perf_counter() - t0
    print(f"ceemdan E=50 N=1000 (two tones, {len(want[0])} IMFs, {len(want[2])} stages): end to end {e2e:.1f} ms; the "
          f"decomposition of 50 noise rows alone, kernel {kern:.1f} ms; {-(-1000 // 256) + 7} barriers per sift evaluation; "
          f"literal oracle, one thread: {cpu:.2f} s = {1e3 * cpu / e2e:.1f} x")
    batch(lib, tm, sp.value, 500, 4096, 4)
    batch(lib, tm, sp.value, 64, 65536, 1)


if __name__ == "__main__":
    main()
