"""Kernel time of the discrete correlation function (``pdc_dcf_scan_dev``: scan + fold, inputs resident in HBM) with HIP
events at three shapes, as pairs per second, with the chunk the library chose (developer tool).  With arguments
``chunk ...`` every shape is also timed at those forced chunks.
``python tools/dcf_timing.py [chunk ...] > profiles/<round>_dcf_timing.txt``"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from periodicity_amd import _cabi  # noqa: E402

NLAG = 1000
SHAPES = (("auto", 10_000, 10_000), ("auto", 100_000, 100_000), ("cross", 100_000, 100_000))


def main():
    lib = _cabi.lib()
    forced = [0] + [int(x) for x in sys.argv[1:]]
    print("device:", _cabi.device_info(0))
    print(f"# {NLAG} lag bins; auto: lags 0 .. half the baseline, the diagonal left out; cross: two curves on one baseline, "
          "lags -half .. +half of it; centred values; median of 3 calls after one warm-up; one visit's measurement")
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(0, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, 0, sp.value)
    DB = _cabi.DeviceBuffer
    for kind, na, nb in SHAPES:
        ta, a, _ = bench.synth_curve(na, k=2)
        tb, b = ta, a
        half = 0.5 * (ta[-1] - ta[0])
        if kind == "cross":
            tb, b, _ = bench.synth_curve(nb, k=3)
            edges = np.linspace(-half, half, NLAG + 1)
        else:
            dlag = half / NLAG
            edges = (0.0 - 0.5 * dlag) + dlag * np.arange(NLAG + 1)
        bufs = [DB.from_array(x, 0) for x in (ta, a - a.mean(), tb, b - b.mean(), edges)] + [DB(NLAG * 8, 0), DB(6 * NLAG * 8, 0)]
        bta, ba, btb, bb, be, bp, bs = bufs
        if kind == "auto":
            btb, bb = bta, ba
        for chunk in forced:
            ms = tm.ms(lambda: _cabi.check(lib.pdc_dcf_scan_dev(0, sp.value, bta.ptr, ba.ptr, na, btb.ptr, bb.ptr, nb, be.ptr,
                                                                NLAG, int(kind == "auto"), chunk, bp.ptr, bs.ptr)), reps=3)
            _cabi.check(lib.pdc_stream_sync(0, sp.value))
            pairs = bp.to_array(np.int64, NLAG)
            chunks, size = _cabi.dcf_last_dispatch()
            print(f"{kind:5s} na={na:6d} nb={nb:6d}: {ms:9.3f} ms  {int(pairs.sum()):12d} pairs ({pairs.min()} .. {pairs.max()} a bin)  "
                  f"{pairs.sum() / ms / 1e6:7.2f} Gpair/s  {chunks} chunks of {size}{'' if chunk == 0 else ' (forced)'}, "
                  f"workspace {_cabi.dcf_work_bytes(na, nb, NLAG, chunk) / 2 ** 20:.1f} MiB")
        for buf in bufs:
            buf.free()


if __name__ == "__main__":
    main()
