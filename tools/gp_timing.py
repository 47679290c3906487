"""Kernel time of the GP period scan (``pdc_gp_scan_dev``: records, repack, likelihoods, fold and best; inputs resident in
HBM, profile / cell / marginal / mean per period taken, no cube) with HIP events at the two ``HarmonicGP`` shapes of
DESIGN 4.1q - 2000 and 200 samples x 4096 periods x 64 cells, J = 2 with the mean profiled out - as likelihoods per second,
as executed fp64 instructions per (sample, candidate), and as a fraction of the fp64 issue rate the fixed-count fma probe
``tools/ubench/fp64_rate`` sustains in the same run; beside each the numpy oracle's float64 recursion
(tests/gp_oracle.py, vectorised over 256 candidates) on one core as the CPU line (developer tool).  The sample loop has
no branch, so the instructions a step executes are the loop's instructions in the unit's assembly:
``make -C periodicity_amd/csrc asm ASM_DIR=<dir>`` first, then
``python tools/gp_timing.py <dir>/gp.s > profiles/<round>_gp_timing.txt``"""
import collections
import ctypes as C
import itertools
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import gp_oracle as go  # noqa: E402
from kepler_timing import fma_probe  # noqa: E402
from periodicity_amd import _cabi, gp  # noqa: E402

SHAPES = ((2000, 4096, 64), (200, 4096, 64))   # n, periods, cells


def sample_loop(asm_path, J, fit_mean):
    """Instruction counts of the innermost loop of gp_loglike_kernel<J, fit_mean> in the unit's assembly."""
    lines = open(asm_path).read().split("\n")
    name = rf"_ZN.*gp_loglike_kernelILi{J}ELb{int(fit_mean)}E.*:"
    start = next(i for i, line in enumerate(lines) if re.match(name, line))
    body = lines[start:next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])]
    labels = {line.split(":")[0]: i for i, line in enumerate(body) if re.match(r"\.LBB\d+_\d+:", line)}
    loops = []
    for i, line in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", line)
        if m and labels.get(m.group(1), i) < i:
            loops.append((labels[m.group(1)], i))
    inner = [span for span in loops if not any(o != span and span[0] <= o[0] and o[1] <= span[1] for o in loops)]
    lo, hi = max(inner, key=lambda span: span[1] - span[0])
    ops = [x.split()[0] for x in (line.strip() for line in body[lo:hi + 1])
           if x and not x.startswith((".", ";")) and not x.endswith(":")]
    return collections.Counter(ops)


def main():
    ops = sample_loop(sys.argv[1], 2, True)
    lib = _cabi.lib()
    total = sum(ops.values())
    f64 = sum(v for k, v in ops.items() if "f64" in k and not k.startswith("v_cvt"))
    print("device:", _cabi.device_info(0))
    print(f"# sample loop of gp_loglike_kernel<2, true>: {total} instructions per (sample, candidate), {f64} of them fp64 "
          f"arithmetic, {ops.get('v_rcp_f64_e32', 0)} v_rcp_f64, {sum(v for k, v in ops.items() if k.startswith('ds_read'))} LDS "
          f"reads, {sum(v for k, v in ops.items() if k.startswith('v_cndmask'))} selects")
    probe, line = fma_probe()
    print(f"# fma probe, best line: {line}")
    print(f"#   = {probe:.3e} fp64 wave-instructions per second on the chip")
    print("# HarmonicGP grid: periods = linspace(1, 20, 4096) x Q0 (4) x dQ (4) x f (4), sigma = std(y), jitter = min(err)^2, "
          "fit_mean; median of 3 calls after one warm-up; one visit's measurement")
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(0, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, 0, sp.value)
    DB = _cabi.DeviceBuffer
    for n, n_periods, nq in SHAPES:
        t, y, dy = bench.synth_curve(n, period=7.3)
        like = gp.CeleriteLikelihood((t, y), dy)
        periods = np.linspace(1.0, 20.0, n_periods)
        cells = np.array(list(itertools.product(np.geomspace(0.5, 50.0, 4), np.geomspace(0.1, 10.0, 4), np.linspace(0.1, 1.0, 4))))
        assert cells.shape[0] == nq
        sigma, jitter = float(np.std(like.y)), float(np.min(like.err) ** 2)
        coeff = gp.device_coefficients(gp.rotation_terms(sigma, np.repeat(periods, nq), *np.tile(cells, (n_periods, 1)).T))
        M = coeff.shape[0]
        yc = like.y - np.mean(like.y)
        bufs = [DB.from_array(a, 0) for a in (like.tau, yc, like.var, coeff, np.full(M, jitter))]
        bufs += [DB(n_periods * 8, 0), DB(n_periods * 4, 0), DB(n_periods * 8, 0), DB(n_periods * 8, 0), DB(8, 0), DB(16, 0)]
        bt, by, bv, bc, bj, bp, bce, bm, bmu, bb, ba = bufs
        ms = tm.ms(lambda: _cabi.check(lib.pdc_gp_scan_dev(0, sp.value, bt.ptr, by.ptr, bv.ptr, n, bc.ptr, 2, bj.ptr, None, M, 1,
                                                           n_periods, nq, bp.ptr, bce.ptr, bm.ptr, bmu.ptr, None, bb.ptr,
                                                           ba.ptr)), reps=3)
        _cabi.check(lib.pdc_stream_sync(0, sp.value))
        best, at = bb.to_array(np.float64, 1), ba.to_array(np.int64, 2)
        steps = float(n) * M
        wave_instr = steps / 64 * f64
        # the CPU line: the float64 oracle on 256 of the candidates, one core
        pick = np.linspace(0, M - 1, 256).astype(int)
        t0 = time.perf_counter()
        want = go.recursion(like.tau, yc, like.var, coeff[pick], jitter, fit_mean=True, dtype=np.float64)
        cpu = (time.perf_counter() - t0) / 256
        got = _cabi.gp_loglike(like.tau, yc, like.var, coeff[pick], jitter, fit_mean=True)[0]
        worst = float(np.max(np.abs(got - want["loglike"]) / np.abs(want["loglike"])))
        print(f"N={n:5d} periods={n_periods} cells={nq} (M={M}, {_cabi.gp_last_dispatch()[2]} launch): {ms:9.3f} ms  "
              f"{M / ms / 1e3:8.2f} M likelihoods/s  {ms * 1e6 / M:7.2f} ns per likelihood  "
              f"{wave_instr / (ms * 1e-3):.3e} fp64 wave-instr/s = {wave_instr / (ms * 1e-3) / probe:.3f} of the probe;  "
              f"best ln L {best[0]:.3f} at period {periods[at[0]]:.4f}, cell {at[1]}")
        print(f"    CPU line: numpy float64 recursion, 256 candidates at once on one core: {cpu * 1e6:9.1f} us per likelihood "
              f"({cpu * M:8.1f} s for the grid); largest relative difference from the device on those 256: {worst:.1e}")
        for b in bufs:
            b.free()


if __name__ == "__main__":
    main()
