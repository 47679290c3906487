"""Kernel time of the Keplerian scan (``pdc_kepler_scan_dev``: prologue + scan + fold, inputs resident in HBM, power and
cell per bin taken, no cube) with HIP events at three shapes, as solves per second, as executed fp64 instructions per
solve, and as a fraction of the fp64 issue rate the fixed-count fma probe ``tools/ubench/fp64_rate`` sustains in the
same run (developer tool).  The sample loop of the scan has no branch, so the instructions a solve executes are the
loop's instructions in the unit's assembly over the cells per thread:
``make -C periodicity_amd/csrc asm ASM_DIR=<dir>`` first, then
``python tools/kepler_timing.py <dir>/kepler.s > profiles/<round>_kepler_timing.txt``"""
import collections
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from periodicity_amd import _cabi  # noqa: E402

SHAPES = ((1000, 100_000, 10, 32), (200, 10_000, 20, 64), (10_000, 10_000, 10, 32))   # n, nf, ne, nm


def sample_loop(asm_path):
    """Instruction counts of the innermost loop of kepler_scan_kernel in the unit's assembly."""
    lines = open(asm_path).read().split("\n")
    start = next(i for i, line in enumerate(lines) if re.match(r"_ZN.*kepler_scan_kernel.*:", line))
    body = lines[start:next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])]
    labels = {line.split(":")[0]: i for i, line in enumerate(body) if re.match(r"\.LBB\d+_\d+:", line)}
    loops = []
    for i, line in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", line)
        if m and labels.get(m.group(1), i) < i:
            loops.append((labels[m.group(1)], i))
    lo, hi = max(loops, key=lambda span: span[1] - span[0])
    ops = [x.split()[0] for x in (line.strip() for line in body[lo:hi + 1])
           if x and not x.startswith((".", ";")) and not x.endswith(":")]
    return collections.Counter(ops)


def fma_probe():
    """The best fp64 rate of tools/ubench/fp64_rate (built on demand) in wave-instructions per second, and its line."""
    exe = os.path.join(ROOT, "tools", "ubench", "fp64_rate")
    if not os.path.isfile(exe):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", exe + ".hip", "-o", exe],
                       check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    best = max(out, key=lambda line: float(re.search(r"([\d.]+) TFLOP/s", line).group(1)))
    tflops = float(re.search(r"([\d.]+) TFLOP/s", best).group(1))
    return tflops * 1e12 / 2 / 64, best


def main():
    ops = sample_loop(sys.argv[1])
    lib = _cabi.lib()
    kc = _cabi.kepler_cell_group()
    total = sum(ops.values())
    f64 = sum(v for k, v in ops.items() if "f64" in k and not k.startswith("v_cvt"))
    f32 = sum(v for k, v in ops.items() if k.startswith("v_") and "f32" in k)
    print("device:", _cabi.device_info(0))
    print(f"# sample loop of kepler_scan_kernel<{kc}>: {total} instructions for {kc} solves, {f64} of them fp64 arithmetic "
          f"({f64 / kc:.1f} per solve: the solve, its six fmas and its share of the phase), {f32} fp32 or conversions, "
          f"{ops.get('v_rcp_f64_e32', 0)} v_rcp_f64, {ops.get('s_load_dwordx8', 0)} scalar load")
    probe, line = fma_probe()
    print(f"# fma probe, best line: {line}")
    print(f"#   = {probe:.3e} fp64 wave-instructions per second on the chip")
    print("# fit_mean, individual weights, ecc = linspace(0, 0.9, ne), m0 = arange(nm) / nm; median of 3 calls after one "
          "warm-up; one visit's measurement")
    sp = C.c_void_p()
    _cabi.check(lib.pdc_stream_create(0, C.byref(sp)))
    tm = bench.EventTimer(lib, _cabi, 0, sp.value)
    DB = _cabi.DeviceBuffer
    for n, nf, ne, nm in SHAPES:
        t, y, dy = bench.synth_curve(n)
        freq, _, _ = bench.throughput_grid(t, nf)
        f0, delta, _ = _cabi.grid_params(freq)
        ecc, m0 = np.linspace(0, 0.9, ne), np.arange(nm) / nm
        bufs = [DB.from_array(a, 0) for a in (t, y, dy, ecc, m0)] + [DB(nf * 8, 0), DB(nf * 4, 0), DB(8, 0), DB(16, 0)]
        bt, by, bdy, be, bm, bp, bc, bb, ba = bufs
        ms = tm.ms(lambda: _cabi.check(lib.pdc_kepler_scan_dev(0, sp.value, bt.ptr, by.ptr, bdy.ptr, n, f0, delta, nf, be.ptr,
                                                               ne, bm.ptr, nm, 1, 0, bp.ptr, bc.ptr, None, bb.ptr, ba.ptr)),
                   reps=3)
        _cabi.check(lib.pdc_stream_sync(0, sp.value))
        best, at = bb.to_array(np.float64, 1), ba.to_array(np.int64, 2)
        solves = float(n) * nf * ne * nm
        wave_instr = solves / 64 * f64 / kc
        _, groups, launches = _cabi.kepler_last_dispatch()
        print(f"N={n:6d} nf={nf:7d} cells={ne:2d}x{nm:2d} ({groups} groups, {launches} launch): {ms:9.3f} ms  "
              f"{solves / ms / 1e6:7.2f} Gsolve/s  {wave_instr / (ms * 1e-3):.3e} fp64 wave-instr/s = "
              f"{wave_instr / (ms * 1e-3) / probe:.3f} of the probe;  best {best[0]:.4f} at bin {at[0]}, cell {at[1]}")
        for b in bufs:
            b.free()


if __name__ == "__main__":
    main()
