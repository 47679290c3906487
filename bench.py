"""Headline benchmark: fp64 generalized Lomb-Scargle, N=1e5 unevenly sampled points x 1e6 trial
frequencies per GPU (BASELINE.json configs[1]); prints ONE JSON line on rank 0.

    python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]   # one process, N devices
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W      # one rank per GPU
    python bench.py --loopback N --full                              # N logical slots on ONE device (testing)

A plain run sets up, warms up, times the K steps and prints the headline line (``value``, ``ms_per_step``, the
``roofline`` block priced from the committed PMC summary and this run's HIP-event times).  Everything measured
beyond that takes ``--full``: the same-run clock probe, the kernel time and end-to-end call of the plan path, the
FFT path, the other configs (``extras``), the CPU baselines, and with N > 1 the sharded extras and the
strong-scaling entries.  ``--dump-outputs DIR`` writes the power array of the last timed step to
``DIR/power.npy`` (float64; the inputs are seeded, so two builds can be compared output for output).

A step = one pass of the hot path over resident inputs: the weights prologue + direct-sum scan + fused
epilogue (``pdc_gls_scan_dev``) writing power[nf] in HBM.  With N > 1 each GPU scans its own
contiguous slab of an N-times longer grid (weak scaling, samples replicated) and the slabs are
all-gathered with RCCL so every GPU ends the step holding the whole power array; the gather of step
i overlaps the scan of step i+1 (double-buffered outputs, everything drained before the clock stops).

Two ways to drive N GPUs, same kernels, same collective:
  * plain ``python bench.py --gpus N``: ONE process, N devices, through the C ABI's persistent plan
    (``pdc_gls_plan_*``: hipSetDevice + two streams per device, ncclCommInitAll, grouped
    ncclAllGather) - no torch anywhere;
  * under ``torch.distributed.run`` (WORLD_SIZE > 1 in the environment): one rank per GPU, torch is
    used for rendezvous, the barrier and the RCCL all-gather only.
With N > 1 the line also carries ``extras``: the other configs sharded the way they shard - C5's period
grid in N slabs (PDM, StringLength), C3's curves in N groups - kernel-only and end to end; and the two
STRONG-scaling entries: ``c4_sharded`` = BASELINE configs[3] (N=1e6 x nf=1e7, fixed, N slabs + all-gather +
D2H of the 80 MB power array; its ``speedup_vs_1gpu`` against one slot of the same run is the north star's
">= 6x at 8 GPUs") and ``c2_strong`` (C2's own grid cut N ways).  The headline ``value`` stays weak-scaled.

The product path is the C ABI (libperiodicity_hip.so).  ``oracle/`` is touched only by the
``cpu_baseline`` legs, after the clock has stopped.

Every roofline figure in the line means one of two things, and says which:
  * ``executed_issue_frac``: VALU issue cycles per launch / 1024 SIMDs / 2.4 GHz / the HIP-event time of this
    run, the cycles priced BY INSTRUCTION TYPE from rocprofv3's typed counters (profiles/r06_pmc_summary.json,
    written by tools/pmc_summary.py for the kernel sources whose hash it records - a summary of other sources
    is refused): the fp64 / int64 classes (SQ_INSTS_VALU_{ADD,MUL,FMA,TRANS}_F64, _INT64) at 4 cycles per
    wave64 instruction, every other VALU instruction at 2 (SIMD-32); ``executed_issue.frac_all_at_4_cycles`` is
    the round-3 figure (everything at 4 cycles, an upper bound) and ``executed_issue.mix`` the counts;
  * ``algorithmic_frac``: SURVEY.md 8d's per-unit work (50 flop per GLS pair, 40 per PDM pair, one
    gathered record per StringLength pair, 8 B per spectrum bin) x units / time / the peak it is priced
    against.  It may exceed 1 where the kernel does less work than the unit assumes (rotation
    recurrences instead of a sincos per pair).
The headline ``roofline.frac`` is the executed-issue fraction.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_PAIR = 50.0            # algorithmic fp64 flop per (sample, frequency) pair
PEAK_FP64_VECTOR_TFLOPS = 78.6  # 256 CU x 4 SIMD x 16 lanes x 2 x 2.4 GHz (MI355X, spec)
SIMDS, CLOCK_HZ, FP64_ISSUE_CYCLES, B32_ISSUE_CYCLES = 1024, 2.4e9, 4, 2
# rocprofv3 counters of the VALU mix (tools/collect_pmc.sh, passes mix64 / mix32): a wave64 fp64 arithmetic
# instruction occupies its SIMD-32 for 4 cycles, a 32-bit one for 2 (MI355X_MICROARCH.md: `v_fma_f32` (wave64) 2 cyc)
F64_COUNTERS = ("SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_TRANS_F64",
                "SQ_INSTS_VALU_INT64")
PDM_FLOP_PER_PAIR = 40.0
SL_MODEL_BYTES_PER_PAIR = 48.0  # HBM bucket-pass model
HBM_PEAK_TBS = 8.0
N_SAMPLES = 100_000
NF_PER_GPU = 1_000_000
PMC_SUMMARY = os.path.join(ROOT, "profiles", "r06_pmc_summary.json")
GATHER_UBENCH = os.path.join(ROOT, "profiles", "r03_ubench_gather_rate.json")


def synth_curve(n, k=2, period=37.3):
    """SURVEY.md 8d synthetic light curve (draw order t, dy, noise)."""
    rng = np.random.default_rng(20241008 + k)
    t = np.sort(rng.uniform(0, float(n), n))
    dy = rng.uniform(0.05, 0.2, n)
    y = 1.0 + 0.5 * np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)
    return t, y, dy


def throughput_grid(t, nf):
    df = 1.0 / (t[-1] - t[0]) / 5
    fmin = 0.5 * df
    for slack in (1.5, 1.25, 1.75, 1.1, 1.9):       # dodge np.arange's length rounding
        freq = np.arange(fmin, fmin + (nf - slack) * df + df, df)
        if freq.size == nf:
            return freq, df, fmin
    raise AssertionError((freq.size, nf))


def c3_batch():
    """BASELINE configs[2]: 4096 curves x 2000 samples, each its own seeded (t, y, dy), one shared grid."""
    B, n, nf = 4096, 2000, 50_000
    rng = np.random.default_rng(20241008 + 3)
    tt = np.sort(rng.uniform(0, float(n), (B, n)), axis=1)
    dd = rng.uniform(0.05, 0.2, (B, n))
    pp = (5.0 + 0.01 * np.arange(B))[:, None]
    yy = 1.0 + 0.5 * np.sin(2 * np.pi * tt / pp) + dd * rng.standard_normal((B, n))
    df = 1.0 / n / 5
    f = np.arange(0.5 * df, 0.5 * df + (nf - 1.5) * df + df, df)
    assert f.size == nf
    return tt, yy, dd, f


def c5_inputs():
    """BASELINE configs[4]: N=5e4 samples x 1e5 trial periods for PDM and StringLength."""
    n, n_per = 50_000, 100_000
    t5, y5, _ = synth_curve(n, 5, period=13.7)
    periods = np.linspace(1.0, 100.0, n_per)
    vmax, vmin = y5.max(), y5.min()
    m = (y5 - vmax) / (2 * (vmax - vmin)) + 0.25
    dfp = 0.1 / (t5[-1] - t5[0])
    sl_periods = 1 / np.linspace(n_per * dfp, dfp, n_per)
    return t5, y5, m, periods, sl_periods


# which sources a profiled kernel was built from: a PMC summary entry is refused once any of them changed
KERNEL_SOURCES = {
    "gls_": ("gls.hip", "gls_epilogue.h", "pdc_device.h"),
    "pdm_": ("pdm.hip", "pdc_device.h"),
    "sl_": ("stringlength.hip", "sl_ranges.inc", "supersmoother.inc", "timesort.inc", "pdc_device.h"),
    "ss_": ("stringlength.hip", "supersmoother.inc", "timesort.inc", "pdc_device.h"),
    "fft_": ("glsfft.hip", "pdc_device.h"),
    "glsfft_": ("glsfft.hip", "gls_epilogue.h", "pdc_device.h"),
    "peak": ("peaks.hip", "pdc_device.h"),
}


def file_sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def source_hashes():
    """sha256 (first 16 hex digits) of every kernel source; tools/pmc_summary.py stores the same."""
    src = os.path.join(ROOT, "periodicity_amd", "csrc")
    return {name: file_sha(os.path.join(src, name))
            for name in sorted(os.listdir(src)) if name.endswith((".hip", ".h", ".inc"))}


def sources_of(kernel_name):
    for prefix, files in KERNEL_SOURCES.items():
        if prefix in kernel_name:
            return files
    return tuple(source_hashes())


def pmc_for(kernel_substr, measured_ms):
    """Counters of the profiled kernel whose name contains `kernel_substr` and whose profiled duration
    is closest to this run's; (None, reason) when the summary is absent or was collected for other
    sources of that kernel."""
    rel = os.path.relpath(PMC_SUMMARY, ROOT)
    if not os.path.isfile(PMC_SUMMARY):
        return None, f"{rel} is missing"
    summ = json.load(open(PMC_SUMMARY))
    now, then = source_hashes(), summ.get("src_sha", {})
    best = None
    parts = (kernel_substr,) if isinstance(kernel_substr, str) else tuple(kernel_substr)
    for name, k in summ.get("kernels", {}).items():
        if all(p in name for p in parts) and "SQ_INSTS_VALU" in k and k.get("ms"):
            d = abs(k["ms"] - measured_ms) / measured_ms
            if best is None or d < best[0]:
                best = (d, name, k)
    if best is None or best[0] > 0.25:
        return None, f"no profiled '{' ... '.join(parts)}' launch within 25% of {measured_ms:.3f} ms"
    changed = [f for f in sources_of(best[1]) if now.get(f) != then.get(f)]
    if changed:
        return None, f"{rel} was collected before {', '.join(changed)} changed: refused as stale"
    return dict(best[2], name=best[1]), None


def profiled_ms_of(kernel_substr):
    """Duration of the longest profiled launch of a kernel (None without a summary)."""
    if not os.path.isfile(PMC_SUMMARY):
        return None
    ms = [k["ms"] for name, k in json.load(open(PMC_SUMMARY)).get("kernels", {}).items()
          if kernel_substr in name and "SQ_INSTS_VALU" in k and k.get("ms")]
    return max(ms) if ms else None


def valu_issue_block(kernel_substr, kernel_ms):
    k, why = pmc_for(kernel_substr, kernel_ms)
    if k is None:
        return None, why
    # issue cycles by instruction type: the typed fp64 / int64 classes at 4 cycles, every other VALU instruction
    # at 2.  The classes the counters do not name (v_cmp_f64, v_floor/fract_f64, 64-bit moves ...) fall in "other" and
    # are priced at 2: the weighted figure is a LOWER bound of the slots taken, the all-at-4 one an upper bound.
    total = k["SQ_INSTS_VALU"]
    have_mix = all(c in k for c in F64_COUNTERS)
    n64 = sum(k[c] for c in F64_COUNTERS) if have_mix else None
    cycles = (n64 * FP64_ISSUE_CYCLES + (total - n64) * B32_ISSUE_CYCLES) if have_mix else total * FP64_ISSUE_CYCLES
    busy_s = cycles / SIMDS / CLOCK_HZ
    upper_s = total * FP64_ISSUE_CYCLES / SIMDS / CLOCK_HZ
    out = {"kernel": k["name"], "valu_wave_instr_per_launch": total,
           "frac": round(busy_s / (kernel_ms * 1e-3), 4),
           "frac_all_at_4_cycles": round(upper_s / (kernel_ms * 1e-3), 4),
           "priced": "typed mix: fp64/int64 classes x 4 cycles, all other VALU x 2" if have_mix
                     else "no typed counters in the summary: every VALU instruction x 4 cycles (upper bound)",
           "profiled_ms": k["ms"], "source": os.path.relpath(PMC_SUMMARY, ROOT)}
    if have_mix:
        out["mix"] = {"fp64_or_int64": n64, "other": total - n64, "fp64_share": round(n64 / total, 4),
                      **{c.replace("SQ_INSTS_VALU_", "").lower(): k[c] for c in F64_COUNTERS + ("SQ_INSTS_VALU_INT32", "SQ_INSTS_VALU_CVT")
                         if c in k}}
    if k.get("GRBM_GUI_ACTIVE"):
        # the chip is power-limited under fp64 load: the clock the PROFILED launch actually ran at (GRBM_GUI_ACTIVE
        # summed over 8 XCDs / 8 / its duration) and the issue fraction of that launch at that clock
        clk = k["GRBM_GUI_ACTIVE"] / 8.0 / (k["ms"] * 1e-3)
        out["profiled_clock_GHz"] = round(clk / 1e9, 3)
        out["frac_at_profiled_clock"] = round(cycles / SIMDS / clk / (k["ms"] * 1e-3), 4)
    for key in ("hbm_bytes", "SQ_INSTS_LDS", "SQ_INSTS_SALU", "SQ_INSTS_VMEM", "SQ_LDS_BANK_CONFLICT",
                "SQ_LDS_IDX_ACTIVE", "TCP_TCC_READ_REQ_sum"):
        if key in k:
            out[key] = k[key]
    return out, None


def executed_flops(blk, kernel_ms):
    """fp64 flops the kernel EXECUTED per second, from the typed counters of its profiled launch: (2 x FMA_F64 +
    ADD_F64 + MUL_F64) wave instructions x 64 lanes / this run's kernel time.  Not the issue-slot figure (`frac`
    prices every fp64 instruction at 4 cycles whether it is an fma or a mul) and not SURVEY 8d's 50 flop per pair
    (`algorithmic`): the arithmetic that actually went through the DP units."""
    mix = (blk or {}).get("mix")
    if not mix or not all(k in mix for k in ("fma_f64", "add_f64", "mul_f64")):
        return None
    flops = (2.0 * mix["fma_f64"] + mix["add_f64"] + mix["mul_f64"]) * 64.0
    tf = flops / (kernel_ms * 1e-3) / 1e12
    return {"TFLOPs": round(tf, 2), "frac_of_peak": round(tf / PEAK_FP64_VECTOR_TFLOPS, 4), "flop_per_launch": flops,
            "counted": "(2 x SQ_INSTS_VALU_FMA_F64 + ADD_F64 + MUL_F64) x 64 lanes of the profiled launch / this run's kernel time"}


def two_fracs(kernel_substr, ms, algorithmic_frac, unit):
    """The two roofline fields every entry of the line carries (module docstring)."""
    blk, why = valu_issue_block(kernel_substr, ms)
    out = {"executed_issue_frac": blk["frac"] if blk else None,
           "algorithmic_frac": None if algorithmic_frac is None else round(algorithmic_frac, 4),
           "algorithmic_unit": unit}
    if blk:
        out["executed_issue"] = {k: blk[k] for k in ("kernel", "valu_wave_instr_per_launch", "priced", "mix",
                                                     "frac_all_at_4_cycles", "profiled_ms", "source",
                                                     "profiled_clock_GHz", "frac_at_profiled_clock") if k in blk}
    else:
        out["executed_issue_note"] = why
    return out, blk


def fft_path_roofline(n, nf, ms, ngrid=3):
    """`roofline` block of the device FFT-extirpolation path (HBM-bound: every Stockham pass streams the
    grid).  Algorithmic bytes of one pdc_gls_scan_fft_dev launch: per grid the deposits write the live cells L (the
    part of the 2^k grid the samples reach: 1/5 at five samples per peak), pass 1 reads L and writes nfft, the
    middle passes read and write nfft, the last pass reads nfft and writes the nf outputs that are kept
    (spectral.py:34 `[:nf]`), 16 B a cell; the epilogue reads ngrid x nf cells and writes nf doubles; the samples
    are read twice (prologue, deposits).  `traffic` = HBM-side bytes of the path's kernels from the PMC summary
    (FETCH_SIZE x 2 + WRITE_SIZE per dispatch x dispatches per launch; the 256 MiB Infinity Cache holds one grid's
    ping-pong at C2, so traffic may lie BELOW the algorithmic bytes)."""
    nfft = 1 << int(nf * 5 - 1).bit_length()
    bits = nfft.bit_length() - 1
    passes = -(-bits // 8)
    live = min(nfft, nfft // 5 + 4)
    per_grid = 16.0 * (live + (live + nfft) + 2.0 * nfft * max(0, passes - 2) + (nfft + nf))
    algo = ngrid * per_grid + 16.0 * ngrid * nf + 8.0 * nf + 2 * 24.0 * n
    gbps = algo / (ms * 1e-3) / 1e9
    out = {"bound": "hbm", "achieved": round(gbps, 1), "peak": HBM_PEAK_TBS * 1000, "unit": "GB/s",
           "frac": round(gbps / (HBM_PEAK_TBS * 1000), 4), "algorithmic_bytes": algo, "passes_per_grid": passes,
           "grids": ngrid, "nfft": nfft, "traffic": None}
    if os.path.isfile(PMC_SUMMARY):
        summ = json.load(open(PMC_SUMMARY))
        now, then = source_hashes(), summ.get("src_sha", {})
        stale = [f for f in KERNEL_SOURCES["glsfft_"] if now.get(f) != then.get(f)]
        ks = {name: k for name, k in summ.get("kernels", {}).items()
              if ("fft_pass" in name or "glsfft_" in name) and "hbm_bytes" in k}
        epi = [k for name, k in ks.items() if name.startswith("glsfft_epilogue_kernel") and
               name.endswith(f"grid={-(-nf // 256) * 256}")]
        if stale:
            out["traffic_note"] = f"{os.path.relpath(PMC_SUMMARY, ROOT)} predates {', '.join(stale)}: refused as stale"
        elif epi and epi[0].get("dispatches_per_pass"):
            launches = epi[0]["dispatches_per_pass"]
            per_kernel = {name: {"dispatches_per_launch": k["dispatches_per_pass"] / launches, "hbm_bytes_per_dispatch": k["hbm_bytes"],
                                 "ms_per_dispatch": k["ms"]} for name, k in ks.items() if k["dispatches_per_pass"] % launches == 0}
            out["traffic"] = int(sum(v["dispatches_per_launch"] * v["hbm_bytes_per_dispatch"] for v in per_kernel.values()))
            out["traffic_GBps"] = round(out["traffic"] / (ms * 1e-3) / 1e9, 1)
            out["traffic_by_kernel"] = per_kernel
        else:
            out["traffic_note"] = "no profiled glsfft_epilogue_kernel launch of this grid in the PMC summary"
    return out


def gls_algorithmic_frac(pairs, ms):
    return pairs * FLOP_PER_PAIR / (ms * 1e-3) / 1e12 / PEAK_FP64_VECTOR_TFLOPS


def pdm_algorithmic_frac(pairs, ms):
    return pairs * PDM_FLOP_PER_PAIR / (ms * 1e-3) / 1e12 / PEAK_FP64_VECTOR_TFLOPS


def l2_gather_ceiling():
    """Random 16-byte gathers per second the chip serves from an L2-resident table, as measured by
    tools/ubench/gather_rate.hip and summarised (with the sha256 of that source) by tools/ubench_summary.py;
    (None, reason) when the summary is absent or belongs to another version of the micro-benchmark."""
    rel = os.path.relpath(GATHER_UBENCH, ROOT)
    if not os.path.isfile(GATHER_UBENCH):
        return None, f"{rel} is missing"
    u = json.load(open(GATHER_UBENCH))
    src = os.path.join(ROOT, "tools", "ubench", "gather_rate.hip")
    if u.get("src_sha") != file_sha(src):
        return None, f"{rel} was measured with another tools/ubench/gather_rate.hip: refused as stale"
    return float(u["gather_16B_per_s"]), None


def host_cores():
    return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)


def cpu_baseline(t, y, dy, freq, df, fmin):
    """The reference's own CPU algorithm (FFT/extirpolation, single-threaded numpy as upstream),
    restated in oracle/scan_oracle.py, on the full N=1e5 x nf=1e6 workload and at C1 / C4 (SURVEY.md
    8d (i)); plus the exact direct sum (the arithmetic the GPU kernel does) on a bounded sample, all
    host cores (8d (ii))."""
    from oracle import c_oracle as co
    from oracle import scan_oracle as so
    t0 = time.perf_counter()
    p_fft = so.gls_power(t, y, dy, freq, df, fmin, True, False, sums="fft")
    dt_fft = time.perf_counter() - t0
    cores = host_cores()
    co.set_threads(cores)
    n_s, nf_s = 10_000, 8 * cores
    t0 = time.perf_counter()
    co.trig_sums_exact(t[:n_s], dy[:n_s], freq[:nf_s])      # calibration pass (also warms OpenMP)
    probe = max(time.perf_counter() - t0, 1e-3)
    nf_s = int(min(freq.size, max(nf_s, nf_s * 6.0 / probe)))  # aim at ~6 s of CPU work
    t0 = time.perf_counter()
    co.trig_sums_exact(t[:n_s], dy[:n_s], freq[:nf_s])
    dt_direct = time.perf_counter() - t0
    base = {
        "value": round(t.size * freq.size / dt_fft / 1e9, 3), "unit": "Gpair/s (effective)",
        "cores": 1, "kind": "port",
        "sample": f"full workload N={t.size} x nf={freq.size}, one pass of the reference's "
                  f"O(nfft log nfft) FFT-extirpolation path in numpy: {dt_fft:.2f} s",
        "direct_sum": {"value": round(n_s * nf_s / dt_direct / 1e9, 4), "unit": "Gpair/s",
                       "cores": cores, "kind": "port",
                       "sample": f"long-double direct sums, N={n_s} x nf={nf_s} "
                                 f"(one trig-sum pair), OpenMP: {dt_direct:.2f} s"},
    }
    # the same single-threaded FFT-path restatement at C1 (1k x 1k) and C4 (1e6 x 1e7: three 1-GiB grids)
    other = {}
    for key, n_c, nf_c, k in (("c1", 1000, 1000, 1), ("c4", 1_000_000, 10_000_000, 4)):
        tc, yc, dyc = synth_curve(n_c, k)
        fc, dfc, fminc = throughput_grid(tc, nf_c)
        reps = 20 if key == "c1" else 1
        t0 = time.perf_counter()
        for _ in range(reps):
            pc = so.gls_power(tc, yc, dyc, fc, dfc, fminc, True, False, sums="fft")
        dt = (time.perf_counter() - t0) / reps
        other[key] = {"seconds": round(dt, 5), "effective_Gpair_per_s": round(n_c * nf_c / dt / 1e9, 2),
                      "cores": 1, "kind": "port", "peak_bin": int(np.nanargmax(pc)),
                      "sample": f"full workload N={n_c} x nf={nf_c}, FFT-extirpolation path in numpy"}
        del pc, fc
    base["fft_path_other_configs"] = other
    return base, p_fft


def cpu_pool_baseline(cores):
    """the phase scans under multiprocessing.Pool(all cores) as upstream runs them, in
    a child process that never touches the GPU (tools/cpu_pool_baseline.py)."""
    sub = max(2000, 16 * cores)
    try:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cpu_pool_baseline.py"), str(sub), str(cores)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        res = json.loads(run.stdout.strip().splitlines()[-1])
    except Exception as exc:                                  # the baseline is informational: never fail the bench
        return {"error": f"{type(exc).__name__}: {exc}"}
    res["kind"] = "port"
    res["sample"] = (f"{sub} of 100000 trial periods of C5 (N=5e4), numpy restatement of _pdm / _stringlength under "
                     f"multiprocessing.Pool({cores}).map as phase.py:69-70,185-186; map time scaled linearly")
    return res


class EventTimer:
    """HIP events on the stream the kernels are launched on."""

    def __init__(self, lib, cabi, dev, stream):
        self.lib, self.cabi, self.dev, self.stream = lib, cabi, dev, stream
        self.ev = [self._new(), self._new()]

    def _new(self):
        e = C.c_void_p()
        self.cabi.check(self.lib.pdc_event_create(self.dev, C.byref(e)))
        return e.value

    def ms(self, fn, reps=3, warm=1):
        for _ in range(warm):
            fn()
        out = []
        for _ in range(reps):
            self.cabi.check(self.lib.pdc_event_record(self.dev, self.ev[0], self.stream))
            fn()
            self.cabi.check(self.lib.pdc_event_record(self.dev, self.ev[1], self.stream))
            ms = C.c_float()
            self.cabi.check(self.lib.pdc_event_elapsed_ms(self.dev, self.ev[0], self.ev[1], C.byref(ms)))
            out.append(ms.value)
        return float(np.median(out))


def host_api_small(with_cpu=True, reps=25):
    """Wall clock of the CLASS calls at the sizes the reference's own tests and bundled data have (every one of them
    100 ... 74 326 samples: /root/reference/tests/test_spectral.py:7-31, src/periodicity/data/__init__.py:6-46) - the
    sizes at which a drop-in is actually dropped in -, median of `reps` calls after three warm-up calls, and the
    reference's CPU path at the same size beside each (GLS: the single-threaded numpy FFT-extirpolation restatement
    `so.gls`; the phase scans: `multiprocessing.Pool(all cores).map` of the numpy restatement, one Pool per call as
    phase.py:69-70,185-186, in a child process)."""
    from periodicity_amd.core import TSeries
    from periodicity_amd.phase import PDM, StringLength
    from periodicity_amd.spectral import GLS

    def median_ms(fn, k=reps):
        for _ in range(3):
            fn()
        w = []
        for _ in range(k):
            ta = time.perf_counter()
            fn()
            w.append(time.perf_counter() - ta)
        return round(float(np.median(w)) * 1e3, 4), round(float(np.min(w)) * 1e3, 4)

    out = {}
    # C1: BASELINE configs[0], SURVEY 8d's inputs
    t, y, dy = synth_curve(1000, 1)
    freq, df, fmin = throughput_grid(t, 1000)
    fmax = fmin + (1000 - 1.5) * df
    sig = TSeries(t, y)
    ms, lo = median_ms(lambda: GLS(fmin=fmin, fmax=fmax)(sig, dy))
    ms_f, lo_f = median_ms(lambda: GLS(fmin=fmin, fmax=fmax, method="fft")(sig, dy))
    out["c1_end_to_end"] = {"n_samples": 1000, "n_freq": 1000, "class_call_ms": ms, "class_call_min_ms": lo,
                            "class_call_fft_method_ms": ms_f, "what": "GLS(fmin, fmax)(TSeries(t, y), dy): grid + H2D + kernels + D2H + FSeries"}
    # SpottedStar's shape (N = 2148, default grid nf = 5680): the curve itself travels as a golden fixture's INPUT
    g3 = os.path.join(ROOT, "tests", "golden", "g3_spotted_star.npz")
    if os.path.isfile(g3):
        g = np.load(g3)
        ts, ys, dys, src = g["t"], g["y"], g["dy"], "tests/golden/g3_spotted_star.npz (the reference's bundled curve)"
    else:
        ts, ys, dys = synth_curve(2148, 3)
        src = "synthetic, 2148 samples"
    sig_s = TSeries(ts, ys)
    ms, lo = median_ms(lambda: GLS()(sig_s, dys))
    nf_s = GLS()(sig_s, dys).size
    out["spotted_star_end_to_end"] = {"n_samples": int(ts.size), "n_freq": int(nf_s), "class_call_ms": ms, "class_call_min_ms": lo,
                                      "data": src, "what": "GLS()(TSeries(t, y), dy) on the default grid"}
    # SunSpots size (74 326 samples), the phase classes' defaults (1000 periods each)
    n_ss = 74_326
    tl, yl, _ = synth_curve(n_ss, 5, period=13.7)
    sig_l = TSeries(tl, yl)
    ms_sl, lo_sl = median_ms(lambda: StringLength()(sig_l), 20)
    ms_pdm, lo_pdm = median_ms(lambda: PDM()(sig_l), 20)
    out["sunspots_size_stringlength_defaults"] = {"n_samples": n_ss, "n_periods": 1000, "class_call_ms": ms_sl, "class_call_min_ms": lo_sl,
                                                  "what": "StringLength()(TSeries(t, y)): scaling + grid + H2D + kernels + D2H + FSeries"}
    out["sunspots_size_pdm_defaults"] = {"n_samples": n_ss, "n_periods": 1000, "class_call_ms": ms_pdm, "class_call_min_ms": lo_pdm,
                                         "what": "PDM()(TSeries(t, y))"}
    if with_cpu:
        from oracle import scan_oracle as so
        cpu, _ = median_ms(lambda: so.gls(t, y, dy, fmin=fmin, fmax=fmax), 20)
        out["c1_end_to_end"].update({"cpu_reference_path_ms": cpu, "cpu_cores": 1, "cpu_kind": "port",
                                     "class_call_vs_cpu": round(cpu / out["c1_end_to_end"]["class_call_ms"], 2)})
        cpu, _ = median_ms(lambda: so.gls(ts, ys, dys), 20)
        out["spotted_star_end_to_end"].update({"cpu_reference_path_ms": cpu, "cpu_cores": 1, "cpu_kind": "port",
                                               "class_call_vs_cpu": round(cpu / out["spotted_star_end_to_end"]["class_call_ms"], 2)})
        cores = host_cores()
        try:
            run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cpu_pool_baseline.py"), "defaults", str(n_ss), str(cores)],
                                 capture_output=True, text=True, timeout=600, cwd=ROOT)
            res = json.loads(run.stdout.strip().splitlines()[-1])
            for key, name in (("sunspots_size_stringlength_defaults", "stringlength"), ("sunspots_size_pdm_defaults", "pdm")):
                out[key].update({"cpu_pool_wall_ms": round(res[name]["wall_s"] * 1e3, 1), "cpu_cores": cores, "cpu_kind": "port",
                                 "class_call_vs_cpu": round(res[name]["wall_s"] * 1e3 / out[key]["class_call_ms"], 1)})
        except Exception as exc:                              # informational: never fail the bench
            out["sunspots_cpu_error"] = f"{type(exc).__name__}: {exc}"
    return out


def extra_configs(lib, cabi, dev, stream, t2, y2, dy2, f0, delta, nf2, with_cpu=True):
    """Kernel-level numbers of the other single-GPU configs (BASELINE.json configs[2], [4]) and the
    PCIe-inclusive rate of the headline config, so that they appear in the driver's record."""
    tm = EventTimer(lib, cabi, dev, stream)
    DB = cabi.DeviceBuffer
    out = {}

    # -- C2 end to end: host buffers in, host buffer out (H2D + prologue + scan + D2H) -------------
    t0 = time.perf_counter()
    cabi.gls_scan(t2, y2, dy2, f0, delta, nf2, device=dev)            # first call sizes the cached workspace
    t1 = time.perf_counter()
    walls = []
    for _ in range(3):
        ta = time.perf_counter()
        cabi.gls_scan(t2, y2, dy2, f0, delta, nf2, device=dev)
        walls.append(time.perf_counter() - ta)
    t2_ = t1 + float(np.median(walls))
    e2e_ms = (t2_ - t1) * 1e3
    fr, _ = two_fracs("gls_scan_kernel", e2e_ms, gls_algorithmic_frac(float(t2.size) * nf2, e2e_ms),
                      "50 flop/pair vs 78.6 TFLOP/s")
    out["c2_end_to_end"] = {"ms": round(e2e_ms, 3), "first_call_ms": round((t1 - t0) * 1e3, 3),
                            "Gpair_per_s": round(t2.size * nf2 / (t2_ - t1) / 1e9, 1), **fr,
                            "note": "pdc_gls_scan on host buffers: H2D of (t, y, dy) + prologue + scan + "
                                    "D2H of power[1e6], wall clock, median of three calls (both fractions priced on the wall time)"}

    # -- BGLST at C2's shape (round 6): gls_scan_kernel<8, MODE_TREND, 1> - eight running sums per pair + the marginal
    # log-likelihood as epilogue -, inputs resident
    try:
        from periodicity_amd.spectral import BGLST
        sc = BGLST._scalars(t2, y2, dy2, 1.0, 1.0, 2.0, 0.5 * (t2[0] + t2[-1]))
        bb = [DB.from_array(a_, dev) for a_ in (t2, y2, dy2)]
        wbb = lib.pdc_gls_work_bytes(t2.size, 1, nf2)
        bw, bo = DB(wbb, dev), DB(nf2 * 8, dev)
        ms = tm.ms(lambda: cabi.check(lib.pdc_bglst_scan_dev(dev, stream, bb[0].ptr, bb[1].ptr, bb[2].ptr, t2.size, f0, delta, 0, nf2,
                                                             sc.ctypes.data_as(C.c_void_p), bo.ptr, bw.ptr, wbb)), reps=3)
        ll = bo.to_array(np.float64, nf2)
        fr, _ = two_fracs(("gls_scan_kernel<8, 3, 1",), ms, float(t2.size) * nf2 * 54.0 / (ms * 1e-3) / 1e12 / PEAK_FP64_VECTOR_TFLOPS,
                          "54 flop/pair (SURVEY 8d's 50 + two more fmas) vs 78.6 TFLOP/s")
        out["c2_bglst"] = {"ms": round(ms, 3), "Gpair_per_s": round(t2.size * nf2 / ms / 1e6, 1), "peak_bin": int(np.nanargmax(ll)), **fr,
                           "note": "pdc_bglst_scan_dev on the C2 inputs: Bayesian GLS with linear trend (the reference exports the name "
                                   "for an empty class, spectral.py:207-208); parity unpinned by the reference, oracle = the published "
                                   "marginal likelihood"}
        for b_ in bb + [bw, bo]:
            b_.free()
    except Exception as exc:                                  # informational: never cost the headline line
        out["c2_bglst"] = {"error": f"{type(exc).__name__}: {exc}"}

    # -- the reference's OWN sizes through the classes (round 6): wall clock of the class call, the CPU path beside it
    out["host_api_small"] = host_api_small(with_cpu)

    # -- C3: 4096 light curves x 2000 samples, shared 5e4-frequency grid ---------------------------
    tt, yy, dd, f = c3_batch()
    B, n = tt.shape
    nf = f.size
    offsets = np.arange(B + 1, dtype=np.int64) * n
    g0, gd, _ = cabi.grid_params(f)
    bt, by, bdy, boff = DB.from_array(tt, dev), DB.from_array(yy, dev), DB.from_array(dd, dev), DB.from_array(offsets, dev)
    bt0 = DB.from_array(tt[0], dev)
    wb = lib.pdc_gls_work_bytes(B * n, B, nf)
    work = DB(wb, dev)
    power = DB(B * nf * 8, dev)
    amax, arg = DB(B * 8, dev), DB(B * 8, dev)
    pairs = float(B) * n * nf

    def c3(shared, peaks_only):
        def fn():
            cabi.check(lib.pdc_gls_scan_dev(dev, stream, bt0.ptr if shared else bt.ptr, by.ptr, bdy.ptr,
                                            boff.ptr, B * n, B, int(shared), g0, gd, 0, nf, 1, 0,
                                            None if peaks_only else power.ptr,
                                            amax.ptr if peaks_only else None,
                                            arg.ptr if peaks_only else None, work.ptr, wb))
        return fn
    for key, shared, peaks, kern in (("c3_power", False, False, "gls_scan_kernel"),
                                     ("c3_peaks_only", False, True, "gls_scan_kernel"),
                                     ("c3_shared_t_peaks_only", True, True, "gls_shared")):
        ms = tm.ms(c3(shared, peaks), reps=3)
        fr, _ = two_fracs(kern, ms, gls_algorithmic_frac(pairs, ms), "50 flop/(pair, curve) vs 78.6 TFLOP/s")
        out[key] = {"ms": round(ms, 3), "Gpair_per_s": round(pairs / ms / 1e6, 1), **fr}
    # ranked peaks with prominences + half-maximum crossings of the 4096 resident spectra (f3)
    k = 4
    pk = DB(B * (1 + 5 * k) * 8, dev)
    p_cnt = pk.ptr
    p_idx, p_lo, p_hi = p_cnt + B * 8, p_cnt + B * 8 * (1 + k), p_cnt + B * 8 * (1 + 2 * k)
    p_h, p_p = p_cnt + B * 8 * (1 + 3 * k), p_cnt + B * 8 * (1 + 4 * k)
    ms = tm.ms(lambda: cabi.check(lib.pdc_peaks_topk_dev(dev, stream, power.ptr, B, nf, k, 1, p_cnt, p_idx, p_h, p_p,
                                                         p_lo, p_hi)), reps=5)
    ms_h = tm.ms(lambda: cabi.check(lib.pdc_peaks_topk_dev(dev, stream, power.ptr, B, nf, k, 0, p_cnt, p_idx, p_h, p_p,
                                                           p_lo, p_hi)), reps=5)
    gbps = B * nf * 8 / ms / 1e6
    fr, _ = two_fracs("peaks_topk_kernel", ms, gbps / (HBM_PEAK_TBS * 1000), "8 B per spectrum bin read once vs 8 TB/s HBM")
    out["c3_peaks_topk"] = {"ms": round(ms, 3), "k": k, "by": "prominence", "ms_by_height": round(ms_h, 3),
                            "GBps_over_spectra": round(gbps, 1), **fr,
                            "algorithmic_frac_by_height": round(B * nf * 8 / ms_h / 1e6 / (HBM_PEAK_TBS * 1000), 4),
                            "roofline": {"bound": "hbm", "achieved": round(gbps, 1), "peak": HBM_PEAK_TBS * 1000,
                                         "unit": "GB/s", "frac": round(gbps / (HBM_PEAK_TBS * 1000), 4),
                                         "algorithmic_bytes": B * nf * 8,
                                         "note": "algorithmic bytes = the spectra read once (8 B per bin); by "
                                                 "prominence a second sweep re-reads the chunks that hold candidates"},
                            "note": "pdc_peaks_topk_dev on the 1.64 GB of spectra left in HBM by c3_power: "
                                    "find_peaks maxima, scipy prominences, 4 most prominent + half-maximum "
                                    "crossings per curve; 0.8 MB come back instead of 1.64 GB"}
    pk.free()
    out["c3_note"] = ("BASELINE configs[2]: 4096 curves x 2000 samples x 5e4 shared frequencies, resident; "
                      "power = 1.64 GB of spectra written; peaks_only = per-curve amax/argmax reduced on "
                      "the device; shared_t = the bootstrap shape (one time axis, trigonometry shared "
                      "between curves)")
    for b in (bt, by, bdy, boff, bt0, work, power, amax, arg):
        b.free()

    # -- C5: PDM and StringLength, N=5e4 x 1e5 trial periods ----------------------------------------
    t5, y5, m, periods, sl_periods = c5_inputs()
    n, n_per = t5.size, periods.size
    bt5 = DB.from_array(t5, dev)
    pairs = float(n) * n_per
    bx, bp, bth = DB.from_array(y5, dev), DB.from_array(periods, dev), DB(n_per * 8, dev)
    sigma = float(np.var(y5, ddof=1))
    ms = tm.ms(lambda: cabi.check(lib.pdc_pdm_scan_dev(dev, stream, bt5.ptr, bx.ptr, n, bp.ptr, n_per, 5, 2,
                                                       sigma, bth.ptr)), reps=5)
    fr, _ = two_fracs(("pdm_scan_kernel<", ", 0> grid"), ms, pdm_algorithmic_frac(pairs, ms), "40 flop/pair vs 78.6 TFLOP/s")
    ach = pairs * PDM_FLOP_PER_PAIR / ms / 1e9
    out["c5_pdm"] = {"ms": round(ms, 4), "Gpair_per_s": round(pairs / ms / 1e6, 1), **fr,
                     "roofline": {"bound": "valu", "achieved": round(ach, 2), "peak": PEAK_FP64_VECTOR_TFLOPS,
                                  "unit": "TFLOP/s", "frac": round(ach / PEAK_FP64_VECTOR_TFLOPS, 4),
                                  "note": "40 algorithmic fp64 flop per (sample, period) pair (SURVEY 8d)"}}
    bm, bsp, be = DB.from_array(m, dev), DB.from_array(sl_periods, dev), DB(n_per * 8, dev)
    swb = lib.pdc_stringlength_work_bytes(n, n_per)
    swork = DB(swb, dev)
    ms = tm.ms(lambda: cabi.check(lib.pdc_stringlength_scan_dev(dev, stream, bt5.ptr, bm.ptr, n, bsp.ptr, n_per,
                                                                be.ptr, swork.ptr, swb)), reps=5)
    ceiling, why_c = l2_gather_ceiling()
    floor_ms = None if ceiling is None else pairs / ceiling * 1e3
    fr, _ = two_fracs("sl_fast_kernel", ms, None if floor_ms is None else floor_ms / ms,
                      "one gathered 16-byte (t, m) record per pair vs the measured L2 random-gather rate")
    out["c5_stringlength"] = {
        "ms": round(ms, 4), "Gpair_per_s": round(pairs / ms / 1e6, 1), **fr,
        "roofline": {"bound": "l2-gather", "achieved": round(pairs / ms / 1e6, 1),
                     "peak": None if ceiling is None else round(ceiling / 1e9, 1),
                     "unit": "G gathered records/s", "frac": None if floor_ms is None else round(floor_ms / ms, 4),
                     "ceiling_source": os.path.relpath(GATHER_UBENCH, ROOT) if ceiling else why_c,
                     "note": "a sort by phase gathers one 16-byte (t, m) record per (sample, period) pair "
                             "from an L2-resident table; random accesses are served at one rate chip-wide "
                             "whatever their width (tools/ubench/gather_rate.hip)"},
        "survey_hbm_model": {"bytes_per_pair": SL_MODEL_BYTES_PER_PAIR,
                             "achieved_TBps": round(pairs * SL_MODEL_BYTES_PER_PAIR / ms / 1e9, 2),
                             "frac_of_8TBps": round(pairs * SL_MODEL_BYTES_PER_PAIR / ms / 1e9 / HBM_PEAK_TBS, 3),
                             "note": "SURVEY 8d's HBM bucket-pass model (48 B/pair); the kernel sorts in LDS "
                                     "and moves none of these bytes through HBM, so this may exceed 1"}}
    # -- StringLength where real data lives: the reference's bundled SunSpots curve has 74 326 samples (several LDS
    # slices per period), and N = 1e6 takes the streamed kernels (counting sort by phase bin through HBM, no gathers)
    for key, n_l, np_l, kern, what in (
            ("sl_sunspots_size", 74_326, 20_000, "sl_fast_kernel", "the several-slice kernel (N > 52 112: one period no longer fits one LDS slice)"),
            ("sl_sunspots_reference_defaults", 74_326, 1000, "sl_fast_kernel",
             "the reference's own defaults (n_periods = 1000, dphi = 0.1, phase.py:38) at the size of its bundled SunSpots curve: ten of "
             "the 1000 periods outlast the samples and are summed without a sort (one-cycle pre-pass)"),
            ("sl_streamed_1e6", 1_000_000, 2048, "sl_sort_kernel", "the streamed kernels, slices mode: histogram -> bin table -> table of the (cycle, bin) cells' first samples -> LDS sort per bin, records fetched as slices of t / m -> links")):
        tl, yl, _ = synth_curve(n_l, 5, period=13.7)
        ml = (yl - yl.max()) / (2 * (yl.max() - yl.min())) + 0.25
        dfl = 0.1 / (tl[-1] - tl[0])
        pl = 1 / np.linspace(np_l * dfl, dfl, np_l)
        bl = [DB.from_array(a_, dev) for a_ in (tl, ml, pl)]
        bel = DB(np_l * 8, dev)
        wbl = lib.pdc_stringlength_work_bytes(n_l, np_l)
        wl = DB(wbl, dev)
        ms = tm.ms(lambda: cabi.check(lib.pdc_stringlength_scan_dev(dev, stream, bl[0].ptr, bl[1].ptr, n_l, bl[2].ptr, np_l,
                                                                    bel.ptr, wl.ptr, wbl)), reps=3)
        pairs_l = float(n_l) * np_l
        entry = {"ms": round(ms, 3), "Gpair_per_s": round(pairs_l / ms / 1e6, 1), "n_samples": n_l, "n_periods": np_l,
                 "per_pair_vs_c5": round((ms / pairs_l) / (out["c5_stringlength"]["ms"] / pairs), 3), "note": what}
        if key == "sl_streamed_1e6":
            # Slices mode (t non-decreasing): no record passes through HBM - t is read by the histogram and the boundary
            # kernel, t and m by the sort kernel, 32 bytes per pair from L2 / the Infinity Cache; the sort kernel (3/4 of
            # the time) is bound by VALU issue and LDS latency.  Its issue fraction is that of its longest PROFILED launch
            # (five kernels per batch of periods: no single launch of this run to price).
            k_ms = profiled_ms_of("sl_sort_kernel")
            blk, why = valu_issue_block("sl_sort_kernel", k_ms) if k_ms else (None, "no profiled sl_sort_kernel launch")
            entry.update({"executed_issue_frac": blk["frac"] if blk else None, "algorithmic_frac": None,
                          "algorithmic_unit": "none: 32 B per pair from L2 / Infinity Cache in slices mode, nothing through HBM "
                                              "(lists mode, unsorted t: 40 B per pair through HBM)"})
            if blk:
                entry["executed_issue"] = {k: blk[k] for k in ("kernel", "valu_wave_instr_per_launch", "priced", "mix",
                                                               "frac_all_at_4_cycles", "profiled_ms", "source",
                                                               "SQ_INSTS_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE",
                                                               "hbm_bytes") if k in blk}
            else:
                entry["executed_issue_note"] = why
            # the front-end kernels of a batch (round 6: the histogram adds one LDS atomic per run of equal buckets)
            front = {}
            for kname in ("sl_hist_kernel", "sl_bound_kernel", "sl_sort_kernel"):
                pm = profiled_ms_of(kname)
                kk, _ = pmc_for(kname, pm) if pm else (None, None)
                if kk and kk.get("SQ_LDS_IDX_ACTIVE"):
                    front[kname] = {"profiled_ms_per_batch": kk["ms"], "lds_bank_conflict_share": round(
                        kk.get("SQ_LDS_BANK_CONFLICT", 0) / kk["SQ_LDS_IDX_ACTIVE"], 4), "kernel": kk["name"]}
            if front:
                entry["per_batch_kernels"] = front
        out[key] = entry
        for b in bl + [bel, wl]:
            b.free()
    # -- samples in any order (the C ABI allows it, a TSeries never is): ordered by time on the device first
    # (csrc/timesort.inc), then the kernels a TSeries gets.  N = 2e6 x 512 is the shape the round-4 review measured at
    # 118 ms (lists mode + the general kernel for the periods that outlast the samples) against 13 ms in order.
    n_l, np_l = 2_000_000, 512
    tl, yl, _ = synth_curve(n_l, 5, period=13.7)
    ml = (yl - yl.max()) / (2 * (yl.max() - yl.min())) + 0.25
    dfl = 0.1 / (tl[-1] - tl[0])
    pl = 1 / np.linspace(np_l * dfl, dfl, np_l)
    order = np.random.default_rng(n_l).permutation(n_l)
    wbl = lib.pdc_stringlength_work_bytes(n_l, np_l)
    bel, wl = DB(np_l * 8, dev), DB(wbl, dev)
    ms_by_order = {}
    for name, tt_, mm_ in (("in_order", tl, ml), ("shuffled", tl[order], ml[order])):
        bl = [DB.from_array(a_, dev) for a_ in (tt_, mm_, pl)]
        ms_by_order[name] = tm.ms(lambda: cabi.check(lib.pdc_stringlength_scan_dev(dev, stream, bl[0].ptr, bl[1].ptr, n_l, bl[2].ptr,
                                                                                   np_l, bel.ptr, wl.ptr, wbl)), reps=3)
        for b in bl:
            b.free()
    out["sl_any_order_2e6"] = {"ms": round(ms_by_order["shuffled"], 3), "ms_in_order": round(ms_by_order["in_order"], 3),
                               "n_samples": n_l, "n_periods": np_l, "round4_ms": 117.3,
                               "note": "samples shuffled: stable radix sort by time on the device (8 passes of 8 bits), then the "
                                       "streamed kernels' slices mode; round 4 took the lists mode and the general kernel"}
    bel.free()
    wl.free()
    # (all GPU legs run back to back; the CPU baselines of C5 follow at the end of this function)
    ms = tm.ms(lambda: cabi.check(lib.pdc_aov_scan_dev(dev, stream, bt5.ptr, bx.ptr, n, bp.ptr, n_per, 10, bth.ptr)),
               reps=5, warm=4)
    fr, _ = two_fracs(("pdm_scan_kernel<", ", 1> grid"), ms, pdm_algorithmic_frac(pairs, ms), "40 flop/pair vs 78.6 TFLOP/s")
    out["c5_aov"] = {"ms": round(ms, 4), "Gpair_per_s": round(pairs / ms / 1e6, 1), "n_bins": 10, **fr}
    lo5, hi5 = y5.min(), y5.max()
    mag = np.minimum(np.floor((y5 - lo5) / (hi5 - lo5) * 5), 4).astype(np.float64)
    bmag = DB.from_array(mag, dev)
    ms = tm.ms(lambda: cabi.check(lib.pdc_cond_entropy_scan_dev(dev, stream, bt5.ptr, bmag.ptr, n, bp.ptr, n_per,
                                                                10, 5, bth.ptr)), reps=5, warm=2)
    fr, _ = two_fracs(("pdm_scan_kernel<", ", 2> grid"), ms, pdm_algorithmic_frac(pairs, ms), "40 flop/pair vs 78.6 TFLOP/s")
    out["c5_cond_entropy"] = {"ms": round(ms, 4), "Gpair_per_s": round(pairs / ms / 1e6, 1), "cells": "10 x 5", **fr}
    # Supersmoother (a one-line TODO upstream, spectral.py:8): streamed sort + the tiled smoother, 4096 of C5's periods
    n_ss = 4096
    wss = lib.pdc_supersmoother_work_bytes(n, n_ss)
    bss = DB(wss, dev)
    ms = tm.ms(lambda: cabi.check(lib.pdc_supersmoother_scan_dev(dev, stream, bt5.ptr, bx.ptr, n, bp.ptr, n_ss, 0.0, bth.ptr,
                                                                 bss.ptr, wss)), reps=3)
    ss_hbm, ss_sweeps = None, None
    if os.path.isfile(PMC_SUMMARY):
        summ = json.load(open(PMC_SUMMARY))
        now, then = source_hashes(), summ.get("src_sha", {})
        fresh = all(now.get(f) == then.get(f) for f in KERNEL_SOURCES["ss_"])
        per = {name: k for name, k in summ.get("kernels", {}).items() if "ss2_stage_kernel" in name and "hbm_bytes" in k}
        if len(per) >= 4 and fresh:      # (each sweep's entry is the mean over its launches of 64 periods)
            ss_hbm = round(sum(k["hbm_bytes"] for k in per.values()) / 64.0 / 1e6, 2)
            ss_sweeps = {}
            for name, k in sorted(per.items()):
                n64 = sum(k.get(c, 0) for c in F64_COUNTERS)
                cyc = n64 * FP64_ISSUE_CYCLES + (k["SQ_INSTS_VALU"] - n64) * B32_ISSUE_CYCLES
                ss_sweeps[name.split("ss2::")[-1].split(" grid")[0]] = {
                    "us_per_launch_of_64_periods": round(k["ms"] * 1e3, 1),
                    "executed_issue_frac_by_type": round(cyc / SIMDS / CLOCK_HZ / (k["ms"] * 1e-3), 3),
                    "fp64_share_of_valu": round(n64 / k["SQ_INSTS_VALU"], 3),
                    "hbm_MB_per_period": round(k["hbm_bytes"] / 64.0 / 1e6, 2),
                    "hbm_TBps": round(k["hbm_bytes"] / (k["ms"] * 1e-3) / 1e12, 2)}
    out["c5_supersmoother"] = {"ms": round(ms, 3), "Gpair_per_s": round(float(n) * n_ss / ms / 1e6, 2), "n_periods": n_ss,
                               "workspace_MB": round(wss / 1e6, 1),
                               "hbm_MB_per_period_smoother_sweeps": ss_hbm,
                               "sweeps": ss_sweeps,
                               "algorithmic_MB_per_period": round(208.0 * n / 1e6, 2),
                               "executed_issue_frac": None, "algorithmic_frac": None,
                               "note": "Friedman's variable span smoother on the phase-sorted curve, mean absolute residual "
                                       "(Reimann 1994); parity unpinned by the reference; round 5: four fused sweeps of sliding "
                                       "window sums over tiles (no prefix arrays), 208 algorithmic bytes per point and period; "
                                       "hbm_MB_per_period = (2 FETCH_SIZE + WRITE_SIZE) of the four sweeps' launches (PMC) / 64 "
                                       "periods (DESIGN 4.7)"}
    bss.free()
    for b in (bt5, bx, bp, bth, bm, bsp, be, swork, bmag):
        b.free()

    # -- C4's per-GPU share: N=1e6 samples x the 1.25e6-frequency slab one of 8 GPUs scans ------------
    n4, nf4 = 1_000_000, 1_250_000
    t4, y4, dy4 = synth_curve(n4, 4)
    df4 = 1.0 / (t4[-1] - t4[0]) / 5
    b4 = [DB.from_array(a_, dev) for a_ in (t4, y4, dy4)]
    wb4 = lib.pdc_gls_work_bytes(n4, 1, nf4)
    w4, p4 = DB(wb4, dev), DB(nf4 * 8, dev)
    ms = tm.ms(lambda: cabi.check(lib.pdc_gls_scan_dev(dev, stream, b4[0].ptr, b4[1].ptr, b4[2].ptr, None, n4, 1, 0,
                                                       0.5 * df4, df4, 3 * nf4, nf4, 1, 0, p4.ptr, None, None,
                                                       w4.ptr, wb4)), reps=2, warm=1)
    fr, _ = two_fracs("gls_scan_kernel", ms, gls_algorithmic_frac(float(n4) * nf4, ms), "50 flop/pair vs 78.6 TFLOP/s")
    out["c4_slab_of_8"] = {"ms": round(ms, 2), "Gpair_per_s": round(float(n4) * nf4 / ms / 1e6, 1), **fr,
                           "note": "BASELINE configs[3] (N=1e6 x nf=1e7 over 8 GPUs): the slab j in [3.75e6, 5e6) "
                                   "one GPU scans, resident; the 8-GPU run adds one 10 MB-per-rank all-gather"}
    for b in b4 + [w4, p4]:
        b.free()
    if with_cpu:
        # the reference's per-period work on the host (never inside a timed GPU region): numpy restatement
        # of PDM._pdm / _stringlength on ONE core as upstream's Pool worker runs it, the same under
        # multiprocessing.Pool(all cores) as upstream fans it out, and the plain-C restatement under OpenMP
        # on all cores, on a bounded subsample of the grid, scaled linearly
        from oracle import c_oracle as co
        from oracle import scan_oracle as so
        cores = host_cores()
        co.set_threads(cores)
        sub = np.linspace(0, n_per - 1, 16 * max(8, cores // 8)).astype(int)
        pool = cpu_pool_baseline(cores)
        for key, np_fn, c_fn, grid in (
                ("c5_pdm", lambda p: so.pdm_scan(t5, y5, p, 5, 2), lambda p: co.pdm_scan(t5, y5, p, 5, 2), periods),
                ("c5_stringlength", lambda p: so.stringlength_scan(t5, m, p), lambda p: co.stringlength_scan(t5, m, p),
                 sl_periods)):
            t0 = time.perf_counter()
            np_fn(grid[sub[:6]])
            dt_np = (time.perf_counter() - t0) / 6
            c_fn(grid[sub[:cores]])                       # warm-up (OpenMP team)
            t0 = time.perf_counter()
            c_fn(grid[sub])
            dt_c = time.perf_counter() - t0
            pooled = {k_: v for k_, v in pool.items() if k_ in ("cores", "periods_sampled", "kind", "sample", "error",
                                                                "start_method")}
            pooled.update(pool.get(key[3:], {}))
            out[key]["cpu_baseline"] = {
                "numpy_ms_per_period_one_core": round(dt_np * 1e3, 3),
                "numpy_core_seconds_full_grid": round(dt_np * n_per, 1),
                "c_openmp_seconds_full_grid": round(dt_c * n_per / sub.size, 2), "cores": cores, "kind": "port",
                "sample": f"{sub.size} of {n_per} trial periods, scaled linearly",
                "multiprocessing_pool": pooled}
    return out


# ---- N > 1: the other configs, sharded the way they shard ------------------------------------------------
def slab(total, n, i):
    per = -(-total // n)
    b = min(i * per, total)
    return b, min(b + per, total)


def sharded_extras_one_process(cabi, lib, devices):
    """One process, the listed device slots (a repeated ordinal = loopback): C5's period grid in one slab
    per slot through the persistent phase plan, C3's curves in one contiguous group per slot."""
    n_slots = len(devices)
    out = {"slots": n_slots}
    t5, y5, m, periods, sl_periods = c5_inputs()
    n, n_per = t5.size, periods.size
    pairs = float(n) * n_per
    sigma = float(np.var(y5, ddof=1))
    plan = cabi.PhasePlan(devices, n, n_per)
    for key, kind, v, grid, args, afrac in (
            ("c5_pdm_sharded", "pdm", y5, periods, (5, 2, sigma), pdm_algorithmic_frac),
            ("c5_stringlength_sharded", "stringlength", m, sl_periods, (), None)):
        plan.upload(t5, v)
        plan.scan(kind, grid, *args)
        plan.wait()
        k_ms = []
        for _ in range(3):
            plan.scan(kind, grid, *args)
            plan.wait()
            k_ms.append(plan.kernel_ms())
        t0 = time.perf_counter()
        plan.upload(t5, v)
        plan.scan(kind, grid, *args)
        got = plan.download()
        e2e = time.perf_counter() - t0
        ms = float(np.median(k_ms))
        out[key] = {"kernel_ms_slowest_slot": round(ms, 4), "Gpair_per_s_kernel": round(pairs / ms / 1e6, 1),
                    "end_to_end_ms": round(e2e * 1e3, 3), "Gpair_per_s_end_to_end": round(pairs / e2e / 1e9, 1),
                    "argmin": int(np.nanargmin(got)),
                    "algorithmic_frac_per_slot": None if afrac is None else round(afrac(pairs / n_slots, ms), 4),
                    "note": f"period grid in {n_slots} contiguous slabs, samples replicated, no exchange; kernel = HIP "
                            "events around each slot's scan, the slowest; end to end = upload through pinned staging + "
                            "scans + results back, wall"}
    plan.close()

    # C3: curves dealt to the slots; resident per-slot buffers, one stream per slot, peaks only
    tt, yy, dd, f = c3_batch()
    B, ns = tt.shape
    nf = f.size
    g0, gd, _ = cabi.grid_params(f)
    DB = cabi.DeviceBuffer
    slots = []
    for i, dev in enumerate(devices):
        b0, b1 = slab(B, n_slots, i)
        if b1 == b0:
            continue
        nb = b1 - b0
        s = C.c_void_p()
        cabi.check(lib.pdc_stream_create(dev, C.byref(s)))
        wb = lib.pdc_gls_work_bytes(nb * ns, nb, nf)
        ev = []
        for _ in range(2):
            e = C.c_void_p()
            cabi.check(lib.pdc_event_create(dev, C.byref(e)))
            ev.append(e.value)
        slots.append({"dev": dev, "nb": nb, "stream": s.value, "ev": ev, "wb": wb,
                      "t": DB.from_array(tt[b0:b1], dev), "y": DB.from_array(yy[b0:b1], dev),
                      "dy": DB.from_array(dd[b0:b1], dev),
                      "off": DB.from_array(np.arange(nb + 1, dtype=np.int64) * ns, dev),
                      "work": DB(wb, dev), "amax": DB(nb * 8, dev), "arg": DB(nb * 8, dev)})

    def launch_all():
        for s in slots:
            cabi.check(lib.pdc_event_record(s["dev"], s["ev"][0], s["stream"]))
            cabi.check(lib.pdc_gls_scan_dev(s["dev"], s["stream"], s["t"].ptr, s["y"].ptr, s["dy"].ptr, s["off"].ptr,
                                            s["nb"] * ns, s["nb"], 0, g0, gd, 0, nf, 1, 0, None, s["amax"].ptr,
                                            s["arg"].ptr, s["work"].ptr, s["wb"]))
            cabi.check(lib.pdc_event_record(s["dev"], s["ev"][1], s["stream"]))
        for s in slots:
            cabi.check(lib.pdc_stream_sync(s["dev"], s["stream"]))
    launch_all()
    walls, kmax = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        launch_all()
        walls.append(time.perf_counter() - t0)
        worst = 0.0
        for s in slots:
            ms = C.c_float()
            cabi.check(lib.pdc_event_elapsed_ms(s["dev"], s["ev"][0], s["ev"][1], C.byref(ms)))
            worst = max(worst, ms.value)
        kmax.append(worst)
    for s in slots:
        for b in ("t", "y", "dy", "off", "work", "amax", "arg"):
            s[b].free()
        cabi.check(lib.pdc_stream_destroy(s["dev"], s["stream"]))
    pairs3 = float(B) * ns * nf
    offsets = np.arange(B + 1, dtype=np.int64) * ns
    cabi.gls_scan_batch(tt.ravel(), yy.ravel(), dd.ravel(), offsets, g0, gd, nf, want_power=False, want_peaks=True,
                        devices=devices)                       # sizes the cached per-slot buffers
    t0 = time.perf_counter()
    _, amax, _ = cabi.gls_scan_batch(tt.ravel(), yy.ravel(), dd.ravel(), offsets, g0, gd, nf, want_power=False,
                                     want_peaks=True, devices=devices)
    e2e = time.perf_counter() - t0
    ms = float(np.median(kmax))
    wall = float(np.median(walls))
    out["c3_sharded_by_curves"] = {
        "kernel_ms_slowest_slot": round(ms, 3), "launch_to_sync_wall_ms": round(wall * 1e3, 3),
        "Gpair_per_s_kernel": round(pairs3 / wall / 1e9, 1),
        "end_to_end_ms": round(e2e * 1e3, 2), "Gpair_per_s_end_to_end": round(pairs3 / e2e / 1e9, 1),
        "algorithmic_frac_per_slot": round(gls_algorithmic_frac(pairs3 / n_slots, ms), 4),
        "max_of_amax": float(np.nanmax(amax)),
        "note": f"4096 curves in {n_slots} contiguous groups, one per slot, peaks only, no exchange; kernel = resident "
                "inputs, all slots launched then synchronised (wall) and each slot's HIP events (slowest); end to end = "
                "pdc_gls_scan_batch_multi on host buffers (H2D of 197 MB of samples + scans + [B] maxima back)"}
    return out


def sharded_extras_dist(cabi, lib, torch, dist, dev, rank, world, coll):
    """One rank per GPU (torch.distributed): this rank takes slab `rank` of C5's period grid / group `rank`
    of C3's curves; kernel time = HIP events on this rank, MAX over ranks; end to end = barrier-to-barrier
    wall of host-buffer calls + the all-gather of the results, MAX over ranks."""
    out = {"ranks": world}
    DB = cabi.DeviceBuffer
    s = C.c_void_p()
    cabi.check(lib.pdc_stream_create(dev, C.byref(s)))
    stream = s.value
    tm = EventTimer(lib, cabi, dev, stream)

    max_over_ranks = coll.max

    def end_to_end(fn):
        fn()
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        dist.barrier()
        return max_over_ranks(time.perf_counter() - t0), got

    from tools import torchrun_sharded as pdist
    t5, y5, m, periods, sl_periods = c5_inputs()
    n, n_per = t5.size, periods.size
    pairs = float(n) * n_per
    sigma = float(np.var(y5, ddof=1))
    b0, b1 = slab(n_per, world, rank)
    cnt = b1 - b0
    bt5 = DB.from_array(t5, dev)
    for key, kind, v, grid, nbnc, afrac, e2e_fn in (
            ("c5_pdm_sharded", 0, y5, periods, (5, 2), pdm_algorithmic_frac,
             lambda: pdist.sharded_pdm(t5, y5, periods, 5, 2, sigma, device=dev)),
            ("c5_stringlength_sharded", 3, m, sl_periods, (1, 1), None,
             lambda: pdist.sharded_stringlength(t5, m, sl_periods, device=dev))):
        bv, bp, bo = DB.from_array(v, dev), DB.from_array(grid[b0:b1], dev), DB(max(cnt, 1) * 8, dev)
        wb = lib.pdc_phase_work_bytes(kind, n, cnt, *nbnc)
        bw = DB(wb + 8, dev)
        ms = tm.ms(lambda: cabi.check(lib.pdc_phase_scan_dev(kind, dev, stream, bt5.ptr, bv.ptr, n, bp.ptr, cnt, nbnc[0],
                                                             nbnc[1], sigma, bo.ptr, bw.ptr, wb + 8)), reps=3)
        ms = max_over_ranks(ms)
        e2e, got = end_to_end(e2e_fn)
        out[key] = {"kernel_ms_slowest_rank": round(ms, 4), "Gpair_per_s_kernel": round(pairs / ms / 1e6, 1),
                    "end_to_end_ms": round(e2e * 1e3, 3), "Gpair_per_s_end_to_end": round(pairs / e2e / 1e9, 1),
                    "argmin": int(np.nanargmin(got)),
                    "algorithmic_frac_per_rank": None if afrac is None else round(afrac(pairs / world, ms), 4),
                    "note": f"period grid in {world} contiguous slabs, one per rank, samples replicated; kernel = HIP "
                            "events, MAX over ranks; end to end = host buffers in, slab scan, all-gather of the "
                            "results (tools/torchrun_sharded.py), barrier to barrier, MAX over ranks"}
        for b in (bv, bp, bo, bw):
            b.free()
    bt5.free()

    tt, yy, dd, f = c3_batch()
    B, ns = tt.shape
    nf = f.size
    g0, gd, _ = cabi.grid_params(f)
    b0, b1 = slab(B, world, rank)
    nb = b1 - b0
    bufs = [DB.from_array(a[b0:b1], dev) for a in (tt, yy, dd)] + [DB.from_array(np.arange(nb + 1, dtype=np.int64) * ns, dev)]
    wb = lib.pdc_gls_work_bytes(nb * ns, nb, nf)
    work, amax, arg = DB(wb, dev), DB(nb * 8, dev), DB(nb * 8, dev)
    ms = tm.ms(lambda: cabi.check(lib.pdc_gls_scan_dev(dev, stream, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                                       nb * ns, nb, 0, g0, gd, 0, nf, 1, 0, None, amax.ptr, arg.ptr,
                                                       work.ptr, wb)), reps=3)
    ms = max_over_ranks(ms)
    per = -(-B // world)
    off = np.arange(nb + 1, dtype=np.int64) * ns

    def c3_host():
        _, a, _ = cabi.gls_scan_batch(tt[b0:b1].ravel(), yy[b0:b1].ravel(), dd[b0:b1].ravel(), off, g0, gd, nf,
                                      want_power=False, want_peaks=True, device=dev)
        send = torch.zeros(per, dtype=torch.float64, device="cuda")
        send[:nb] = torch.from_numpy(a).cuda()
        full = torch.empty(per * world, dtype=torch.float64, device="cuda")
        coll.gather_into(full, send)
        return full[:B].cpu().numpy()
    e2e, got = end_to_end(c3_host)
    pairs3 = float(B) * ns * nf
    out["c3_sharded_by_curves"] = {
        "kernel_ms_slowest_rank": round(ms, 3), "Gpair_per_s_kernel": round(pairs3 / ms / 1e6, 1),
        "end_to_end_ms": round(e2e * 1e3, 2), "Gpair_per_s_end_to_end": round(pairs3 / e2e / 1e9, 1),
        "algorithmic_frac_per_rank": round(gls_algorithmic_frac(pairs3 / world, ms), 4),
        "max_of_amax": float(np.nanmax(got)),
        "note": f"4096 curves in {world} contiguous groups, one per rank, peaks only; kernel = resident inputs, HIP "
                "events, MAX over ranks; end to end = host buffers in, batched scan, all-gather of the [B] maxima"}
    for b in bufs + [work, amax, arg]:
        b.free()
    return out

# ---- N > 1: STRONG scaling - a fixed grid cut into N slabs + the all-gather of the power array ----------------
STRONG_CONFIGS = (
    # key, samples, frequencies, synth_curve index, steps of the back-to-back loop (0 = single shots only)
    ("c4_sharded", 1_000_000, 10_000_000, 4, 0),
    ("c2_strong", N_SAMPLES, NF_PER_GPU, 2, 20),
)
STRONG_NOTES = {
    "c4_sharded": "BASELINE configs[3]: N=1e6 samples x nf=1e7 frequencies = 1e13 pairs, FIXED total work; the grid in "
                  "one contiguous slab per slot + one all-gather of the power array (10 MB per rank at 8 slots) + D2H "
                  "of power[1e7] (80 MB); the north star's '>= 6x at 8 GPUs' is speedup_vs_1gpu of THIS entry",
    "c2_strong": "BASELINE configs[1]'s grid (N=1e5 x nf=1e6 = 1e11 pairs) cut N ways: the honest worst case of "
                 "strong scaling - 27 ms / N of scan per GPU against the gather of an 8 MB array and the launch "
                 "overheads",
}


def strong_entry(key, n, nf, slots, k_ms, scan_gather_s, e2e_s, one, loop, power, power_one, rccl, loopback, what):
    pairs = float(n) * nf
    worst = max(k_ms)
    out = {
        "workload": STRONG_NOTES[key], "scaling": "strong", "slots": slots, "pairs": pairs,
        "kernel_ms_slowest_slot": round(worst, 4), "kernel_ms_per_slot": [round(v, 4) for v in k_ms],
        "scan_plus_gather_ms": round(scan_gather_s * 1e3, 4), "end_to_end_ms": round(e2e_s * 1e3, 3),
        "Gpair_per_s_kernel": round(pairs / worst / 1e6, 1),
        "Gpair_per_s_scan_plus_gather": round(pairs / scan_gather_s / 1e9, 1),
        "Gpair_per_s_end_to_end": round(pairs / e2e_s / 1e9, 1),
        "algorithmic_frac_per_slot": round(gls_algorithmic_frac(pairs / slots, worst), 4),
        "one_gpu": {k_: round(v, 4) for k_, v in one.items()},
        "speedup_vs_1gpu": {"kernel": round(one["kernel_ms"] / worst, 3),
                            "scan_plus_gather": round(one["scan_ms_wall"] / (scan_gather_s * 1e3), 3),
                            "end_to_end": round(one["end_to_end_ms"] / (e2e_s * 1e3), 3)},
        "rccl": rccl,
        "peak_bin": int(np.nanargmax(power)),
        "peak_bin_matches_one_gpu": bool(int(np.nanargmax(power)) == int(np.nanargmax(power_one))),
        "max_abs_diff_vs_one_gpu": float(np.nanmax(np.abs(power - power_one))),
        "note": what + ("; LOOPBACK: the slots share ONE device, so the speedups here are ~1 by construction - the "
                        "entry proves the code path, the real figure needs N GPUs" if loopback else ""),
    }
    if loop:
        out["back_to_back"] = loop
    return out


def strong_scaling_one_process(cabi, devices, loopback):
    """One process, the listed device slots, through the persistent plan (pdc_gls_plan_*): the fixed-size
    configs in `len(devices)` slabs against the same plan with ONE slot on devices[0] in the same run."""
    slots = len(devices)
    out = {}
    for key, n, nf, k, steps in STRONG_CONFIGS:
        t, y, dy = synth_curve(n, k)
        freq, df, fmin = throughput_grid(t, nf)
        f0, delta, _ = cabi.grid_params(freq)
        del freq
        res = {}
        for tag, n_sl in (("one", 1), ("all", slots)):
            if tag == "all" and loopback:
                plan = cabi.GlsPlan([devices[0]], n, nf, loopback_slots=n_sl)
            else:
                plan = cabi.GlsPlan(list(devices[:n_sl]), n, nf)
            info = plan.info()
            plan.upload(t, y, dy)
            plan.scan(f0, delta, min(nf, 200_000))          # clocks up, code objects loaded
            plan.wait()
            t0 = time.perf_counter()
            plan.scan(f0, delta, nf)
            plan.wait()
            sg = time.perf_counter() - t0
            k_ms = plan.slot_ms()
            t0 = time.perf_counter()
            plan.upload(t, y, dy)
            plan.scan(f0, delta, nf)
            power = plan.download(0)
            e2e = time.perf_counter() - t0
            loop = None
            if steps:
                plan.scan(f0, delta, nf)
                plan.wait()
                t0 = time.perf_counter()
                for _ in range(steps):
                    plan.scan(f0, delta, nf)
                plan.wait()
                per = (time.perf_counter() - t0) / steps
                loop = {"steps": steps, "ms_per_step": round(per * 1e3, 4),
                        "Gpair_per_s": round(float(n) * nf / per / 1e9, 1),
                        "note": "scans enqueued back to back; the gather of step i overlaps the scan of step i+1"}
            if tag == "all" and slots > 1:
                assert np.array_equal(power, plan.download(slots - 1), equal_nan=True), \
                    f"{key}: the all-gather left the slots with different arrays"
            plan.close()
            res[tag] = (k_ms, sg, e2e, loop, power, info)
        k1, sg1, e1, loop1, p1, _ = res["one"]
        kN, sgN, eN, loopN, pN, info = res["all"]
        one = {"kernel_ms": k1[0], "scan_ms_wall": sg1 * 1e3, "end_to_end_ms": e1 * 1e3}
        if loop1:
            one["back_to_back_ms_per_step"] = loop1["ms_per_step"]
            loopN["speedup_vs_1gpu"] = round(loop1["ms_per_step"] / loopN["ms_per_step"], 3)
        out[key] = strong_entry(
            key, n, nf, slots, kN, sgN, eN, one, loopN, pN, p1,
            {"ranks_in_communicator": info["rccl_ranks"], "exchange": info["exchange"], "slots": info["n_slots"],
             "init_error": info.get("init_error")},
            loopback,
            "one process, N devices (pdc_gls_plan_*); kernel = HIP events around every slot's slab scan, the slowest; "
            "scan_plus_gather = enqueue to all streams drained, wall; end to end = upload of (t, y, dy) to every "
            "device + scans + all-gather + D2H of the whole power array from slot 0, wall; one_gpu = the same plan "
            "with one slot on devices[0], same run")
        del p1, pN, res
    return out


def strong_scaling_dist(cabi, lib, torch, dist, dev, rank, world, coll):
    """One rank per GPU: rank r scans slab r of the fixed grid, all_gather_into_tensor (RCCL), rank 0 brings the
    whole array to the host.  Times are barrier to barrier, MAX over ranks; one_gpu = the whole grid on rank 0
    alone while the others wait."""
    out = {}
    DB = cabi.DeviceBuffer
    stream = torch.cuda.current_stream().cuda_stream
    tm = EventTimer(lib, cabi, dev, stream)

    max_over_ranks = coll.max

    def timed(fn):
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        dist.barrier()
        return max_over_ranks(time.perf_counter() - t0), got

    for key, n, nf, k, steps in STRONG_CONFIGS:
        t, y, dy = synth_curve(n, k)
        freq, df, fmin = throughput_grid(t, nf)
        f0, delta, _ = cabi.grid_params(freq)
        del freq
        host = np.stack([t, y, dy])
        per = -(-nf // world)
        b0 = min(rank * per, nf)
        cnt = min(per, nf - b0)
        dev_in = [torch.from_numpy(host).cuda()]
        wb = lib.pdc_gls_work_bytes(n, 1, per)
        work = DB(wb, dev)
        send = torch.zeros(per, dtype=torch.float64, device="cuda")
        full = torch.empty(per * world, dtype=torch.float64, device="cuda")

        def scan(j_begin, count, out_ptr, wptr, wbytes):
            tt = dev_in[0]
            cabi.check(lib.pdc_gls_scan_dev(dev, stream, tt[0].data_ptr(), tt[1].data_ptr(), tt[2].data_ptr(), None, n, 1,
                                            0, f0, delta, j_begin, count, 1, 0, out_ptr, None, None, wptr, wbytes))

        def slab_scan():
            if cnt > 0:
                scan(b0, cnt, send.data_ptr(), work.ptr, wb)

        def scan_gather():
            slab_scan()
            coll.gather_into(full, send)

        def end_to_end():
            dev_in[0] = torch.from_numpy(host).cuda()
            scan_gather()
            return full[:nf].cpu().numpy() if rank == 0 else None

        scan(b0, min(cnt, 200_000), send.data_ptr(), work.ptr, wb)          # clocks up
        k_ms = max_over_ranks(tm.ms(slab_scan, reps=1, warm=0))
        all_ms = coll.all_scalars(tm.ms(slab_scan, reps=1, warm=0))
        sg, _ = timed(scan_gather)
        e2e, power = timed(end_to_end)
        loop = None
        if steps:
            def many():
                for _ in range(steps):
                    scan_gather()
            many()
            per_step = timed(many)[0] / steps
            loop = {"steps": steps, "ms_per_step": round(per_step * 1e3, 4),
                    "Gpair_per_s": round(float(n) * nf / per_step / 1e9, 1),
                    "note": "scan then all-gather, step after step on one stream per rank (no overlap between a "
                            "step's gather and the next scan)"}
        # the whole grid on rank 0 alone
        one, power_one = None, None
        if rank == 0:
            wb1 = lib.pdc_gls_work_bytes(n, 1, nf)
            work1 = DB(wb1, dev)
            whole = torch.empty(nf, dtype=torch.float64, device="cuda")

            def one_scan():
                scan(0, nf, whole.data_ptr(), work1.ptr, wb1)

            def one_e2e():
                dev_in[0] = torch.from_numpy(host).cuda()
                one_scan()
                return whole.cpu().numpy()
            one_k = tm.ms(one_scan, reps=1, warm=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one_scan()
            torch.cuda.synchronize()
            one_wall = time.perf_counter() - t0
            t0 = time.perf_counter()
            power_one = one_e2e()
            one = {"kernel_ms": one_k, "scan_ms_wall": one_wall * 1e3, "end_to_end_ms": (time.perf_counter() - t0) * 1e3}
            if steps:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    one_scan()
                torch.cuda.synchronize()
                one["back_to_back_ms_per_step"] = (time.perf_counter() - t0) / steps * 1e3
                loop["speedup_vs_1gpu"] = round(one["back_to_back_ms_per_step"] / loop["ms_per_step"], 3)
            work1.free()
            del whole
        dist.barrier()
        if rank == 0:
            out[key] = strong_entry(
                key, n, nf, world, all_ms, sg, e2e, one, loop, power, power_one,
                {"ranks_in_communicator": dist.get_world_size(), "exchange": coll.describe(), "slots": world},
                False,
                "one rank per GPU (torch.distributed); kernel = HIP events around this rank's slab scan, every rank's "
                "listed; scan_plus_gather / end to end = barrier to barrier, MAX over ranks; end to end = H2D of "
                "(t, y, dy) on every rank + slab scan + all_gather_into_tensor + D2H of the whole power array on rank 0; "
                "one_gpu = the whole grid on rank 0 alone, the other ranks waiting")
            out[key]["kernel_ms_slowest_slot_first_launch"] = round(k_ms, 4)
        work.free()
        del send, full, dev_in
    return out


def headline_roofline(n, slab_nf, kernel_s, kernel_all_ms, clock):
    """The line's ``roofline`` block: the committed PMC summary priced against this run's kernel time."""
    launch_pairs = float(n) * float(slab_nf)
    kernel_ms_now = kernel_s * 1e3
    algorithmic = launch_pairs * FLOP_PER_PAIR / kernel_s / 1e12
    fr, blk = two_fracs("gls_scan_kernel", kernel_ms_now, algorithmic / PEAK_FP64_VECTOR_TFLOPS,
                        "50 flop/pair vs 78.6 TFLOP/s")
    why = fr.get("executed_issue_note")
    algo_bytes = 24.0 * n + 8.0 * slab_nf
    if blk:
        # the issue fraction priced by instruction type (valu_issue_block); `achieved` = that fraction of the peak
        frac = blk["frac"]
        achieved = frac * PEAK_FP64_VECTOR_TFLOPS
        traffic = blk.get("hbm_bytes")
    else:
        achieved = frac = traffic = None
    return {"bound": "valu",
            "achieved": None if achieved is None else round(achieved, 3),
            "peak": PEAK_FP64_VECTOR_TFLOPS, "unit": "TFLOP/s", "frac": frac,
            "achieved_is": "issue slots: frac x 78.6 (every fp64 / int64 VALU instruction priced at its 4 "
                           "issue cycles) - NOT flops; the flops are achieved_flops_TFLOPs",
            "achieved_flops_TFLOPs": (executed_flops(blk, kernel_ms_now) or {}).get("TFLOPs"),
            "achieved_flops": executed_flops(blk, kernel_ms_now),
            "traffic": traffic,
            "kernel": "gls_scan_kernel (+ prologue kernels, <0.1%)",
            "kernel_ms": round(kernel_ms_now, 4),
            "kernel_ms_is": "median of the HIP-event times of the timed steps",
            "kernel_ms_all": kernel_all_ms,
            "effective_clock_GHz": clock.get("effective_clock_GHz"),
            "frac_at_effective_clock": None if (frac is None or not clock.get("effective_clock_GHz"))
            else round(frac * (CLOCK_HZ / 1e9) / clock["effective_clock_GHz"], 4),
            "clock_probe": clock,
            **fr,
            "valu_issue": blk,
            "algorithmic": {"flop_per_pair": FLOP_PER_PAIR,
                            "achieved_TFLOPs": round(algorithmic, 3),
                            "ratio_to_direct_evaluation_roofline": round(
                                algorithmic / PEAK_FP64_VECTOR_TFLOPS, 4),
                            "bytes_per_launch": algo_bytes},
            "note": "fp64 vector-ALU bound (software sincos + rotation recurrences; no fp64 "
                    "transcendental unit, not a contraction).  achieved/frac = EXECUTED "
                    "issue: VALU issue cycles per launch (fp64/int64 instructions x 4 cycles, all "
                    "others x 2, from the typed rocprofv3 counters) / 1024 SIMDs / 2.4 GHz / "
                    "HIP-event time, `achieved` = that fraction of the 78.6 TFLOP/s peak; "
                    "`algorithmic` prices SURVEY 8d's 50 flop/pair of a direct "
                    "evaluation and may exceed the roofline; traffic = HBM-side bytes per "
                    "launch (FETCH_SIZE x 2 + WRITE_SIZE, separate PMC passes) vs "
                    "24 N + 8 nf algorithmic"
                    + ("" if blk else f"; executed-issue figures unavailable: {why}")}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, **arrays):
    """``out_dir/<name>.npy`` (float64) for every array, at most DUMP_LIMIT_BYTES in all: an array over its share is
    replaced by a fixed seeded sample of its elements, their indices in ``<name>_index.npy``."""
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_LIMIT_BYTES // (2 * len(arrays))
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64).ravel()
        if a.nbytes > share:
            keep = share // (a.itemsize + 8)
            idx = np.sort(np.random.default_rng(20241008).choice(a.size, keep, replace=False))
            np.save(os.path.join(out_dir, f"{name}_index.npy"), idx.astype(np.float64))
            a = a[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def clock_probe(lib, cabi, dev, stream, iters=10_000, reps=3):
    """The clock this box sustains under fp64 load, measured in THIS run right after the timed steps: a fixed count
    of v_fma_f64 (pdc_clock_probe: 16 independent chains per lane, 4 waves on every SIMD) / HIP-event time, at 4 issue
    cycles per wave64 instruction.  A 26.3-vs-28.3 ms swing of the same kernel between two boxes of the pool is then
    attributable from the line itself (the chip is power-limited under fp64 load: 2.04-2.13 GHz seen, nominal 2.4)."""
    ghz, ratios, all_ms = [], [], []
    for _ in range(reps):
        ms, wi, ratio = C.c_float(), C.c_double(), C.c_double()
        cabi.check(lib.pdc_clock_probe(dev, stream, iters, C.byref(ms), C.byref(wi), C.byref(ratio)))
        ghz.append(wi.value * FP64_ISSUE_CYCLES / (ms.value * 1e-3) / 1e9)
        ratios.append(ratio.value)
        all_ms.append(round(ms.value, 4))
    return {"effective_clock_GHz": round(float(np.median(ghz)), 4), "probe_ms": all_ms,
            "fma_wave_instr_per_simd": 4.0 * iters * 128.0,
            "s_memtime_ticks_per_100MHz_tick": round(float(np.median(ratios)), 4),
            "note": "fixed-instruction-count fp64 fma spin (pdc_clock_probe) run right after the timed steps: "
                    "wave-instructions per SIMD x 4 cycles / HIP-event time, median of 3; a LOWER bound of the clock "
                    "(it assumes the fmas issue back to back)"}


class Coll:
    """The few collectives bench.py needs, on whichever backend init_dist() got: device tensors over RCCL ("nccl"),
    or - the loud fallback - host tensors over gloo."""

    def __init__(self, torch, dist, backend):
        self.torch, self.dist, self.backend = torch, dist, backend
        self.where = "cuda" if backend == "nccl" else "cpu"

    def max(self, x):
        v = self.torch.tensor([x], dtype=self.torch.float64, device=self.where)
        self.dist.all_reduce(v, op=self.dist.ReduceOp.MAX)
        return float(v.item())

    def all_scalars(self, x):
        mine = self.torch.tensor([x], dtype=self.torch.float64, device=self.where)
        got = [self.torch.zeros_like(mine) for _ in range(self.dist.get_world_size())]
        self.dist.all_gather(got, mine)
        return [float(v.item()) for v in got]

    def gather_into(self, full, send, async_op=False):
        """all_gather_into_tensor of device tensors; through the host under gloo (synchronous there)."""
        if self.backend == "nccl":
            return self.dist.all_gather_into_tensor(full, send, async_op=async_op)
        host = self.torch.empty(full.numel(), dtype=full.dtype)
        self.dist.all_gather_into_tensor(host, send.cpu())
        full.copy_(host)
        return None

    def describe(self):
        if self.backend == "nccl":
            return f"rccl (torch.distributed, backend {self.dist.get_backend()})"
        return "FALLBACK: gloo through host memory (the RCCL process group could not be built)"


def init_dist(torch, dist, local_rank):
    """torch.distributed over RCCL (backend "nccl"); if the communicator cannot be built - or its first collective
    fails - every rank falls back, LOUDLY, to gloo: the barrier / max-over-ranks timing and the all-gather of the
    power array then go through host memory, the line says so (`rccl.exchange`, `rccl.init_error`), and the run
    still prints its headline instead of dying with rc != 0.  Returns (backend, error or None)."""
    err = None
    if os.environ.get("PDC_FORCE_RCCL_FAIL") == "1":
        err = "PDC_FORCE_RCCL_FAIL=1 (injected)"
    elif not torch.cuda.is_available():
        err = "torch.cuda.is_available() is False"
    else:
        try:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
            probe = torch.ones(1, device="cuda")
            dist.all_reduce(probe)
            torch.cuda.synchronize()
            if int(probe.item()) != dist.get_world_size():
                raise RuntimeError(f"all_reduce probe returned {probe.item()} on {dist.get_world_size()} ranks")
            return "nccl", None
        except Exception as exc:
            err = f"{type(exc).__name__}: {exc}"[:400]
            try:
                if dist.is_initialized():
                    dist.destroy_process_group()
            except Exception:
                pass
    sys.stderr.write(f"bench.py: WARNING: RCCL process group unavailable ({err}); falling back to gloo - the power "
                     "array is gathered through host memory\n")
    dist.init_process_group(backend="gloo")
    return "gloo", err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the C3/C5/end-to-end extra keys")
    ap.add_argument("--force-dist", action="store_true",
                    help="take the torch.distributed path even with one rank (testing)")
    ap.add_argument("--force-plan", action="store_true",
                    help="take the one-process multi-device plan path even with one GPU (testing)")
    ap.add_argument("--force-sharded-extras", action="store_true",
                    help="run the N > 1 extras even with one rank / one slot (testing)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline: clock probe, FFT path, extras, CPU baselines, "
                         "and with N > 1 the plan's kernel time, the sharded extras and the strong-scaling entries")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the power array of the last timed step to DIR/power.npy (float64)")
    ap.add_argument("--loopback", type=int, default=0, metavar="N",
                    help="N logical slots on ONE device through the plan path (testing the N > 1 code on a 1-GPU box); "
                         "the all-gather runs as device-to-device copies; `value` is not a scaling figure")
    args = ap.parse_args()

    # ONE JSON line on stdout, nothing else: RCCL writes a version banner to the C-level stdout of every
    # process that creates a communicator (flushed at exit, i.e. AFTER anything Python printed), so file
    # descriptor 1 is pointed at stderr for the whole run and the line goes to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist_mode = world > 1 or args.force_dist            # one rank per GPU (torchrun)
    if dist_mode and args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    loopback = args.loopback if not dist_mode else 0
    plan_mode = not dist_mode and (args.gpus > 1 or args.force_plan or loopback > 0)   # one process, N devices
    n_gpus = world if dist_mode else args.gpus
    n_slots = loopback if loopback else n_gpus          # slabs of the grid

    torch = dist = None
    dist_backend, dist_error = None, None
    # (the host driver of this pool only supports dmabuf IPC: RCCL between processes - and, to be safe, between the
    # devices of one process - needs it set before anything initialises HIP)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if dist_mode:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        import torch
        import torch.distributed as dist
        dist_backend, dist_error = init_dist(torch, dist, local_rank)
        coll = Coll(torch, dist, dist_backend)
        if torch.cuda.is_available():
            torch.cuda.set_device(local_rank)

    from periodicity_amd import _cabi
    lib = _cabi.lib()
    dev = local_rank
    have = _cabi.device_count()
    if have <= dev or (plan_mode and have < args.gpus):
        raise SystemExit(f"bench.py needs {args.gpus if plan_mode else dev + 1} GPU(s), {have} visible; "
                         "no CPU fallback exists")

    # ---- workload --------------------------------------------------------------------------
    n = N_SAMPLES
    nf_total = NF_PER_GPU * n_slots
    t, y, dy = synth_curve(n)
    freq, df, fmin = throughput_grid(t, nf_total)
    f0, delta, _ = _cabi.grid_params(freq)
    slab_nf = NF_PER_GPU
    j_begin = rank * slab_nf if dist_mode else 0
    stream = None
    plan = None
    plan_info = None

    if plan_mode:
        if loopback:
            plan = _cabi.GlsPlan([0], n, nf_total, loopback_slots=loopback)
        else:
            plan = _cabi.GlsPlan(list(range(args.gpus)), n, nf_total)
        plan_info = plan.info()
        plan.upload(t, y, dy)
    elif dist_mode:
        tt = torch.from_numpy(np.stack([t, y, dy])).cuda()
        d_t, d_y, d_dy = (tt[i].data_ptr() for i in range(3))
        # two generations of the output buffers: the all-gather of step i (RCCL's own stream) overlaps
        # the scan of step i+1 (compute stream); a buffer is reused only after its gather was waited on
        powers = [torch.empty(nf_total, dtype=torch.float64, device="cuda") for _ in range(2)]
        work_bytes = lib.pdc_gls_work_bytes(n, 1, slab_nf)
        work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
        d_work = work.data_ptr()
        slabs = [torch.empty(slab_nf, dtype=torch.float64, device="cuda") for _ in range(2)]
        pending = [None, None]
        counter = [0]
        stream = torch.cuda.current_stream().cuda_stream
    else:
        bufs = [_cabi.DeviceBuffer.from_array(a, dev) for a in (t, y, dy)]
        d_t, d_y, d_dy = (b.ptr for b in bufs)
        power_buf = _cabi.DeviceBuffer(nf_total * 8, dev)
        work_bytes = lib.pdc_gls_work_bytes(n, 1, slab_nf)
        work_buf = _cabi.DeviceBuffer(work_bytes, dev)
        d_work, d_power_slab = work_buf.ptr, power_buf.ptr
        sp = C.c_void_p()
        _cabi.check(lib.pdc_stream_create(dev, C.byref(sp)))
        stream = sp.value

    def new_event():
        e = C.c_void_p()
        _cabi.check(lib.pdc_event_create(dev, C.byref(e)))
        return e.value

    plan_kernel_ms = []

    def step(ev=None):
        if plan_mode:
            plan.scan(f0, delta, nf_total)
            return
        out_ptr = d_power_slab if not dist_mode else None
        if dist_mode:
            g = counter[0] % 2
            if pending[g] is not None:      # stream-level wait: buffers of generation g are free again
                pending[g].wait()
            out_ptr = slabs[g].data_ptr()
        if ev:
            _cabi.check(lib.pdc_event_record(dev, ev[0], stream))
        _cabi.check(lib.pdc_gls_scan_dev(dev, stream, d_t, d_y, d_dy, None, n, 1, 0, f0, delta,
                                         j_begin, slab_nf, 1, 0, out_ptr, None, None, d_work,
                                         work_bytes))
        if ev:
            _cabi.check(lib.pdc_event_record(dev, ev[1], stream))
        if dist_mode:
            pending[g] = coll.gather_into(powers[g], slabs[g], async_op=True)
            counter[0] += 1

    def drain():
        if dist_mode:
            for h in pending:
                if h is not None:
                    h.wait()

    def sync():
        if plan_mode:
            plan.wait()
        elif dist_mode:
            torch.cuda.synchronize()
        else:
            _cabi.check(lib.pdc_stream_sync(dev, stream))

    def barrier():
        if dist_mode:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    drain()
    events = [] if plan_mode else [(new_event(), new_event()) for _ in range(args.steps)]
    barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(None if plan_mode else events[i])
    drain()
    sync()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist_mode:
        elapsed = coll.max(elapsed)

    # what the last timed step computed, read back before anything else runs on the device (the FFT path of
    # --full writes into the same buffer)
    got = None
    if rank == 0:
        if plan_mode:
            got = plan.download(0)
            if n_slots > 1:      # every slot must hold the same gathered array
                other = plan.download(n_slots - 1)
                assert np.array_equal(got, other, equal_nan=True), "all-gather left the devices with different arrays"
        elif dist_mode:
            got = powers[(counter[0] - 1) % 2].cpu().numpy()
        else:
            got = power_buf.to_array(np.float64, nf_total)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, power=got)

    if args.full:
        # same-run clock evidence: what this box sustains under fp64 load, right after the timed steps
        try:
            clock = clock_probe(lib, _cabi, dev, None if plan_mode else stream)
        except Exception as exc:
            clock = {"effective_clock_GHz": None, "error": f"{type(exc).__name__}: {exc}"}
    else:
        clock = {"effective_clock_GHz": None, "note": "the clock probe runs with --full"}

    if plan_mode and not args.full:
        kernel_all_ms, end_to_end_s = [], None
    elif plan_mode:
        # kernel time of one slab scan on device 0, measured outside the timed region (the plan keeps
        # one event pair; reading it per step would serialise the double buffering)
        for _ in range(3):
            plan.scan(f0, delta, nf_total)
            plan.wait()
            plan_kernel_ms.append(plan.kernel_ms())
        kernel_all_ms = [round(v, 4) for v in plan_kernel_ms]
        # PCIe-inclusive figure of the sharded call (never `value`): replicate the samples, scan, gather,
        # bring the whole power array back to the host
        te = time.perf_counter()
        plan.upload(t, y, dy)
        plan.scan(f0, delta, nf_total)
        plan.download(0)
        end_to_end_s = time.perf_counter() - te
    else:
        kernel_all_ms = []
        for a, b in events:
            ms = C.c_float()
            _cabi.check(lib.pdc_event_elapsed_ms(dev, a, b, C.byref(ms)))
            kernel_all_ms.append(round(ms.value, 4))
    kernel_s = float(np.median(kernel_all_ms)) / 1e3 if kernel_all_ms else None

    sharded = None
    if args.full and (n_slots > 1 or args.force_sharded_extras) and not args.no_extras:
        # (informational: a failure here must not cost the headline line - every rank runs the same code, so an
        # exception raised before a collective is raised on all of them)
        try:
            if dist_mode:
                sharded = sharded_extras_dist(_cabi, lib, torch, dist, dev, rank, world, coll)
            else:
                sharded = sharded_extras_one_process(_cabi, lib, [0] * loopback if loopback else list(range(args.gpus)))
        except Exception as exc:
            sharded = {"error": f"{type(exc).__name__}: {exc}"}
        # STRONG scaling: BASELINE configs[3] (C4, the config the '>= 6x at 8 GPUs' target is stated on) and C2's
        # grid cut N ways, against one slot of the same run
        try:
            if dist_mode:
                strong = strong_scaling_dist(_cabi, lib, torch, dist, dev, rank, world, coll)
            else:
                strong = strong_scaling_one_process(_cabi, [0] * loopback if loopback else list(range(args.gpus)),
                                                    bool(loopback))
        except Exception as exc:
            strong = {"strong_scaling_error": f"{type(exc).__name__}: {exc}"}
        sharded = dict(sharded or {}, **strong)

    if rank == 0:
        pairs_per_step = float(n) * float(nf_total)
        value = pairs_per_step * args.steps / elapsed / 1e9
        out = {
            "metric": "Lomb-Scargle Gpair/s (sample x freq), fp64, N=1e5 x 1e6 per GPU",
            "value": round(value, 2), "unit": "Gpair/s", "n_gpus": n_gpus, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "fp64 generalized Lomb-Scargle (fit_mean, heteroscedastic dy), "
                                   f"N={n} unevenly sampled points x {NF_PER_GPU} trial "
                                   "frequencies per GPU (BASELINE configs[1]); inputs resident in "
                                   "HBM, exact direct summation",
                       "n_samples": n, "n_freq_total": nf_total,
                       "sharding": f"frequency grid in {n_slots} contiguous slab(s)"
                                   + (", RCCL all-gather of power" if n_gpus > 1 else "")
                                   + (f"; LOOPBACK: {loopback} logical slots on one device, the all-gather as "
                                      "device-to-device copies (a test of the N > 1 logic, not a scaling figure)"
                                      if loopback else ""),
                       "launcher": "one process, N devices (pdc_gls_plan_*, ncclCommInitAll)" if plan_mode
                                   else ("one rank per GPU (torch.distributed over RCCL)" if dist_mode
                                         else "one process, one device")},
            "roofline": None if kernel_s is None else headline_roofline(n, slab_nf, kernel_s, kernel_all_ms, clock),
            "peak_bin": int(np.nanargmax(got)),
        }
        if plan_mode:
            out["rccl"] = {"ranks_in_communicator": plan_info["rccl_ranks"], "exchange": plan_info["exchange"],
                           "slots": plan_info["n_slots"], "init_error": plan_info.get("init_error")}
        if plan_mode and end_to_end_s is not None:
            out["end_to_end_sharded"] = {
                "ms": round(end_to_end_s * 1e3, 3),
                "Gpair_per_s": round(pairs_per_step / end_to_end_s / 1e9, 1),
                "note": "H2D of (t, y, dy) to every device + slab scans + all-gather + D2H of power[nf] "
                        "from device 0, wall clock (the shape of pdc_gls_scan_multi / GLS(devices=...))"}
        if dist_mode:
            out["rccl"] = {"ranks_in_communicator": dist.get_world_size(), "exchange": coll.describe(), "slots": world,
                           "init_error": dist_error}
        if sharded is not None:
            out["extras"] = sharded
            c4 = sharded.get("c4_sharded") if isinstance(sharded, dict) else None
            if isinstance(c4, dict) and "speedup_vs_1gpu" in c4:
                # `value` above is WEAK-scaled (C2 per GPU); the north star's ">= 6x at 8 GPUs" is THIS figure
                out["strong_scaling"] = dict(c4["speedup_vs_1gpu"], config="BASELINE configs[3]: N=1e6 x nf=1e7, fixed total work",
                                             slots=c4["slots"], end_to_end_ms=c4["end_to_end_ms"],
                                             one_gpu_end_to_end_ms=c4["one_gpu"]["end_to_end_ms"],
                                             note="copy of extras.c4_sharded.speedup_vs_1gpu: strong scaling of the fixed C4 "
                                                  "workload against one slot of the same run" + ("; LOOPBACK: ~1 by construction"
                                                                                                    if loopback else ""))
            else:
                out["strong_scaling"] = None
        if args.full and n_slots == 1 and not dist_mode and not plan_mode:
            # informational: the reference's own algorithm on the device (Tier F), same workload
            wb = lib.pdc_gls_fft_work_bytes(n, nf_total)
            fwork = _cabi.DeviceBuffer(wb, dev)
            tm = EventTimer(lib, _cabi, dev, stream)
            fms = tm.ms(lambda: _cabi.check(lib.pdc_gls_scan_fft_dev(
                dev, stream, d_t, d_y, d_dy, n, fmin, df, nf_total, 1, 0, d_power_slab, fwork.ptr, wb)),
                reps=5)
            fft_power = power_buf.to_array(np.float64, nf_total)
            out["fft_path"] = {"ms": round(fms, 4),
                               "effective_Gpair_per_s": round(pairs_per_step / fms / 1e6, 1),
                               "peak_bin": int(np.nanargmax(fft_power)),
                               "roofline": fft_path_roofline(n, nf_total, fms),
                               "note": "pdc_gls_scan_fft_dev: the reference's extirpolation + FFT "
                                       "algorithm on the device (approximate, like upstream); not "
                                       "the headline metric, which counts exact pair evaluations"}
            fwork.free()
            if not args.no_extras:
                out["extras"] = extra_configs(lib, _cabi, dev, stream, t, y, dy, f0, delta, nf_total,
                                               with_cpu=not args.no_cpu_baseline)
        if args.full and not args.no_cpu_baseline and n_gpus == 1 and n_slots == 1:
            base, p_fft = cpu_baseline(t, y, dy, freq, df, fmin)
            out["cpu_baseline"] = base
            out["peak_bin_matches_cpu_reference_path"] = bool(
                int(np.nanargmax(p_fft)) == out["peak_bin"])
        os.write(real_stdout, (json.dumps(out) + "\n").encode())

    if plan_mode:
        plan.close()
    if dist_mode:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
