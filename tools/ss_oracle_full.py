"""The Supersmoother through the C ABI against the C oracle on EVERY period of grids that cross the host driver's batch
and sub-batch seams (developer tool; tests/test_supersmoother_gpu.py runs it in child processes because the library reads
its PDC_SS_* / PDC_SL_* switches once per process).

    python tools/ss_oracle_full.py 50000x4096 4097x787e@3 300000x203du 74326x603o
      NxP[flags][@alpha]: N samples (mean cadence 0.1) x P periods, bass control alpha (default 0).
      flags: d = duplicate time stamps, two gaps, a negative start; o = Julian-date offset (t + 2454953.5); u = the
      samples handed over in a random order (the oracle gets the stable time sort); e = even sampling, cadence 0.1.

The grid (`build_grid`) puts every kind of period into every batch and sub-batch of supersmoother_scan_impl: P periods
uniform in frequency from 4.37 cadences to the baseline, then every 37th slot (coprime to 8 and 64), the slots 64 k - 1,
64 k, 64 k + 1, z k - 1, z k for the batch sizes z = 256, 384, 512 (and 16 where P < 64), and the last slot are overwritten with, in rotation:
  kind 1  a period beyond the baseline (1.001, 2, 57 baselines; with o also 2454953.5 and half of it) -> ss_direct_kernel;
  kind 2  with e: a commensurate period (an integer or a simple fraction times the cadence) -> tied runs longer than a
          halo -> flag[q] -> ss_smooth_kernel;
  kind 3  a tenth of the cadence.
With e, slots 70 .. 113 (one batch, beyond its first 64 slots) are 44 consecutive commensurate periods: more than the 16
workgroups the generic kernel walks the flagged list with.

Checks per spec: every period within 1e-9 of oracle/c_oracle.supersmoother_scan; the same argmin (the grid repeats
periods: a slot whose oracle value lies within 1e-9 of the oracle's minimum counts); a second call bit-identical; the grid
REVERSED (same count: the same launch shape) gives every period the same bits - a period's arithmetic must not depend on
its slot.  A miss prints its slot, kind, batch / sub-batch origin and the same period scanned alone.
    SS_FULL_DEV=1     through pdc_supersmoother_scan_dev with a workspace of exactly pdc_supersmoother_work_bytes(n, P)
                      bytes, filled with 0xFF first (stale-workspace reads show).
    SS_CHECK_SAVE=f   saves the results per spec (np.savez) for A/B comparisons between switch settings.
OpenMP threads of the oracle: OMP_NUM_THREADS, else min(16, cpus)."""
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RTOL = 1e-9
CADENCE = 0.1
KIND = {0: "grid", 1: "one-cycle", 2: "commensurate", 3: "tenth-of-cadence"}
STRETCH = (70, 114)
# multiples of the cadence: few distinct phases, each a run of n / k ... n equal (or all but equal) phases
COMMENSURATE = (3.0, 7.0, 2.5, 16.0, 1.5, 50.0, 12.0, 1.0, 100.0, 4.0 / 3.0, 25.0, 9.0)


def parse_spec(spec):
    m = re.fullmatch(r"(\d+)x(\d+)([deou]*)(?:@([0-9.]+))?", spec)
    if not m:
        raise ValueError(f"bad spec {spec!r}: NxP[deou][@alpha]")
    return int(m.group(1)), int(m.group(2)), m.group(3), float(m.group(4) or 0.0)


def make_curve(n, n_per, flags):
    """(t, y) as handed to the device and (t, y) as a TSeries would hold them (stable time sort)."""
    rng = np.random.default_rng(n + 3 * n_per)
    t = np.arange(float(n)) * CADENCE if "e" in flags else np.sort(rng.uniform(0, CADENCE * n, n))
    if "d" in flags:
        t[n // 3:] += 0.31 * CADENCE * n
        t[2 * n // 3:] += 0.07 * CADENCE * n
        t[5:n:7] = t[4:n - 1:7]
        t -= 0.4 * CADENCE * n
    if "o" in flags:
        t += 2454953.5
    y = np.sin(2 * np.pi * t / 7.3) + 0.3 * np.cos(4 * np.pi * t / 7.3) + 0.2 * rng.standard_normal(n)
    gt, gy = t, y
    if "u" in flags:
        order = rng.permutation(n)
        gt, gy = t[order], y[order]
        back = np.argsort(gt, kind="stable")
        t, y = gt[back], gy[back]
    return gt, gy, t, y


def special_slots(n_per):
    s = set(range(0, n_per, 37)) | {n_per - 1}
    for k in range(1, n_per // 64 + 2):
        s |= {64 * k - 1, 64 * k, 64 * k + 1}
    for z in (256, 384, 512) + ((16,) if n_per < 64 else ()):      # (a million samples: batches of 16, grids of tens)
        for k in range(1, n_per // z + 2):
            s |= {z * k - 1, z * k}
    return sorted(i for i in s if 0 <= i < n_per)


def build_grid(t_sorted, n_per, flags):
    """(periods, kind): see the module docstring."""
    base = float(t_sorted[-1] - t_sorted[0])
    periods = 1.0 / np.linspace(1.0 / (4.37 * CADENCE), 1.0 / base, n_per)
    kind = np.zeros(n_per, dtype=np.int8)
    beyond = [1.001 * base, 2.0 * base, 57.0 * base] + ([2454953.5, 2454953.5 / 2] if "o" in flags else [])
    kinds = (1, 2, 3) if "e" in flags else (1, 3)
    used = {1: 0, 2: 0, 3: 0}
    for r, slot in enumerate(special_slots(n_per)):
        k = kinds[r % len(kinds)]
        if k == 1:
            periods[slot] = beyond[used[1] % len(beyond)]
        elif k == 2:
            periods[slot] = COMMENSURATE[used[2] % len(COMMENSURATE)] * CADENCE
        else:
            periods[slot] = 0.1 * CADENCE
        used[k] += 1
        kind[slot] = k
    if "e" in flags and n_per >= STRETCH[1] + 6:
        for i, slot in enumerate(range(*STRETCH)):
            periods[slot] = (2 + i) * 0.5 * CADENCE
            kind[slot] = 2
    return periods, kind


def shape_of(n, n_per):
    """batch, sub-batch (0: the tiled smoother is not used), segments: the pdc_test_ss_shape hook."""
    import ctypes
    from periodicity_amd import _cabi
    out = (ctypes.c_int64 * 10)()
    _cabi.check(_cabi.lib().pdc_test_ss_shape(n, n_per, out))
    return dict(zip(("batch", "sb", "seg", "seg34", "grid_ss", "grid_fb", "tiled", "streamed", "fastsort", "bytes"), out))


def scan(t, y, periods, alpha):
    from periodicity_amd import _cabi
    if not os.environ.get("SS_FULL_DEV"):
        return _cabi.supersmoother_scan(t, y, periods, alpha)
    lib, DB = _cabi.lib(), _cabi.DeviceBuffer
    wb = lib.pdc_supersmoother_work_bytes(t.size, periods.size)
    bufs = [DB.from_array(t, 0), DB.from_array(y, 0), DB.from_array(periods, 0), DB(periods.size * 8, 0), DB(wb, 0)]
    try:
        _cabi.check(lib.pdc_memset(0, bufs[4].ptr, 0xFF, wb))
        _cabi.check(lib.pdc_memset(0, bufs[3].ptr, 0xFF, periods.size * 8))
        _cabi.check(lib.pdc_supersmoother_scan_dev(0, None, bufs[0].ptr, bufs[1].ptr, t.size, bufs[2].ptr, periods.size,
                                                   float(alpha), bufs[3].ptr, bufs[4].ptr, wb))
        _cabi.check(lib.pdc_device_sync(0))
        return bufs[3].to_array(np.float64, periods.size)
    finally:
        for b in bufs:
            b.free()


def main(specs):
    from oracle import c_oracle as co
    co.set_threads(int(os.environ.get("OMP_NUM_THREADS") or min(16, os.cpu_count() or 1)))
    worst, failed, saved = 0.0, [], {}
    for spec in specs:
        n, n_per, flags, alpha = parse_spec(spec)
        gt, gy, t, y = make_curve(n, n_per, flags)
        periods, kind = build_grid(t, n_per, flags)
        z = shape_of(n, n_per)
        got = scan(gt, gy, periods, alpha)
        again = scan(gt, gy, periods, alpha)
        back = scan(gt, gy, periods[::-1].copy(), alpha)[::-1]
        t0 = time.time()
        want = co.supersmoother_scan(t, y, periods, alpha)
        dt = time.time() - t0
        rel = np.abs(got - want) / np.abs(want)
        rel[~np.isfinite(rel)] = np.inf
        w = int(rel.argmax())
        moved = np.nonzero(got != back)[0]
        moved_rel = float(np.max(np.abs(got[moved] - back[moved]) / np.abs(got[moved]))) if moved.size else 0.0
        a = int(np.argmin(got))
        same_min = a == int(np.argmin(want)) or want[a] <= want.min() * (1 + RTOL)
        worst = max(worst, float(rel.max()))
        print(f"{spec}: batch {z['batch']} sb {z['sb']} seg {z['seg']}/{z['seg34']}; ALL {n_per} periods "
              f"({', '.join(f'{int((kind == k).sum())} {v}' for k, v in KIND.items())}), max rel err vs oracle {rel.max():.2e} "
              f"(slot {w}, {KIND[int(kind[w])]}), {int((rel > RTOL).sum())} over 1e-9; bitwise repeatable: "
              f"{np.array_equal(got, again)}; reversed grid: {moved.size} periods differ (max {moved_rel:.1e}); "
              f"argmin {'same' if same_min else 'DIFFERS'}; oracle {dt:.1f} s", flush=True)
        for q in np.argsort(-rel)[:5]:
            if rel[q] > RTOL:
                alone = scan(gt, gy, periods[q:q + 1].copy(), alpha)[0]
                p0 = q // z["batch"] * z["batch"]
                q0 = (q - p0) // z["sb"] * z["sb"] if z["sb"] else 0
                print(f"  MISS slot {q} ({KIND[int(kind[q])]}, period {periods[q]!r}) p0 {p0} q0 {q0}: got {got[q]!r} "
                      f"want {want[q]!r} rel {rel[q]:.2e}; alone {alone!r} (rel {abs(alone - want[q]) / abs(want[q]):.2e})", flush=True)
        for q in moved[:5]:
            print(f"  MOVED slot {q} ({KIND[int(kind[q])]}, period {periods[q]!r}): forward {got[q]!r} reversed {back[q]!r}", flush=True)
        if not (rel.max() <= RTOL and np.array_equal(got, again) and moved.size == 0 and same_min):
            failed.append(spec)
        saved[spec] = got
    if os.environ.get("SS_CHECK_SAVE"):
        np.savez(os.environ["SS_CHECK_SAVE"], **saved)
    assert not failed, failed
    print("ok", worst)


if __name__ == "__main__":
    main(sys.argv[1:])
