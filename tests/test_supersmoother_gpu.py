"""The Supersmoother period search (a one-line TODO upstream, spectral.py:8) through the C ABI against the oracle's
restatement of the published algorithm (Friedman 1984 `supsmu`, periodic; Reimann 1994).  PARITY UNPINNED BY THE
REFERENCE: the oracle is pinned to a literal restatement of the Fortran's updating formulas (CPU test below)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import scan_oracle as so
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.phase import SuperSmoother

RTOL = 1e-9


def curve(n, seed, even=False, period=7.3):
    rng = np.random.default_rng(seed)
    t = np.arange(float(n)) * 0.1 if even else np.sort(rng.uniform(0, 0.1 * n, n))
    y = np.sin(2 * np.pi * t / period) + 0.3 * np.cos(4 * np.pi * t / period) + 0.2 * rng.standard_normal(n)
    return t, y


def window_sums_equal_the_literal_updating_formulas(smooth):
    """`smooth` (so.ss_smooth, or its C restatement: tests/test_oracle_golden.py) against the literal restatement of
    Friedman's `smooth` (one point out, one point in), ties included, and the whole of `supsmu` built on either."""
    rng = np.random.default_rng(1)
    for n in (40, 101, 400):
        x = np.sort(rng.uniform(0, 1, n))
        y = np.sin(2 * np.pi * x) + 0.3 * rng.standard_normal(n)
        if n == 101:
            x[10] = x[11]
            x[50:53] = x[50]
        v = (1e-3 * (x[3 * (n // 4) - 1] - x[n // 4 - 1])) ** 2
        for span in so.SS_SPANS:
            a, ra = so.ss_smooth_incremental(x, y, span, v, True)
            b, rb = smooth(x, y, span, v, True)
            np.testing.assert_allclose(b, a, rtol=0, atol=1e-12)
            np.testing.assert_allclose(rb, ra, rtol=0, atol=1e-12)
        for alpha in (0.0, 4.0):
            np.testing.assert_allclose(so.supersmoother(x, y, alpha, smooth), so.supersmoother(x, y, alpha, so.ss_smooth_incremental),
                                       rtol=0, atol=1e-12)


def test_oracle_window_sums_equal_the_literal_updating_formulas():
    """CPU: the vectorised smoother (window sums) against the literal restatement of Friedman's `smooth` (one point
    out, one point in), ties included, and the whole of `supsmu` built on either."""
    window_sums_equal_the_literal_updating_formulas(so.ss_smooth)
    t, y = curve(2000, 3)
    per = np.linspace(5.0, 10.0, 21)
    assert abs(per[np.argmin(so.supersmoother_scan(t, y, per))] - 7.3) < 0.26


def window_sums_stay_exact_for_phases_crowded_into_a_sliver_of_the_cycle(smooth):
    """`smooth` against a brute-force fit of every window in locally centred long-double arithmetic (see the test below)."""
    L = np.longdouble
    rng = np.random.default_rng(2)
    n = 300
    for spread in (1e-5, 1e-7):
        x = np.sort(2.45e-3 + spread * rng.uniform(0, 1, n))
        y = np.sin(2 * np.pi * (x - x[0]) / spread * 3) + 0.3 * rng.standard_normal(n)
        v = (1e-3 * (x[3 * (n // 4) - 1] - x[n // 4 - 1])) ** 2
        for span in so.SS_SPANS:
            ibw = so.ss_half_width(n, span)
            want = np.empty(n)
            for j in range(n):
                idx = np.arange(j - ibw, j + ibw + 1)
                xs = np.where(idx < 0, x[idx % n] - 1, np.where(idx >= n, x[idx % n] + 1, x[idx % n])).astype(L) - L(x[j])
                ys = y[idx % n].astype(L)
                xm, ym = xs.mean(), ys.mean()
                var, cvar = ((xs - xm) ** 2).sum(), ((xs - xm) * (ys - ym)).sum()
                want[j] = (cvar / var if var > v else 0) * (0 - xm) + ym
            got, _ = smooth(x, y, span, v, False)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


def test_oracle_window_sums_stay_exact_for_phases_crowded_into_a_sliver_of_the_cycle():
    """CPU: a period far beyond the baseline folds the samples into a sliver of the cycle (spread 1e-5 ... 1e-7).  The
    oracle's window sums (long double, abscissae relative to the median, wrapped parts added through their own sums)
    equal a brute-force fit of every window in LOCALLY centred long-double arithmetic to rounding - where the literal
    double-precision updating formulas of the Fortran, and the round-4 oracle that prefixed over shifted abscissae, lose
    var = Sxx - fbw xm^2 altogether (errors of 1e-4 ... 0.2).  The device kernels are held to THIS oracle."""
    window_sums_stay_exact_for_phases_crowded_into_a_sliver_of_the_cycle(so.ss_smooth)


@pytest.mark.gpu
@pytest.mark.parametrize("n,even,alpha", [(300, False, 0.0), (5000, False, 0.0), (5000, False, 5.0), (9000, False, 0.0),
                                          (4000, True, 0.0), (6000, True, 2.0)])
def test_supersmoother_scan_matches_the_oracle(n, even, alpha):
    """Below 4096 samples every period is sorted by the fallback kernel, above by the streamed kernels; even
    sampling at commensurate periods gives tied phases (averaged fits) and clustered bins (fallback sort)."""
    t, y = curve(n, n + 1, even)
    periods = np.concatenate([np.linspace(2.1, 40.0, 24), [7.3, 10.0, 0.5, 25.0, 3.7 * t[-1]]])
    got = _cabi.supersmoother_scan(t, y, periods, alpha)
    want = so.supersmoother_scan(t, y, periods, alpha)
    np.testing.assert_allclose(got, want, rtol=RTOL)
    assert np.array_equal(got, _cabi.supersmoother_scan(t, y, periods, alpha))      # bitwise repeatable


@pytest.mark.gpu
@pytest.mark.parametrize("n", [50_000, 74_326, 200_000])
def test_supersmoother_scan_matches_the_oracle_at_the_sizes_it_runs(n):
    """N = 5e4 is bench.py's shape, 74 326 the reference's SunSpots curve, 2e5 the class the workspace is sized for:
    ten periods each - a commensurate (tied phases) one on an evenly sampled copy, periods beyond the baseline, the
    bass control on - against the oracle's long-double window sums.  The observed error is printed per N so that the
    trend with N (the device forms windows from fp64 running sums) is on record."""
    worst = {}
    for even, alpha in ((False, 0.0), (False, 6.0), (True, 0.0)):
        t, y = curve(n, n + 7, even)
        periods = np.array([0.61, 2.1, 7.3, 10.0, 25.0, 33.3, 0.013 * t[-1], 0.31 * t[-1], 1.7 * t[-1], 12.0 * t[-1]])
        if even and n > 60_000:
            periods = periods[[1, 3, 6, 8]]        # (long tied runs are one oracle loop each: keep the CPU leg short)
        got = _cabi.supersmoother_scan(t, y, periods, alpha)
        want = so.supersmoother_scan(t, y, periods, alpha)
        rel = np.abs(got - want) / np.abs(want)
        worst[(even, alpha)] = float(rel.max())
        np.testing.assert_allclose(got, want, rtol=RTOL)
        assert np.array_equal(got, _cabi.supersmoother_scan(t, y, periods, alpha))
    print(f"supersmoother N={n}: max rel err vs oracle " + ", ".join(f"even={e} alpha={a}: {v:.2e}" for (e, a), v in worst.items()))


@pytest.mark.gpu
def test_supersmoother_samples_in_any_order_at_the_streamed_sizes():
    """N >= 262 144 handed over in a random order (the C ABI allows it; a TSeries never is): the device orders the
    samples by time first (csrc/timesort.inc, stable - duplicates of a time stamp keep the caller's order) and the
    result is the one for TSeries(t, y); periods beyond the baseline (written as the samples stand) included."""
    n = 300_000
    t, y = curve(n, 99)
    t[5:n:9] = t[4:n - 1:9]
    rng = np.random.default_rng(5)
    order = rng.permutation(n)
    ts, ys = t[order], y[order]
    back = np.argsort(ts, kind="stable")
    periods = np.array([2.1, 7.3, 33.3, 0.31 * t[-1], 1.7 * t[-1], 12.0 * t[-1]])
    got = _cabi.supersmoother_scan(ts, ys, periods, 0.0)
    np.testing.assert_allclose(got, so.supersmoother_scan(ts[back], ys[back], periods, 0.0), rtol=RTOL)
    assert np.array_equal(got, _cabi.supersmoother_scan(ts, ys, periods, 0.0))
    # in order, the same samples take the same kernels: the same bits
    assert np.array_equal(got, _cabi.supersmoother_scan(ts[back], ys[back], periods, 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("n,alpha", [(30_000, 0.0), (30_000, 7.0), (8_192, 0.0), (4_096, 3.0)])
def test_tiled_smoother_short_runs_of_equal_phases(n, alpha):
    """Duplicate time stamps give runs of two and three equal phases at every period: the tiled kernels (n >= 4096)
    average the fitted values over such runs from their halos - wherever the runs fall with respect to the tiles and
    the segments - and hand nothing back to the generic kernel; a tail of 300 equal stamps (a run longer than a halo)
    is the generic kernel's."""
    t, y = curve(n, 3 * n + 1)
    t[5:n:7] = t[4:n - 1:7]
    t[100:n:1001] = t[99:n - 1:1001]
    t[101:n:1001] = t[99:n - 2:1001]
    periods = np.array([0.37, 2.1, 7.3, 9.99, 31.0, 0.2 * t[-1], 2.5 * t[-1]])
    got = _cabi.supersmoother_scan(t, y, periods, alpha)
    np.testing.assert_allclose(got, so.supersmoother_scan(t, y, periods, alpha), rtol=RTOL)
    assert np.array_equal(got, _cabi.supersmoother_scan(t, y, periods, alpha))
    t[-300:] = t[-300]
    got = _cabi.supersmoother_scan(t, y, periods[:4], alpha)
    np.testing.assert_allclose(got, so.supersmoother_scan(t, y, periods[:4], alpha), rtol=RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5_000, 40_000])
def test_supersmoother_periods_that_outlast_the_samples(n):
    """p > baseline: less than one cycle, the phase order is the time order - or, with Julian-date stamps, the later
    samples first (a cycle boundary inside the samples): written as they stand by ss_direct_kernel, no sort (the
    bitonic fallback took ~200 passes over the padded curve for each such period).  Duplicated stamps keep their order."""
    t, y = curve(n, n + 3)
    t = t + 2454953.5
    t[7:n:11] = t[6:n - 1:11]
    base = t[-1] - t[0]
    periods = np.concatenate([base * np.array([0.999, 1.0, 1.001, 1.5, 2.0, 3.3, 9.99, 57.0]), [2454953.5, 2454953.5 / 2, 1e7, 1e9]])
    for alpha in (0.0, 4.0):
        got = _cabi.supersmoother_scan(t, y, periods, alpha)
        np.testing.assert_allclose(got, so.supersmoother_scan(t, y, periods, alpha), rtol=RTOL)


@pytest.mark.gpu
def test_supersmoother_class_finds_the_period_and_edges():
    t, y = curve(6000, 11)
    res = SuperSmoother(p_min=5.0, p_max=10.0, n_periods=201)(TSeries(t, y))
    assert res.size == 201 and abs(res.period[np.argmin(res.values)] - 7.3) < 0.03
    assert np.all(np.diff(res.frequency) > 0)
    with pytest.raises(ValueError):
        _cabi.supersmoother_scan(t[:4], y[:4], [1.0])                  # the woofer window needs five points
    with pytest.raises(ValueError):
        _cabi.supersmoother_scan(t, y, [1.0], alpha=11.0)
    assert _cabi.supersmoother_scan(t, y, []).size == 0
    five = _cabi.supersmoother_scan(t[:5], y[:5], [0.3, 1.7])
    np.testing.assert_allclose(five, so.supersmoother_scan(t[:5], y[:5], [0.3, 1.7]), rtol=RTOL)


@pytest.mark.gpu
def test_supersmoother_over_device_slots_equals_one_launch():
    """`devices=(...)` cuts the period grid into one slab per listed slot (the phase plan, kind 5): same values.  Also at
    bench.py's curve size with 700 periods: one call walks three batches of 256 (the last partial), each slab one batch of
    234 / 233 in sub-batches of 64 - the same segment count, so the same bits wherever a period lands."""
    t, y = curve(5000, 21)
    periods = np.linspace(3.0, 30.0, 50)
    one = _cabi.supersmoother_scan(t, y, periods, 3.0)
    many = _cabi.supersmoother_scan(t, y, periods, 3.0, devices=(0, 0, 0))
    assert np.array_equal(one, many)
    res = SuperSmoother(alpha=3.0, p_min=3.0, p_max=30.0, n_periods=50, devices=(0, 0))(TSeries(t, y))
    assert np.array_equal(res.values[::-1], one)
    t, y = curve(50_000, 23)
    periods = np.linspace(0.45, 900.0, 700)
    one = _cabi.supersmoother_scan(t, y, periods, 0.0)
    many = _cabi.supersmoother_scan(t, y, periods, 0.0, devices=(0, 0, 0))
    assert np.array_equal(one, many)


# ---- every period of grids that cross the host driver's batch and sub-batch seams (tools/ss_oracle_full.py) ---------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Per dispatch class of supersmoother_scan_impl, with the (batch / sub-batch) pdc_test_ss_shape reports for each spec and
# the seams its P periods cross.  P ends every grid in a partial batch and, where the tiled smoother runs, in a last
# sub-batch that is not a multiple of eight.  Below 1e4 samples the sub-batch IS the batch (384) and the streamed sizes
# sort one sub-batch per batch: there q0 > 0 exists only under PDC_SS_SB (the switch test below).
SEAM_SPECS = {
    # generic smoother, whole-period bitonic sort (n < 64): 384 / -
    "bitonic": ["40x1100",           # batches 384 + 384 + 332: two seams
                "63x530"],           # 384 + 146
    # LDS sort + generic smoother (64 <= n < 4096): 384 / -
    "lds_generic": ["64x800",        # 384 + 384 + 32
                    "3000x900d",     # 384 + 384 + 132, duplicated stamps
                    "4095x777e"],    # 384 + 384 + 9, tied runs
    # LDS sort + tiled smoother
    "lds_tiled": ["4096x803",        # 384 / 384: two batch seams, last sub-batch 35 (800 would end on 32 = 4 x 8)
                  "4097x787e@3",     # 384 / 384: last 19; 44 flagged periods in a row for the generic kernel's 16 workgroups
                  "5377x401",        # 384 / 384: 3 x 1792 + 1 points (a last tile of one), last batch 17
                  "12000x700d",      # 256 / 128: batches 256 + 256 + 188, sub-batches 128 + 60
                  "39999x300",       # 256 / 128: 256 + 44, the last n under the 64-period sub-batch rule
                  "40000x300"],      # 256 / 64: 4 sub-batches + 44
    # bench.py's shape and the reference's own curve size
    "bench": ["50000x4096",          # 256 / 64: 16 batches x 4 sub-batches, all full (what bench.py times)
              "50000x1003e@6",       # 256 / 64: 3 batches + 235 = 3 x 64 + 43, flagged periods in every sub-batch
              "74326x603o"],         # 128 / 64: 4 batches + 91 = 64 + 27 (600 would end on 24 = 3 x 8); Julian offset
    # streamed sort (n >= 262 144): the batch is one sub-batch
    "streamed": ["262144x150",       # 64 / 64: 64 + 64 + 22
                 "300000x203du",     # 64 / 64: 3 batches + 11 (200 would end on 8); shuffled, duplicated stamps
                 "1000000x45o"],     # 16 / 16: 16 + 16 + 13
}
SWITCH_SPECS = ["5000x300e", "50000x600e@2", "300000x96d"]
SWITCHES = [("PDC_SS_SB", "8"), ("PDC_SS_SB", "24"), ("PDC_SS_SEG", "1"), ("PDC_SS_SEG", "32"), ("PDC_SS_SEG34", "1"),
            ("PDC_SS_BATCH", "8"), ("PDC_SS_BATCH", "40"), ("PDC_SS_FASTSORT", "0"), ("PDC_WORK_BUDGET_GB", "1.5"),
            ("PDC_WORK_BUDGET_GB", "0.3")]


def ss_oracle_full(specs, timeout=900, **env):
    """tools/ss_oracle_full.py in a child process (the library reads its switches once per process): EVERY period
    against the C oracle at 1e-9, the same argmin, a second call and the reversed grid bit for bit."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ss_oracle_full.py"), *specs],
                         env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout[-4000:] + out.stderr[-2500:]
    return out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(SEAM_SPECS))
def test_supersmoother_every_period_across_batch_and_sub_batch_seams(family):
    """Default switches; which seam each spec is there for stands beside it in SEAM_SPECS.  Every grid carries periods
    beyond the baseline (ss_direct_kernel's marks are re-armed per batch), a tenth of the cadence and - even sampling -
    commensurate periods (handed back by the tiles through flag[q]) in every batch and sub-batch."""
    ss_oracle_full(SEAM_SPECS[family])


def segments_of(stdout):
    """{spec: (segments of the first two sweeps, of the last two)} from the tool's lines."""
    import re
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\S+): batch \d+ sb \d+ seg (\d+)/(\d+);", stdout, re.M)}


@pytest.fixture(scope="module")
def default_switch_run(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ss") / "default.npz")
    out = ss_oracle_full(SWITCH_SPECS, SS_CHECK_SAVE=path)
    return np.load(path), segments_of(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name,value", SWITCHES, ids=[f"{k}={v}" for k, v in SWITCHES])
def test_supersmoother_switches_every_period_and_against_the_default_run(name, value, default_switch_run, tmp_path):
    """Each launch-shape switch (and two workspace budgets): every period against the oracle, and against the default
    run at rtol 1e-12 - the bound the budget test of tests/test_multi_gpu.py holds this scan to.  What moves a result is
    the tiles' segment count (a window's running sums start elsewhere), which follows the sub-batch, which follows the
    batch and the budget; the batch origin, the sub-batch origin and the sort do not enter a period's arithmetic (the
    reversed-grid check), so a switch that leaves both segment counts of a spec alone must give the same bits.
    Measured (profiles/ss_oracle_full.txt): worst default-vs-switch difference 1.0e-14 (PDC_SS_SB=24, 300000x96d: 4 -> 11
    segments), 5e-16 at 5e4 samples; bit-identical under PDC_SS_FASTSORT=0 (all three specs), PDC_WORK_BUDGET_GB=1.5
    (5e3, 5e4) and wherever 5000 samples keep their three segments."""
    base, base_segments = default_switch_run
    path = str(tmp_path / "switch.npz")
    segments = segments_of(ss_oracle_full(SWITCH_SPECS, SS_CHECK_SAVE=path, **{name: value}))
    run = np.load(path)
    for spec in SWITCH_SPECS:
        a, b = base[spec], run[spec]
        diff = float(np.max(np.abs(a - b) / np.abs(a)))
        print(f"{name}={value} {spec}: segments {base_segments[spec]} -> {segments[spec]}, {int((a != b).sum())} of {a.size} "
              f"periods differ from the default run, max rel {diff:.2e}")
    for spec in SWITCH_SPECS:
        np.testing.assert_allclose(run[spec], base[spec], rtol=1e-12, err_msg=f"{name}={value} {spec}")
        if segments[spec] == base_segments[spec]:
            assert np.array_equal(run[spec], base[spec]), f"{name}={value} {spec}: same segments, other bits"


@pytest.mark.gpu
def test_supersmoother_dev_entry_every_period_with_a_poisoned_workspace():
    """pdc_supersmoother_scan_dev with a workspace of exactly pdc_supersmoother_work_bytes bytes filled with 0xFF: a
    read of anything a launch of THIS batch did not write shows as NaN or as a miss."""
    ss_oracle_full(["50000x600", "4097x500e", "300000x80u"], SS_FULL_DEV="1")
