"""PDM.batch, AOV.batch and ConditionalEntropy.batch: many light curves, each on its own period grid, in one set
of launches (pdm_ragged.hip) - against the single-curve call, the long-double oracle and the host FSeries peak
methods."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.phase import AOV, PDM, ConditionalEntropy, _pdm_periods

pytestmark = pytest.mark.gpu

LENGTHS = [2, 3, 4, 7, 31, 64, 255, 256, 257, 1000, 5000]
NAN_CURVE, CONSTANT_CURVE = 12, 13


def catalogue(count=40, seed=5):
    """Curves of every length in LENGTHS, then random ones; negative and large time origins; one curve holding a
    NaN value and one constant curve; some with a signal near their longest trial periods (the periodogram stays
    low up to its last bin)."""
    rng = np.random.default_rng(seed)
    sigs = []
    for b in range(count):
        n = LENGTHS[b] if b < len(LENGTHS) else int(np.exp(rng.uniform(np.log(20), np.log(3000))))
        span = rng.uniform(0.5, 3.0) * n * rng.choice([0.1, 1.0, 10.0])
        t = np.sort(rng.uniform(0.0, span, n)) + rng.choice([-1.0, 1.0]) * rng.uniform(0, 1) * rng.choice([10.0, 1e6])
        period = span / (rng.uniform(1.05, 1.6) if b % 5 == 4 else rng.uniform(3.0, 40.0))
        y = 2.0 + np.sin(2 * np.pi * t / period) + 0.3 * rng.standard_normal(n)
        if b == NAN_CURVE:
            y[n // 2] = np.nan
        if b == CONSTANT_CURVE:
            y[:] = 1.5
        sigs.append(TSeries(t, y))
    return sigs


@pytest.fixture(scope="module")
def cat():
    return catalogue()


def finite_mags(sigs):
    """ConditionalEntropy()(s) refuses a curve without magnitude bins (NaN values, a constant curve)."""
    return [s for b, s in enumerate(sigs) if b not in (NAN_CURVE, CONSTANT_CURVE)]


# an explicit descending grid: FSeries(1 / periods) keeps the period order (ascending frequency) instead of reversing it
DESCENDING = dict(p_min=50.0, p_max=1.0, n_periods=300)


def scans():
    grids = [dict(), dict(n_periods=None), dict(p_min=0.7, p_max=55.0, n_periods=700), DESCENDING]
    out = []
    for g in grids:
        for nb, nc in ((5, 2), (10, 1), (20, 5)):
            for sub in (False, True):
                out.append((f"PDM{nb}x{nc}-sub{int(sub)}-{sorted(g)}", lambda g=g, nb=nb, nc=nc, sub=sub:
                            PDM(nb, nc, do_subharmonic=sub, **g)))
        out.append((f"AOV-{sorted(g)}", lambda g=g: AOV(**g)))
        out.append((f"CE-{sorted(g)}", lambda g=g: ConditionalEntropy(**g)))
    return out


SCANS = scans()


@pytest.mark.parametrize("name,make", SCANS, ids=[s[0] for s in SCANS])
def test_each_curve_is_bit_identical_to_the_single_call(cat, name, make):
    sigs = finite_mags(cat) if name.startswith("CE") else cat
    if "sub1" in name:   # (sub-harmonic averaging needs two trial periods; n_periods=None gives some curves one)
        sigs = [s for s in sigs if _pdm_periods(s, make().p_min, make().p_max, make().n_periods, 1)[0].size >= 2]
    res = make().batch(sigs)
    assert res.peaks is None and len(res.periodograms) == len(sigs)
    for b, s in enumerate(sigs):
        scan = make()
        one = scan(s)
        assert np.array_equal(res.periods[b], _pdm_periods(s, scan.p_min, scan.p_max, scan.n_periods, 1)[0])
        assert np.array_equal(res.periods[b], scan.periods)
        assert np.array_equal(res.periodograms[b].frequency, one.frequency)
        assert np.array_equal(res.periodograms[b].values, one.values, equal_nan=True), (name, b, len(s))


def test_oracle_rows(cat):
    pdm = PDM().batch(cat)
    aov = AOV().batch(cat)
    ce = ConditionalEntropy().batch(finite_mags(cat))
    for b in (4, 8, 9, 10):   # 31, 257, 1000, 5000 samples
        s = cat[b]
        p = pdm.periods[b]
        want = co.pdm_scan(s.time, s.values, p, 5, 2)
        got = pdm.periodograms[b].values[::-1]
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(aov.periodograms[b].values[::-1], co.aov_scan(s.time, s.values, p), rtol=1e-9)
        one = ConditionalEntropy()
        one(s)
        np.testing.assert_allclose(ce.periodograms[b].values[::-1], co.cond_entropy_scan(s.time, one.mag_bin, p),
                                   rtol=1e-9, atol=1e-12)


def half_max_pair(fs, rank, by_prominence):
    try:
        return fs.periods_at_half_max(rank + 1, use_prominence=by_prominence)
    except IndexError:
        return None


@pytest.mark.parametrize("grid", ["default", "descending"])
@pytest.mark.parametrize("by_prominence", [False, True])
@pytest.mark.parametrize("k", [1, 4, 200])
@pytest.mark.parametrize("kind", ["PDM", "AOV", "CE"])
def test_peak_table_matches_the_host_methods(cat, kind, k, by_prominence, grid):
    """Every curve's table against find_dips / find_peaks and periods_at_half_max of the single call's FSeries.  The
    default grid descends on the 2-sample curve (2 median_dt > baseline), the explicit one on every curve: there
    FSeries keeps the period order.  Curves whose ranked extrema share a height (short PDM / CE curves have
    piecewise-constant statistics) are compared as sets: upstream leaves the order of equal heights to argsort."""
    make = {"PDM": PDM, "AOV": AOV, "CE": ConditionalEntropy}[kind]
    kw = DESCENDING if grid == "descending" else {}
    sigs = finite_mags(cat) if kind == "CE" else cat
    lean = make(**kw).batch(sigs, peaks=k, by_prominence=by_prominence, want_power=False)
    assert lean.periodograms is None
    tab = lean.peaks
    assert tab.index.shape == (len(sigs), k)
    no_right = ordered = as_sets = 0
    for b, s in enumerate(sigs):
        one = make(**kw)(s)
        fs = one if kind == "AOV" else -one   # the dips of the statistic are the peaks of its negation
        found = fs.find_peaks()
        c = len(found)
        assert tab.count[b] == c
        assert len(one.find_dips() if kind != "AOV" else one.find_peaks()) == c
        top = min(k, c)
        assert np.all(tab.index[b, top:] == -1) and np.all(np.isnan(tab.height[b, top:]))
        if c == 0:
            continue
        idx = tab.index[b, :top]
        assert np.array_equal(tab.period[b, :top], one.period[idx])
        assert np.array_equal(tab.height[b, :top], one.values[idx])
        key = found.attrs["prominences"] if by_prominence else found.values
        ranked = np.sort(key)[::-1]
        if len(np.unique(key)) < len(key):
            # equal heights: the same ranked keys, every index one of find_peaks' own with that key
            got_key = tab.prominence[b, :top] if by_prominence else -tab.height[b, :top] if kind != "AOV" \
                else tab.height[b, :top]
            assert np.array_equal(got_key, ranked[:top])
            pos = np.searchsorted(found.attrs["indices"], idx)
            assert np.array_equal(found.attrs["indices"][pos], idx) and np.array_equal(key[pos], got_key)
            as_sets += 1
            continue
        want = fs.psort_by_prominence() if by_prominence else fs.psort_by_peak()
        assert np.array_equal(tab.period[b, :top], want[:top])
        ranks = list(range(min(top, 6))) + ([top - 1] if top > 6 else [])
        for r in ranks:
            pair = half_max_pair(fs, r, by_prominence)
            lo, hi = tab.period_lo[b, r], tab.period_hi[b, r]
            if pair is None:
                assert np.isnan(lo) or np.isnan(hi), (b, r)
                no_right += np.isnan(lo)
            else:
                assert (lo, hi) == pair, (b, r)
        ordered += 1
    assert ordered >= len(sigs) // 2, (ordered, as_sets)
    print(f"{kind} {grid} k={k} by_prominence={by_prominence}: {ordered} curves compared rank by rank, {as_sets} "
          f"with tied extrema as sets; {no_right} ranked extrema without a right-hand crossing")


def test_grids_through_zero_get_no_peak_table(cat):
    with pytest.raises(ValueError, match="curve 0"):
        PDM(p_min=-3.0, p_max=20.0).batch(cat[4:6], peaks=1)
    res = PDM(p_min=-3.0, p_max=20.0).batch(cat[4:6])   # (the periodograms are the single call's FSeries)
    assert np.array_equal(res.periodograms[0].values, PDM(p_min=-3.0, p_max=20.0)(cat[4]).values, equal_nan=True)


def test_peaks_with_and_without_power(cat):
    full = PDM(do_subharmonic=False).batch(cat, peaks=5)
    lean = PDM().batch(cat, peaks=5, want_power=False)
    for name in ("count", "index", "height", "prominence", "period", "period_lo", "period_hi"):
        assert np.array_equal(getattr(full.peaks, name), getattr(lean.peaks, name), equal_nan=True), name


def same_result(a, b):
    for pa, pb in zip(a.periodograms, b.periodograms):
        assert np.array_equal(pa.values, pb.values, equal_nan=True)
    for name in ("count", "index", "height", "prominence", "period_lo", "period_hi"):
        assert np.array_equal(getattr(a.peaks, name), getattr(b.peaks, name), equal_nan=True), name


def test_device_slots_are_bit_identical_and_cached(cat):
    one = PDM(device=0, do_subharmonic=True).batch(cat[2:], peaks=3)
    three = PDM(devices=(0, 0, 0), do_subharmonic=True).batch(cat[2:], peaks=3)
    same_result(one, three)
    before = _cabi.alloc_counts()
    again = PDM(devices=(0, 0, 0), do_subharmonic=True).batch(cat[2:], peaks=3)
    assert _cabi.alloc_counts() == before
    same_result(one, again)
    same_result(AOV().batch(cat, peaks=2), AOV(devices=(0,) * 5).batch(cat, peaks=2))


BUDGET_CHILD = r"""
import ctypes, pickle, sys
sys.path.insert(0, sys.argv[1] + "/tests")
from periodicity_amd import _cabi
from test_phase_batch_gpu import catalogue
from periodicity_amd.phase import AOV, PDM
cat = catalogue()
out = {}
if sys.argv[2] == "tiny":
    try:
        PDM().batch(cat, peaks=2)
    except ValueError as e:
        out["error"] = str(e)
else:
    for name, scan in (("pdm", PDM(10, 1, do_subharmonic=True)), ("aov", AOV())):
        r = scan.batch(cat[2:], peaks=4)
        groups = ctypes.c_int64(0)
        _cabi.check(_cabi.lib().pdc_test_phase_ragged_groups(ctypes.byref(groups)))
        out[name + "_groups"] = groups.value
        out[name] = ([p.values for p in r.periodograms],
                     {k: getattr(r.peaks, k) for k in ("count", "index", "height", "prominence", "period_lo", "period_hi")})
sys.stdout.buffer.write(pickle.dumps(out))
"""


def run_child(budget_gb, mode="run"):
    """One batch in a child process, so that PDC_WORK_BUDGET_GB (read once per process) reaches no other test."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("PDC_WORK_BUDGET_GB", None)
    if budget_gb is not None:
        env["PDC_WORK_BUDGET_GB"] = repr(budget_gb)
    proc = subprocess.run([sys.executable, "-c", BUDGET_CHILD, root, mode], env=env, capture_output=True,
                          timeout=600, cwd=root)
    assert proc.returncode == 0, proc.stderr.decode()[-2000:]
    return pickle.loads(proc.stdout)


def test_budget_groups_are_bit_identical(cat):
    ref = run_child(None)
    n = sum(len(s) for s in cat[2:])
    p = sum(r.size for r in PDM().batch(cat[2:]).periods)
    whole = 2 * 8 * n + 8 * p + _cabi.lib().pdc_phase_ragged_work_bytes(len(cat) - 2, p, 0, 0)
    small = run_child(whole / 6 / 2 ** 30)   # several groups
    assert ref["pdm_groups"] == 1 and ref["aov_groups"] == 1
    assert small["pdm_groups"] >= 3 and small["aov_groups"] >= 3, small
    for name in ("pdm", "aov"):
        for a, b in zip(ref[name][0], small[name][0]):
            assert np.array_equal(a, b, equal_nan=True)
        for key, a in ref[name][1].items():
            assert np.array_equal(a, small[name][1][key], equal_nan=True), key
    assert "budget" in run_child(1e-9, "tiny").get("error", "")


def long_curve(n=20000, seed=8):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 3000.0, n)) + 2.4e6
    return TSeries(t, np.sin(2 * np.pi * t / 37.3) + 0.5 * rng.standard_normal(n))


@pytest.mark.parametrize("make", [PDM, AOV])
def test_long_curves_agree_to_rounding(cat, make):
    s = long_curve()
    res = make().batch([cat[9], s, cat[10]])
    one = make()(s)
    assert np.array_equal(res.periods[1], _pdm_periods(s, None, None, 1000, 1)[0])
    got, want = res.periodograms[1].values, one.values
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    assert rel.max() <= 1e-12, rel.max()
    assert np.nanargmin(got) == np.nanargmin(want) and np.nanargmax(got) == np.nanargmax(want)
    assert np.array_equal(res.periodograms[0].values, make()(cat[9]).values, equal_nan=True)


def test_conditional_entropy_size_limit(cat):
    big = TSeries(np.arange(65281.0), np.cos(np.arange(65281.0) / 7.0))
    before = _cabi.alloc_counts()
    with pytest.raises(ValueError, match="65280"):
        ConditionalEntropy().batch([cat[5], big])
    assert _cabi.alloc_counts() == before
