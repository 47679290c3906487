"""GLS.batch: many light curves, each on its own grid, in one set of launches (gls_ragged.hip) - against the
single-curve call, the long-double oracle and the host FSeries peak methods."""
import numpy as np
import pytest

from oracle import c_oracle as co
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.spectral import BGLST, GLS

pytestmark = pytest.mark.gpu

LENGTHS = [2, 3, 4, 7, 31, 64, 100, 255, 256, 257, 300, 511, 1000, 2047, 3000, 5000]


def catalogue(count=64, seed=11, lengths=LENGTHS):
    """Curves of every length in `lengths` (then random ones), different baselines, cadences and time origins;
    plus a constant curve (no finite bin) and evenly sampled curves with a signal close to their Nyquist
    frequency (the spectrum rises into its last bins)."""
    rng = np.random.default_rng(seed)
    sigs, errs = [], []
    for b in range(count):
        n = lengths[b] if b < len(lengths) else int(np.exp(rng.uniform(np.log(20), np.log(3000))))
        span = rng.uniform(0.5, 3.0) * n * rng.choice([0.1, 1.0, 10.0])
        if b % 7 == 3:
            # near-even cadence (jittered: an exactly even one puts a 0/0 bin on the Nyquist frequency): the spectrum
            # about mirrors there,
            t = (np.arange(n) + rng.uniform(-0.05, 0.05, n)) * (span / n)
            period = 2.0 * (span / n) * n / (n - 0.5 * (b % 3 + 1))   # a signal half a lobe or so below it
        else:
            t = np.sort(rng.uniform(0.0, span, n))
            period = span / rng.uniform(3.0, 40.0)
        t = t + rng.uniform(-5e3, 5e3)
        dy = rng.uniform(0.05, 0.3, n)
        y = 2.0 + np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)
        if b == 40:
            y[n // 2] = np.nan                                 # no finite bin
        sigs.append(TSeries(t, y))
        errs.append(dy)
    return sigs, errs


def assert_rows_match(batch_power, single_power, n, max_rtol=1e-12):
    pb, ps = np.asarray(batch_power), np.asarray(single_power)
    assert pb.shape == ps.shape
    assert np.array_equal(np.isnan(pb), np.isnan(ps))
    fin = np.isfinite(ps)
    if not fin.any():
        return
    m = np.nanmax(ps)
    if n <= 3:
        # (three parameters fitted to <= 3 samples: every bin is 1 or 0/0 in exact arithmetic, and rounding decides
        # between 1, a huge value and inf - in either kernel)
        return
    big = fin & (np.abs(ps) > 1e-6 * abs(m))
    rel = np.abs(pb[big] - ps[big]) / np.abs(ps[big])
    assert rel.max() <= 1e-9, rel.max()
    assert abs(np.nanmax(pb) - m) <= max_rtol * abs(m)
    runner_up = np.sort(ps[fin])[-2] if fin.sum() > 1 else -np.inf
    if runner_up < m - 1e-9 * abs(m):   # (a unique maximum)
        assert np.nanargmax(pb) == np.nanargmax(ps)


def assert_tier_e(power, exact, rtol=1e-6, floor=1e-13):
    exact = np.asarray(exact)
    ok = np.abs(exact) > floor * np.nanmax(np.abs(exact))
    assert ok.mean() > 0.99
    rel = np.abs(power[ok] - exact[ok]) / np.abs(exact[ok])
    assert rel.max() <= rtol, rel.max()


@pytest.fixture(scope="module")
def cat():
    return catalogue()


@pytest.mark.parametrize("with_errs", [False, True])
@pytest.mark.parametrize("fit_mean,psd", [(True, False), (False, False), (True, True), (False, True)])
def test_each_curve_equals_the_single_call(cat, with_errs, fit_mean, psd):
    sigs, errs = cat
    errs = errs if with_errs else None
    res = GLS(psd=psd).batch(sigs, errs, fit_mean)
    assert res.peaks is None and len(res.periodograms) == len(sigs)
    for b, s in enumerate(sigs):
        one = GLS(psd=psd)(s, None if errs is None else errs[b], fit_mean)
        assert np.array_equal(res.frequency[b], one.frequency)
        assert np.array_equal(res.periodograms[b].frequency, one.frequency)
        assert_rows_match(res.periodograms[b].values, one.values, len(s))
    if with_errs and fit_mean and not psd:
        for b in (5, 9, 14, 15):   # 31, 256, 3000, 5000 samples
            exact = co.gls_power_exact(sigs[b].time, sigs[b].values, errs[b], res.frequency[b], fit_mean, psd)
            assert_tier_e(res.periodograms[b].values, exact)


def test_a_single_sample_curve_fails_as_the_single_call_does(cat):
    one = TSeries(np.array([3.0]), np.array([1.0]))
    with pytest.raises(ValueError):
        GLS()(one)
    with pytest.raises(ValueError):
        GLS().batch([cat[0][5], one])


def test_user_fixed_grid_limits(cat):
    sigs, errs = cat
    gls = GLS(fmin=0.003, fmax=0.4, n=3)
    res = gls.batch(sigs, errs)
    for b, s in enumerate(sigs):
        one = GLS(fmin=0.003, fmax=0.4, n=3)(s, errs[b])
        assert np.array_equal(res.frequency[b], one.frequency)
        # (this grid runs far past the Nyquist frequency of most curves - up to ~1e5 cycles over a baseline - where
        # the two kernels' phase rounding differs by a few 1e-12 of the row maximum)
        assert_rows_match(res.periodograms[b].values, one.values, len(s), max_rtol=1e-11)


def half_max_pair(fs, rank, by_prominence):
    try:
        return fs.periods_at_half_max(rank + 1, use_prominence=by_prominence)
    except IndexError:
        return None


@pytest.mark.parametrize("by_prominence", [False, True])
@pytest.mark.parametrize("k", [1, 5, 130])
def test_peak_table_matches_the_host_methods(cat, k, by_prominence):
    sigs, errs = cat
    res = GLS().batch(sigs, errs, peaks=k, by_prominence=by_prominence)
    tab = res.peaks
    assert tab.index.shape == (len(sigs), k) and tab.count.shape == (len(sigs),)
    assert tab.count[40] == 0 and np.all(tab.index[40] == -1) and np.all(np.isnan(tab.period[40]))
    rising = 0   # spectra above half maximum from a ranked peak to their last bin (the NaN-pad boundary)
    for b, fs in enumerate(res.periodograms):
        fs = FSeries(res.frequency[b], fs.values)
        found = fs.find_peaks()
        c = len(found)
        assert tab.count[b] == c
        top = min(k, c)
        assert np.all(tab.index[b, top:] == -1) and np.all(np.isnan(tab.height[b, top:]))
        if c == 0 or len(sigs[b]) <= 3:   # (<= 3 samples: equal heights, whose order upstream leaves to argsort)
            continue
        want = fs.psort_by_prominence() if by_prominence else fs.psort_by_peak()
        assert np.array_equal(tab.period[b, :top], want[:top])
        assert np.array_equal(tab.height[b, :top], fs.values[tab.index[b, :top]])
        assert np.array_equal(tab.frequency[b, :top], res.frequency[b][tab.index[b, :top]])
        best = fs.period_at_highest_prominence if by_prominence else fs.period_at_highest_peak
        assert tab.period[b, 0] == best
        ranks = list(range(min(top, 6))) + ([top - 1] if top > 6 else [])
        for r in ranks:
            pair = half_max_pair(fs, r, by_prominence)
            lo, hi = tab.period_lo[b, r], tab.period_hi[b, r]
            if pair is None:
                assert np.isnan(lo) or np.isnan(hi), (b, r)
                rising += np.isnan(lo)
            else:
                assert (lo, hi) == pair, (b, r)
    print(f"k={k} by_prominence={by_prominence}: {rising} ranked peaks without a right-hand half-maximum crossing")


def test_peaks_only(cat):
    sigs, errs = cat
    full = GLS().batch(sigs, errs, peaks=5, by_prominence=True)
    lean = GLS().batch(sigs, errs, peaks=5, by_prominence=True, want_power=False)
    assert lean.periodograms is None
    for name in ("count", "index", "height", "prominence", "period", "frequency", "period_lo", "period_hi"):
        assert np.array_equal(getattr(full.peaks, name), getattr(lean.peaks, name), equal_nan=True), name


def same_result(a, b):
    for pa, pb in zip(a.periodograms, b.periodograms):
        assert np.array_equal(pa.values, pb.values, equal_nan=True)
    for name in ("count", "index", "height", "prominence", "period_lo", "period_hi"):
        assert np.array_equal(getattr(a.peaks, name), getattr(b.peaks, name), equal_nan=True), name


def test_device_slots_are_bit_identical_and_cached(cat):
    sigs, errs = cat
    one = GLS(device=0).batch(sigs, errs, peaks=3)
    three = GLS(devices=(0, 0, 0)).batch(sigs, errs, peaks=3)
    same_result(one, three)
    before = _cabi.alloc_counts()
    again = GLS(devices=(0, 0, 0)).batch(sigs, errs, peaks=3)
    assert _cabi.alloc_counts() == before
    same_result(one, again)
    few = [sigs[b] for b in (8, 12, 40)]
    e_few = [errs[b] for b in (8, 12, 40)]
    same_result(GLS(device=0).batch(few, e_few, peaks=2), GLS(devices=(0,) * 5).batch(few, e_few, peaks=2))


def test_budget_groups_are_bit_identical(cat, monkeypatch):
    sigs, errs = cat
    ref = GLS().batch(sigs, errs, peaks=4)
    n = sum(len(s) for s in sigs)
    nf = sum(f.size for f in ref.frequency)
    # the slot buffer without the peak table: inputs, power and workspace, all additive over groups
    whole = 3 * 8 * n + 8 * nf + _cabi.lib().pdc_gls_ragged_work_bytes(n, len(sigs), nf, 0, 0)
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", repr(whole / 4 / 2 ** 30))   # >= 4 groups
    same_result(ref, GLS().batch(sigs, errs, peaks=4))
    plain = GLS().batch(sigs, errs)
    for pa, pb in zip(ref.periodograms, plain.periodograms):
        assert np.array_equal(pa.values, pb.values, equal_nan=True)
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "1e-6")
    with pytest.raises(ValueError, match="budget"):
        GLS().batch(sigs, errs)


def test_validation_before_device_work(cat):
    sigs, errs = cat
    before = _cabi.alloc_counts()
    with pytest.raises(ValueError):
        GLS().batch([])
    with pytest.raises(ValueError):
        GLS().batch(sigs, errs[:-1])
    with pytest.raises(NotImplementedError):
        GLS(method="fft").batch(sigs)
    with pytest.raises(NotImplementedError):
        BGLST().batch(sigs)
    assert _cabi.alloc_counts() == before


def survey(count=4096, seed=2026):
    """The survey shape of tools/gls_batch_timing.py: N log-uniform in 300 .. 5000, baselines 100 .. 3000 days,
    jittered cadences, one injected period per curve."""
    rng = np.random.default_rng(seed)
    sigs, errs, periods = [], [], []
    for b in range(count):
        n = int(np.exp(rng.uniform(np.log(300), np.log(5000))))
        span = rng.uniform(100.0, 3000.0)
        t = np.sort((np.arange(n) + rng.uniform(-0.4, 0.4, n)) * (span / n)) + rng.uniform(0, 1e4)
        period = np.exp(rng.uniform(np.log(8 * span / n), np.log(span / 8)))
        dy = rng.uniform(0.05, 0.2, n)
        y = 1.0 + np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)
        sigs.append(TSeries(t, y))
        errs.append(dy)
        periods.append(period)
    return sigs, errs, np.array(periods)


def test_survey_shape_at_full_size():
    sigs, errs, periods = survey()
    res = GLS().batch(sigs, errs, peaks=1)
    f_true = 1.0 / periods
    step = np.array([f[1] - f[0] for f in res.frequency])
    hit = np.abs(res.peaks.frequency[:, 0] - f_true) <= step
    assert hit.mean() >= 0.99, hit.mean()
    n = np.array([len(s) for s in sigs])
    pick = sorted({int(np.argmax(n)), int(np.argmin(n))} | set(range(0, 4096, 683)))[:8]
    for b in pick:
        exact = co.gls_power_exact(sigs[b].time, sigs[b].values, errs[b], res.frequency[b])
        assert_tier_e(res.periodograms[b].values, exact)
