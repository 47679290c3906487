"""The discrete correlation function without a GPU: the test-local oracle (tests/dcf_oracle.py) against the reference's
FFT autocorrelation on an evenly sampled curve and against hand counts, the host class - its argument rules, its lag
grid, its defaults, its two normalisations, its peak rules - on sums the oracle provides, and the size functions of the
C ABI.  The reference has no such statistic - PARITY UNPINNED BY THE REFERENCE."""
import inspect

import numpy as np
import pytest

import dcf_oracle as do
import dcf_raw as raw
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.correlation import DCF


def _fake_scan(calls):
    """``_cabi.dcf_scan`` answered by the oracle in float64 (the class's own arithmetic is what these tests look at)."""
    def scan(ta, a, tb, b, edges, skip_same_index=False, chunk=0, device=None):
        calls.append(dict(ta=ta, a=a, tb=tb, b=b, edges=edges, skip=skip_same_index, same=ta is tb and a is b))
        o = do.scan(ta, a, tb, b, edges, skip_same_index)
        return o.pairs, o.sums.astype(np.float64)
    return scan


def test_oracle_on_an_even_curve_is_the_fft_acf_of_the_reference():
    t, x = do.random_walk(600)
    o = do.scan(t, x, t, x, -0.5 + np.arange(301))
    assert np.array_equal(o.pairs, 600 - np.arange(300))
    dcf = (o.sums[4] / (o.pairs * np.var(x))).astype(np.float64)
    err = np.max(np.abs(dcf - do.fft_acf(x, 300)))
    print(f"oracle DCF vs FFT ACF, 300 lags of 600 samples: {err:.1e}")
    assert err <= 1e-12


def test_a_pair_on_an_edge_goes_to_the_bin_it_opens():
    t, x = do.random_walk(600)
    o = do.scan(t, x, t, x, 0.0 + np.arange(11), skip_same_index=True)
    assert o.pairs.tolist() == [0] + list(range(599, 590, -1))
    assert np.all(o.sums[:, 0] == 0) and np.all(o.abs_sums[:, 0] == 0)


def test_float64_accumulation_sits_far_inside_the_gate():
    t, x = do.random_walk(600)
    edges = -0.5 + np.arange(301)
    exact = do.scan(t, x, t, x, edges)
    plain = do.scan(t, x, t, x, edges, dtype=np.float64)
    ratio = do.worst_ratio(plain.pairs, plain.sums, exact)
    print(f"float64 np.add.at / gate: {ratio:.3f}")
    assert ratio <= 0.25


def test_shared_inputs_pair_counts_and_the_wandering_sinusoid():
    """The figures of the inputs both test files share.  The uneven case is built as its issue states it
    (``default_rng(1)``, ``sort(uniform(0, 100, 500)) + 2450000``, edges ``0.37 arange(65)``, diagonal skipped); the
    counts that issue quotes for it (681 to 973 a bin, 51 951 in all) are not reproducible from that generator, which
    gives 692 to 949 and 52 389.  The wandering sinusoid gives the issue's figures: lag 16.0, prominences 0.74, 0.63."""
    t, x, edges = do.uneven_auto()
    o = do.scan(t, x, t, x, edges, skip_same_index=True)
    assert (o.pairs.min(), o.pairs.max(), o.pairs.sum()) == (692, 949, 52389)
    t, y = do.wandering_sinusoid()
    lags = np.arange(61.0)
    o = do.scan(t, y - y.mean(), t, y - y.mean(), -0.5 + np.arange(62.0), skip_same_index=True)
    dcf = (o.sums[4] / (o.pairs * np.var(y))).astype(np.float64)
    period, res = do.period_rule(lags, dcf)
    top = np.sort(res["prominences"])[::-1]
    print(f"wandering sinusoid: period {period}, prominences {top[0]:.2f} and {top[1]:.2f}")
    assert period == 16.0 and abs(period - 17.3) <= 1.5
    assert abs(top[0] - 0.74) < 0.005 and abs(top[1] - 0.63) < 0.005


def test_class_signature_and_validation(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refused argument reached the library")
    monkeypatch.setattr(_cabi, "dcf_scan", no_device)
    sig = inspect.signature(DCF.__init__)
    assert list(sig.parameters)[1:7] == ["max_lag", "dlag", "min_lag", "normalization", "min_pairs", "include_self"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[1:7]] == [None, None, None, "global", 2, False]
    assert list(inspect.signature(DCF.__call__).parameters)[1:] == ["signal", "other", "err", "other_err"]
    for kw in (dict(normalization="pearson"), dict(min_pairs=1), dict(min_pairs=2.5), dict(dlag=0.0), dict(dlag=-1.0),
               dict(dlag=np.nan), dict(max_lag=np.inf), dict(min_lag=np.nan)):
        with pytest.raises(ValueError):
            DCF(**kw)
    t, x = do.random_walk(50)
    s = TSeries(t, x)
    with pytest.raises(ValueError):
        DCF(max_lag=1.0, min_lag=2.0)(s)
    with pytest.raises(ValueError):
        DCF()(TSeries([0.0], [1.0]))
    with pytest.raises(ValueError):
        DCF()(s, err=np.ones(49))
    with pytest.raises(ValueError):
        DCF()(s, other_err=np.ones(50))          # no other curve
    with pytest.raises(ValueError):
        DCF()(s, s, other_err=np.ones(49))
    # the error variance exceeds the variance: no global normalisation
    with pytest.raises(ValueError, match="variance"):
        DCF()(s, err=np.full(50, 2 * np.std(x)))
    with pytest.raises(ValueError, match="variance"):
        DCF()(s, TSeries(t, x), other_err=np.full(50, 2 * np.std(x)))


def test_grid_defaults_and_fields(monkeypatch):
    calls = []
    monkeypatch.setattr(_cabi, "dcf_scan", _fake_scan(calls))
    rng = np.random.default_rng(5)
    ta = np.sort(rng.uniform(0, 40, 90))
    a = rng.standard_normal(90) + 3.0
    sa = TSeries(ta, a)
    # one curve: dlag = median_dt, max_lag = half the baseline, min_lag = 0, the diagonal left out
    d = DCF()
    out = d(sa)
    dlag, max_lag = sa.median_dt, 0.5 * sa.baseline
    nlag = int(np.floor(max_lag / dlag)) + 1
    assert np.array_equal(d.lags, 0.0 + dlag * np.arange(nlag))
    assert np.array_equal(d.edges, (0.0 - 0.5 * dlag) + dlag * np.arange(nlag + 1))
    assert calls[-1]["skip"] is True and calls[-1]["same"] and np.array_equal(calls[-1]["a"], a - a.mean())
    assert out is d.correlogram and isinstance(out, TSeries)
    assert np.array_equal(out.time, d.lags) and np.array_equal(out.values, d.dcf, equal_nan=True)
    assert d.signal is sa and d.other is None and sorted(d.sums) == sorted(do.SUMS) and d.pairs.dtype == np.int64
    assert DCF(include_self=True)(sa) is not None and calls[-1]["skip"] is False
    # an array is values on arange times, as for GLS
    DCF()(a)
    assert np.array_equal(calls[-1]["ta"], np.arange(90.0))
    # two curves: the larger median_dt, half the shorter baseline, lags from -max_lag, nothing left out
    tb = np.sort(rng.uniform(5, 30, 40))
    sb = TSeries(tb, rng.standard_normal(40))
    c = DCF()
    c(sa, sb)
    dlag, max_lag = max(sa.median_dt, sb.median_dt), 0.5 * min(sa.baseline, sb.baseline)
    nlag = int(np.floor((max_lag + max_lag) / dlag)) + 1
    assert np.array_equal(c.lags, -max_lag + dlag * np.arange(nlag))
    assert np.array_equal(c.edges, (-max_lag - 0.5 * dlag) + dlag * np.arange(nlag + 1))
    assert calls[-1]["skip"] is False and not calls[-1]["same"] and c.other is sb
    assert np.array_equal(calls[-1]["b"], sb.values - sb.values.mean())
    with pytest.raises(ValueError):
        c.period
    # explicit grid
    e = DCF(max_lag=7.0, dlag=0.5, min_lag=-2.0)
    e(sa, sb)
    assert np.array_equal(e.lags, -2.0 + 0.5 * np.arange(19)) and e.edges.size == 20
    twin = e.copy()
    assert twin is not e and np.array_equal(twin.dcf, e.dcf, equal_nan=True) and twin.lags is not e.lags


def test_both_normalisations_against_hand_formulas(monkeypatch):
    monkeypatch.setattr(_cabi, "dcf_scan", _fake_scan([]))
    rng = np.random.default_rng(6)
    ta, tb = np.sort(rng.uniform(0, 40, 120)), np.sort(rng.uniform(0, 40, 80))
    a, b = rng.standard_normal(120), rng.standard_normal(80) * 2 + 1
    ea, eb = np.full(120, 0.3), rng.uniform(0.1, 0.4, 80)
    g = DCF(max_lag=10.0, dlag=0.25, min_pairs=40)
    g(TSeries(ta, a), TSeries(tb, b), ea, eb)
    o = do.scan(ta, a - a.mean(), tb, b - b.mean(), g.edges)
    n = o.pairs.astype(float)
    Sa, Sb, Saa, Sbb, Sab, Sabab = o.sums.astype(np.float64)
    norm = np.sqrt((np.var(a) - np.mean(ea ** 2)) * (np.var(b) - np.mean(eb ** 2)))
    few = o.pairs < 40
    assert few.any() and not few.all()
    assert np.array_equal(np.isnan(g.dcf), few) and np.array_equal(np.isnan(g.sigma), few)
    dcf = Sab / (n * norm)
    sigma = np.sqrt(np.maximum(Sabab / norm ** 2 - n * dcf ** 2, 0)) / (n - 1)
    assert np.array_equal(g.dcf[~few], dcf[~few]) and np.array_equal(g.sigma[~few], sigma[~few])
    loc = DCF(max_lag=10.0, dlag=0.25, normalization="local")
    loc(TSeries(ta, a), TSeries(tb, b))
    few = o.pairs < 2
    r = (Sab / n - (Sa / n) * (Sb / n)) / np.sqrt((Saa / n - (Sa / n) ** 2) * (Sbb / n - (Sb / n) ** 2))
    assert np.allclose(loc.dcf[~few], r[~few], rtol=1e-13, atol=0) and np.all(np.abs(loc.dcf[~few]) <= 1 + 1e-12)
    assert np.allclose(loc.sigma[~few], ((1 - r ** 2) / np.sqrt(n - 1))[~few], rtol=1e-12, atol=1e-15)
    # Pearson's r of a bin's own pairs, the long way
    k = int(np.argmax(o.pairs))
    ai, bj = (a - a.mean())[o.i[o.k == k]], (b - b.mean())[o.j[o.k == k]]
    assert abs(loc.dcf[k] - np.corrcoef(ai, bj)[0, 1]) <= 1e-12


def test_peak_lag_and_period_rules(monkeypatch):
    monkeypatch.setattr(_cabi, "dcf_scan", _fake_scan([]))
    t, y = do.wandering_sinusoid()
    d = DCF(max_lag=60.0, dlag=1.0)
    d(TSeries(t, y))
    assert d.period == do.period_rule(d.lags, d.dcf)[0] == 16.0
    assert d.peak_lag == float(d.lags[np.nanargmax(d.dcf)])
    # ties: the smaller |lag| for the largest value, the smaller lag for the most prominent peak; NaN bins are dropped
    d.lags = np.arange(-4.0, 9.0)
    d.dcf = np.array([0.9, 0.1, 0.9, np.nan, 0.2, 0.1, 0.5, 0.2, 0.5, 0.1, np.nan, 0.3, 0.1])
    assert d.peak_lag == -2.0
    assert d.period == 2.0                       # lags 2 and 4: prominence 0.4 each; lag 7 (across the NaN bin): 0.2
    d.dcf = np.array([np.nan, 0.1, 0.2, np.nan, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0])
    assert d.period is None and d.peak_lag == 8.0
    d.dcf = np.full(13, np.nan)
    assert d.peak_lag is None and d.period is None


def test_size_functions_and_loud_failure_without_a_device(monkeypatch):
    for name in ("pdc_dcf_scan", "pdc_dcf_scan_dev", "pdc_dcf_work_bytes", "pdc_dcf_chunk", "pdc_dcf_last_dispatch"):
        assert name in _cabi.PROTOTYPES and hasattr(_cabi.lib(), name)
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    small = _cabi.dcf_work_bytes(500, 500, 64)
    assert small >= 7 * 8 * 64
    assert _cabi.dcf_work_bytes(500, 500, 65) > small and _cabi.dcf_work_bytes(500, 500, 1000) > small
    assert _cabi.dcf_work_bytes(500, 500, 64, chunk=1) >= 500 * 7 * 8 * 64        # a slab per chunk
    assert _cabi.dcf_work_bytes(0, 0, 1) > 0 and _cabi.dcf_work_bytes(0, 500, 64) > 0
    for bad in ((-1, 5, 4, 0), (5, -1, 4, 0), (5, 5, 0, 0), (5, 5, -3, 0), (5, 5, (1 << 22) + 1, 0), (5, 5, 4, -1),
                (1 << 31, 5, 4, 0), (5, (1 << 31) - 63, 4, 0)):
        assert _cabi.dcf_work_bytes(*bad) == -1
    assert _cabi.dcf_chunk(-1, 5, 4) == -1 and _cabi.dcf_chunk(5, 5, 0) == -1
    for shape in ((1, 1, 1), (500, 500, 64), (10_000, 10_000, 1000), (100_000, 100_000, 1000), (0, 5, 3)):
        assert _cabi.dcf_chunk(*shape) >= 1
    assert _cabi.dcf_chunk(100_000, 100_000, 1000) < 100_000                      # more than one chunk
    # a budget enlarges the chunk until the slabs fit
    big = (1_000_000, 1_000_000, 1000)
    free, free_chunk = _cabi.dcf_work_bytes(*big), _cabi.dcf_chunk(*big)
    assert 1 << 25 < free <= 1 << 31                                                # (the library's own cap: 2 GiB)
    for gb, cap in (("0.03125", 1 << 25), ("0.0078125", 1 << 23)):
        monkeypatch.setenv("PDC_WORK_BUDGET_GB", gb)
        assert 0 < _cabi.dcf_work_bytes(*big) <= cap and _cabi.dcf_chunk(*big) > free_chunk
        assert 0 < _cabi.dcf_work_bytes(*big, chunk=1) <= cap                       # a forced chunk too
        assert _cabi.dcf_work_bytes(500, 500, 64) == small                          # a scan that fits is not touched
    monkeypatch.delenv("PDC_WORK_BUDGET_GB")
    assert _cabi.dcf_work_bytes(*big) == free
    assert _cabi.dcf_last_dispatch() == (0, 0) or _cabi.device_count() > 0          # zeros before the first scan

    t, x, edges = do.uneven_auto()
    good = dict(ta=t, a=x, tb=t, b=x, edges=edges)
    # arguments the library refuses before it looks for a device
    for kw in (dict(edges=edges[:1]), dict(edges=np.array([])), dict(edges=edges[::-1]),
               dict(edges=np.where(np.arange(65) == 9, edges[8], edges)), dict(edges=np.where(np.arange(65) == 64, np.inf, edges)),
               dict(edges=np.where(np.arange(65) == 3, np.nan, edges)), dict(ta=t[::-1]), dict(tb=t[::-1].copy()),
               dict(ta=np.where(np.arange(500) == 7, np.nan, t)), dict(tb=np.where(np.arange(500) == 499, np.inf, t)),
               dict(tb=t[:-1], b=x[:-1], skip_same_index=True), dict(chunk=-1), dict(a=x[:-1]), dict(b=x[:-1])):
        with pytest.raises(ValueError):
            _cabi.dcf_scan(**{**good, **kw})
    # ... and what the wrapper cannot say (negative sizes, NULL outputs and inputs), through both entries themselves
    for refused in raw.refusals(t, x, edges):
        for entry in (raw.raw_scan, raw.raw_scan_dev):
            with pytest.raises(ValueError):
                entry(**refused)
    with pytest.raises(ValueError, match="chunks"):      # 2^24 chunks: refused by the count, before an array is read
        raw.raw_scan(t, x, t, x, edges, na=1 << 24, nb=1 << 24, skip=1, chunk=1)
    assert _cabi.dcf_work_bytes(1 << 24, 1 << 24, 64, chunk=1) == -1 and _cabi.dcf_work_bytes(1 << 24, 1 << 24, 64, chunk=2) > 0
    if _cabi.device_count() == 0:
        # the product path fails loudly and never answers from the CPU - an empty curve included
        with pytest.raises(RuntimeError):
            _cabi.dcf_scan(**good)
        with pytest.raises(RuntimeError):
            _cabi.dcf_scan(t[:0], x[:0], t, x, edges)
        with pytest.raises(RuntimeError):
            DCF()(TSeries(t, x))
