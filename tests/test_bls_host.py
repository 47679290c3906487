"""BLS without a GPU: the test-local oracle (tests/bls_oracle.py) against a naive triple loop and against itself in
float64, the host class, the limits the library checks before it looks for a device.  The reference has no such class -
PARITY UNPINNED BY THE REFERENCE."""
import inspect

import numpy as np
import pytest

import bls_oracle as bo
from periodicity_amd import _cabi, phase
from periodicity_amd.core import TSeries
from periodicity_amd.phase import BLS


@pytest.mark.parametrize("dips_only", [False, True])
def test_oracle_search_is_the_naive_triple_loop(dips_only):
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0, 30, 12))
    y = rng.standard_normal(12)
    err = rng.uniform(0.5, 1.5, 12)
    for period in (2.7, 5.0, 11.3):
        for e in (err, None):
            sc = bo.scan(t, y, e, [period], 6, 1, 5, min_points=2, dtype=np.float64)
            power, table = bo.naive(t, y, e, period, 6, 1, 5, min_points=2, dips_only=dips_only)
            tab = sc.table(dips_only)[0]
            assert len(table) == int(np.sum(~np.isnan(tab))) and len(table) > 0
            for (i, L), v in table.items():
                assert abs(tab[L - 1, i] - v) <= 1e-12 * max(1.0, abs(v)), (i, L)
            assert abs(sc.power(dips_only)[0] - power) <= 1e-12


@pytest.mark.parametrize("n,n_bins,len_min,len_max", [(40, 8, 1, 7), (65, 64, 1, 63), (257, 50, 1, 6), (600, 100, 2, 10)])
def test_float64_and_longdouble_oracles_agree(n, n_bins, len_min, len_max):
    t, y, err = bo.curve(n, n)
    periods = np.linspace(2 * np.median(np.diff(t)), t[-1] - t[0], 40)
    for e in (err, None):
        p64 = bo.scan(t, y, e, periods, n_bins, len_min, len_max, dtype=np.float64)
        p80 = bo.scan(t, y, e, periods, n_bins, len_min, len_max, dtype=np.longdouble)
        for dips_only in (False, True):
            a, b = p64.power(dips_only), p80.power(dips_only)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.any(~np.isnan(b))
            assert np.nanmax(np.abs(a - b)) <= 1e-12
            assert np.all((b[~np.isnan(b)] >= 0) & (b[~np.isnan(b)] <= 1 + 1e-12))   # a share of the weighted variance


def test_oracle_nan_rules_and_the_last_bin():
    t, y, err = bo.curve(40, 1)
    assert np.all(np.isnan(bo.scan(t, np.where(np.arange(40) == 3, np.nan, y), err, [5.0], 8, 1, 3).power()))
    assert np.all(np.isnan(bo.scan(t, y, np.where(np.arange(40) == 3, 0.0, err), [5.0], 8, 1, 3).power()))
    assert np.all(np.isnan(bo.scan(t, np.zeros(40), None, [5.0], 8, 1, 3).power()))
    p = bo.scan(t, y, err, [5.0, 0.0, 6.0], 8, 1, 3).power()
    assert np.isnan(p[1]) and not np.isnan(p[0]) and not np.isnan(p[2])
    assert np.array_equal(bo.bin_index([-1e-20, 0.0, 0.5, 3.5, 4.0], 4.0, 8), [7, 0, 1, 7, 0])   # phi == 1.0: last bin


def test_class_signature_and_defaults():
    sig = inspect.signature(BLS.__init__)
    assert list(sig.parameters) == ["self", "n_bins", "q_min", "q_max", "p_min", "p_max", "n_periods", "oversample",
                                    "min_points", "dips_only", "cores", "device"]
    want = dict(n_bins=200, q_min=0.01, q_max=0.1, p_min=None, p_max=None, n_periods=1000, oversample=1, min_points=5,
                dips_only=False, cores=None, device=None)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == want
    assert sig.parameters["device"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(BLS.__call__).parameters) == ["self", "signal", "err"]
    assert "BLS" in phase.__all__
    b = BLS(64, 0.05, 0.2, 1.0, 9.0, 77, 2, 3, True, 4, device=1)
    assert (b.n_bins, b.q_min, b.q_max, b.p_min, b.p_max, b.n_periods, b.oversample, b.min_points, b.dips_only, b.cores,
            b.device) == (64, 0.05, 0.2, 1.0, 9.0, 77, 2, 3, True, 4, 1)


@pytest.mark.parametrize("n_bins,q_min,q_max,want", [(200, 0.01, 0.1, (2, 20)), (8, 0.01, 0.99, (1, 7)), (50, 0.5, 0.5, (25, 25))])
def test_box_lengths_reach_the_library_as_integers(monkeypatch, n_bins, q_min, q_max, want):
    seen = {}

    def fake(t, y, dy, periods, n_bins, len_min, len_max, min_points=5, dips_only=False, slices=0, device=None):
        seen.update(n_bins=n_bins, lens=(len_min, len_max), dy=dy, min_points=min_points, dips_only=dips_only)
        k = periods.size
        return np.full(k, 0.5), np.full(k, 0.1), np.full(k, 1, dtype=np.int32), np.full(k, len_min, dtype=np.int32)

    monkeypatch.setattr(_cabi, "bls_scan", fake)
    t, y, err = bo.curve(60, 2)
    b = BLS(n_bins, q_min, q_max, n_periods=9)
    p = b(TSeries(t, y))
    assert seen["lens"] == want and all(type(v) is int for v in seen["lens"]) and seen["n_bins"] == n_bins
    assert seen["dy"] is None and np.all(b.err == 1.0) and b.periodogram is p and p.size == 9
    # the O(n_periods) conversions: duration in time, mid-box time modulo the period
    assert np.allclose(b.duration, want[0] / n_bins * b.periods, rtol=1e-15)
    assert np.allclose(b.transit_time, ((1 + want[0] / 2) / n_bins % 1) * b.periods, rtol=1e-15)
    assert b.best["period"] == b.periods[0] and b.best["power"] == 0.5
    b(TSeries(t, y), err)
    assert seen["dy"] is not None and np.array_equal(b.err, err)


def test_every_value_error_is_raised_before_any_library_call(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_cabi, "bls_scan", never)
    for kw in (dict(q_min=0.0), dict(q_min=-0.1), dict(q_min=0.2, q_max=0.1), dict(q_max=1.0), dict(q_max=1.5),
               dict(n_bins=1), dict(n_bins=2049), dict(n_bins=10.5), dict(min_points=0), dict(min_points=-3)):
        with pytest.raises(ValueError):
            BLS(**kw)
    t, y, err = bo.curve(60, 2)
    with pytest.raises(ValueError, match="incompatible lengths"):
        BLS()(TSeries(t, y), err[:-1])
    b = BLS()
    b.q_max = 2.0            # attributes changed after construction are checked again by the call
    with pytest.raises(ValueError):
        b(TSeries(t, y), err)


def test_library_limits_and_loud_failure_without_a_device():
    assert "pdc_bls_scan" in _cabi.PROTOTYPES and "pdc_bls_scan_dev" in _cabi.PROTOTYPES
    lib = _cabi.lib()
    assert hasattr(lib, "pdc_bls_scan") and hasattr(lib, "pdc_bls_scan_dev")
    t, y, err = bo.curve(60, 2)
    periods = np.linspace(2.0, 20.0, 11)
    good = dict(n_bins=50, len_min=1, len_max=5, min_points=5, slices=0)
    for bad, text in ((dict(n_bins=1, len_max=1), "n_bins"), (dict(n_bins=2049), "n_bins"), (dict(len_max=50), "len_max"),
                      (dict(len_min=0), "len_min"), (dict(len_min=6), "len_min"), (dict(min_points=0), "min_points"),
                      (dict(slices=-1), "slices"), (dict(slices=1025), "slices")):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match=text):       # refused with a message before the library looks for a device
            _cabi.bls_scan(t, y, err, periods, **kw)
    out = np.empty(11)
    status = lib.pdc_bls_scan(_cabi._ptr(t), _cabi._ptr(y), None, -1, _cabi._ptr(periods), 11, 50, 1, 5, 5, 0, 0, _cabi._ptr(out),
                              None, None, None, 0)
    assert status == -1 and b"negative" in lib.pdc_last_error()
    with pytest.raises(ValueError):
        _cabi.bls_scan(t, y[:-1], None, periods, **good)
    if _cabi.device_count() == 0:
        with pytest.raises((RuntimeError, ValueError)):      # no GPU: the class fails loudly, never a CPU answer
            BLS()(TSeries(t, y), err)
        with pytest.raises((RuntimeError, ValueError)):
            _cabi.bls_scan(t, y, err, periods, **good)
