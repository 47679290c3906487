"""BLS on the GPU (csrc/bls.hip through the C ABI and the class) against the test-local oracle (tests/bls_oracle.py,
longdouble sums).  The reference has no such class - PARITY UNPINNED BY THE REFERENCE.

Gates (derived, not observed): a window sum of the device's 64-bit fixed-point scheme is within N 2^-61 of the real one
on a scale where the total weight is 1, then a few float64 roundings: power within 1e-9 |exact| + 1e-11, every period
compared, NaN positions equal.  The device's box is looked up in the oracle's table and must reach the oracle's maximum
within the same gate (robust to exact ties); its depth is the oracle's depth of THAT box within
1e-9 |d| + 1e-11 max |y'|."""
import functools

import numpy as np
import pytest

import bls_oracle as bo
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.phase import BLS
from periodicity_amd.spectral import GLS

pytestmark = pytest.mark.gpu

# (N, n_bins, len_min, len_max, n_periods): a wave and a 256-thread workgroup straddled, bin counts that are no multiple
# of 64, the full-wrap window (len_max = n_bins - 1), the largest LDS histogram
CASES = [(40, 8, 1, 7, 64), (65, 64, 1, 63, 70), (257, 50, 1, 6, 129), (1000, 200, 2, 20, 300), (3000, 2048, 20, 205, 16)]
SEEDS = {40: 21, 65: 22, 257: 23, 1000: 24, 3000: 25, 8192: 26}
MIN_POINTS = 5


@functools.lru_cache(maxsize=None)
def curve(n):
    return bo.curve(n, SEEDS[n])


def grid(n, n_periods):
    t = curve(n)[0]
    return np.linspace(2 * np.median(np.diff(t)), t[-1] - t[0], n_periods)


@functools.lru_cache(maxsize=2)
def oracle(case, with_err):
    """The oracle's tables of one case, evaluated once and shared by the tests that need them (read only)."""
    n, n_bins, len_min, len_max, n_periods = case
    t, y, err = curve(n)
    return bo.scan(t, y, err if with_err else None, grid(n, n_periods), n_bins, len_min, len_max, MIN_POINTS)


def y_scale(t, y, err):
    w, yc, _ = bo.centred(t, y, err)
    return float(np.max(np.abs(yc)))


def assert_meets_oracle(label, got, sc, dips_only, scale):
    power, depth, start, box = got
    exact = sc.power(dips_only)
    assert not np.any(np.isinf(power)) and not np.any(np.isinf(depth)), label
    assert np.array_equal(np.isnan(power), np.isnan(exact)), label
    none = np.isnan(exact)
    assert np.all(np.isnan(depth[none])) and np.all(start[none] == -1) and np.all(box[none] == -1), label
    some = np.flatnonzero(~none)
    gate = 1e-9 * np.abs(exact[some]) + 1e-11
    err = np.abs(power[some] - exact[some])
    at_box = np.array([sc.box(p, start[p], box[p], dips_only) for p in some]).reshape(-1, 2)
    err_box = np.abs(at_box[:, 0] - exact[some])
    gate_d = 1e-9 * np.abs(at_box[:, 1]) + 1e-11 * scale
    err_d = np.abs(depth[some] - at_box[:, 1])
    print(f"{label}: periods {power.size} with a box {some.size} max |power err| {err.max(initial=0):.3e} err/gate "
          f"{np.max(err / gate, initial=0):.3e}; box err/gate {np.nanmax(err_box / gate, initial=0):.3e}; depth err/gate "
          f"{np.nanmax(err_d / gate_d, initial=0):.3e}")
    assert np.all(err <= gate), (label, float(np.max(err / gate)))
    assert np.all(err_box <= gate), label            # (a NaN - a box the oracle does not admit - fails)
    assert np.all(err_d <= gate_d), label
    assert np.all((start[some] >= 0) & (box[some] >= sc.len_min)), label


@pytest.mark.parametrize("dips_only", [False, True])
@pytest.mark.parametrize("with_err", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-bins%d-len%d_%d-periods%d" % c)
def test_parity_with_the_oracle(case, with_err, dips_only):
    n, n_bins, len_min, len_max, n_periods = case
    t, y, err = curve(n)
    e = err if with_err else None
    got = _cabi.bls_scan(t, y, e, grid(n, n_periods), n_bins, len_min, len_max, MIN_POINTS, dips_only)
    assert got[0].size == n_periods and got[2].dtype == np.int32 and got[3].dtype == np.int32
    assert_meets_oracle(f"parity N={n} bins={n_bins} len={len_min}..{len_max} err={int(with_err)} dips={int(dips_only)}",
                        got, oracle(case, with_err), dips_only, y_scale(t, y, e))


@pytest.mark.parametrize("case", [CASES[2], CASES[3]], ids=lambda c: "N%d-bins%d" % c[:2])
def test_routes_are_bit_identical(case):
    """The integer scheme: one workgroup per period, the samples split over 2, 3 and 7 workgroups (3 and 7 do not divide
    N) through the global histogram, and the route chosen from the shape give the same bits - twice."""
    n, n_bins, len_min, len_max, n_periods = case
    t, y, err = curve(n)
    periods = grid(n, n_periods)
    runs = [_cabi.bls_scan(t, y, err, periods, n_bins, len_min, len_max, MIN_POINTS, False, slices=s)
            for s in (1, 2, 3, 7, 0, 1, 2, 3, 7, 0)]
    assert np.any(~np.isnan(runs[0][0]))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b, equal_nan=True)
    assert_meets_oracle(f"routes N={n}", runs[3], oracle(case, True), False, y_scale(t, y, err))


def test_route_chosen_from_the_shape_and_the_workspace_budget(monkeypatch):
    """8192 samples on 4 periods is the smallest shape at which ``slices=0`` splits the samples: same bits as one
    workgroup per period; under a budget the global histogram does not fit, the chosen route falls back and a forced
    split is refused."""
    t, y, err = curve(8192)
    periods = np.array([7.3, 3.65, 11.0, 5.1])
    one = _cabi.bls_scan(t, y, err, periods, 50, 1, 5, slices=1)
    for s in (0, 2):
        for a, b in zip(one, _cabi.bls_scan(t, y, err, periods, 50, 1, 5, slices=s)):
            assert np.array_equal(a, b, equal_nan=True)
    sc = bo.scan(t, y, err, periods, 50, 1, 5, MIN_POINTS)
    assert_meets_oracle("N=8192 auto route", one, sc, False, y_scale(t, y, err))
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "1e-6")
    for a, b in zip(one, _cabi.bls_scan(t, y, err, periods, 50, 1, 5, slices=0)):
        assert np.array_equal(a, b, equal_nan=True)
    with pytest.raises(ValueError, match="budget"):
        _cabi.bls_scan(t, y, err, periods, 50, 1, 5, slices=2)


def test_edges_of_the_bins():
    """Every phase is an exact bin edge and one is exactly 1.0 (t = -1e-20): membership must be numpy's."""
    t = np.concatenate([[-1e-20, 0.0, 0.5], np.arange(1.0, 22.0)])
    assert t.size == 24
    rng = np.random.default_rng(5)
    y = rng.standard_normal(24)
    err = rng.uniform(0.5, 1.5, 24)
    periods = np.array([4.0, 8.0, 0.5])
    assert np.any((t / 4.0) % 1 == 1.0)
    for e in (err, None):
        for len_max in (3, 7):
            got = _cabi.bls_scan(t, y, e, periods, 8, 1, len_max, 1, False)
            sc = bo.scan(t, y, e, periods, 8, 1, len_max, 1)
            assert np.any(~np.isnan(sc.power()))
            assert_meets_oracle(f"edges err={int(e is not None)} len_max={len_max}", got, sc, False, y_scale(t, y, e))


def all_nan(got):
    power, depth, start, box = got
    return bool(np.all(np.isnan(power)) and np.all(np.isnan(depth)) and np.all(start == -1) and np.all(box == -1))


def test_nan_rules():
    t, y, err = curve(257)
    periods = grid(257, 33)
    args = (50, 1, 6, MIN_POINTS)
    good = _cabi.bls_scan(t, y, err, periods, *args)
    assert not np.any(np.isnan(good[0]))
    bad_y, bad_err, zero_err = y.copy(), err.copy(), err.copy()
    bad_y[100] = np.nan
    bad_err[3] = np.nan
    zero_err[256] = 0.0
    for label, inputs in (("NaN in y", (t, bad_y, err)), ("NaN in err", (t, y, bad_err)), ("err == 0", (t, y, zero_err)),
                          # (256 unit weights: the mean of a constant is exact, so YY is exactly 0)
                          ("constant y", (t[:256], np.full(256, 3.0), None)), ("inf in y", (t, np.where(np.arange(257) == 9, np.inf, y), err))):
        for slices in (1, 2):
            assert all_nan(_cabi.bls_scan(*inputs, periods, *args, slices=slices)), label
    with_zero = periods.copy()
    with_zero[[4, 20]] = 0.0, np.nan
    for slices in (1, 3):
        got = _cabi.bls_scan(t, y, err, with_zero, *args, slices=slices)
        keep = np.ones(33, dtype=bool)
        keep[[4, 20]] = False
        assert all_nan([a[~keep] for a in got])
        for a, b in zip(got, good):
            assert np.array_equal(a[keep], b[keep])          # NaN at those periods only
        assert not np.any(np.isinf(got[0])) and not np.any(np.isinf(got[1]))
    assert all_nan(_cabi.bls_scan(t, y, err, periods, 50, 1, 6, 257))     # min_points = N: no box has N inside and outside


def test_finds_a_transit_and_measures_it():
    """A box of depth 1 over 5 % of the phase at period 7.3 (the float64 oracle gives 7.30, 0.975, 0.365 and a second
    power of 0.16 against 0.88)."""
    t, y, err = bo.curve(600, 11)
    periods = np.linspace(5.0, 10.0, 501)
    b = BLS(n_bins=100, q_min=0.02, q_max=0.1, p_min=5.0, p_max=10.0, n_periods=501, dips_only=True)
    p = b(TSeries(t, y), err)
    assert np.array_equal(b.periods, periods)
    gls = GLS()(TSeries(t, y), err)
    print(f"transit: BLS best {b.best}; GLS peak at {gls.period_at_highest_peak:.4f} (period 7.3)")
    assert abs(b.best["period"] - 7.3) <= 0.01 * 7.3
    assert abs(b.best["depth"] - 1.0) <= 0.1
    assert abs(b.best["duration"] - 0.365) <= 0.01 * b.best["period"]
    assert b.best["power"] == np.nanmax(p.values) and np.sort(p.values)[-2] < 0.5 * b.best["power"]
    # mid-transit time modulo the period: the box covers the first 5 % of the phase
    assert abs(b.best["transit_time"] - 0.025 * 7.3) <= 0.01 * b.best["period"]


def test_class_conveniences():
    t, y, err = curve(257)
    b = BLS(n_bins=50, q_min=0.02, q_max=0.12, n_periods=40)
    raw = b(y)                                                # raw arrays are wrapped as the other phase scans wrap them
    assert isinstance(raw, FSeries) and raw.size == 40 and np.all(b.err == 1.0) and b.t.size == 257
    p = b(TSeries(t, y), err)
    assert isinstance(p, FSeries) and b.periodogram is p and b.signal.size == 257
    assert np.array_equal(b.t, t) and np.array_equal(b.x, y) and np.array_equal(b.err, err)
    order = np.argsort(1 / b.periods, kind="stable")          # an FSeries is kept in ascending frequency
    assert np.array_equal(b.periods, grid(257, 40)) and np.array_equal(p.frequency, (1 / b.periods)[order])
    for name in ("power", "depth", "duration", "transit_time", "start_bin", "box_bins"):
        assert getattr(b, name).shape == (40,), name
    assert np.array_equal(p.values, b.power[order], equal_nan=True)
    want = _cabi.bls_scan(t, y, err, b.periods, 50, 1, 6, 5, False)
    assert np.array_equal(b.power, want[0], equal_nan=True) and np.array_equal(b.depth, want[1], equal_nan=True)
    found = want[2] >= 0
    assert found.any()
    assert np.array_equal(b.start_bin[found], want[2][found]) and np.all(np.isnan(b.start_bin[~found]))
    assert np.allclose(b.duration[found], want[3][found] / 50 * b.periods[found], rtol=1e-15)
    assert np.all((b.transit_time[found] >= 0) & (b.transit_time[found] < b.periods[found]))
    j = int(np.nanargmax(b.power))
    assert b.best == {"period": b.periods[j], "power": b.power[j], "depth": b.depth[j], "duration": b.duration[j],
                      "transit_time": b.transit_time[j]}
    with pytest.raises(ValueError):
        b(TSeries(t, y), err[:-1])
    starved = BLS(n_bins=50, n_periods=8, min_points=257)(TSeries(t, y), err)   # no box anywhere: NaN, not an error
    assert np.all(np.isnan(starved.values))


def test_hygiene_no_allocation_on_a_repeated_or_rejected_call():
    t, y, err = curve(1000)
    periods = grid(1000, 300)
    for slices in (1, 3):
        first = _cabi.bls_scan(t, y, err, periods, 200, 2, 20, slices=slices)
        counts = _cabi.alloc_counts()
        again = _cabi.bls_scan(t, y, err, periods, 200, 2, 20, slices=slices)
        assert _cabi.alloc_counts() == counts
        for a, b in zip(first, again):
            assert np.array_equal(a, b, equal_nan=True)
    for bad in (dict(n_bins=1), dict(n_bins=2049), dict(len_max=200), dict(min_points=0), dict(slices=1025)):
        kw = dict(n_bins=200, len_min=2, len_max=20, min_points=5, slices=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            _cabi.bls_scan(t, y, err, periods, **kw)
    assert _cabi.alloc_counts() == counts
