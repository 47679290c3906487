"""StringLength.batch: many light curves, each on its own reciprocal-linspace period grid, in one set of launches
(sl_ragged.inc) - against the single-curve call, the long-double oracle and the host FSeries dip methods."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import scan_oracle as so
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.phase import StringLength, _string_periods

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 7, 64, 255, 256, 1000, 4096, 4097, 9000, 26048]
NAN_CURVE, CONSTANT_CURVE, TIED_CURVE = 13, 14, 15
ORACLE_LENGTHS = [31, 257, 1000, 5000]


def catalogue(count=24, seed=11, long_curves=True):
    """Curves of every length in LENGTHS, then random ones; negative and large (1e6) time origins; a NaN value, a
    constant curve, tied time stamps; optionally one curve of 30 000 and one of 300 000 samples (the single call's own
    route, the streamed kernels at the larger)."""
    rng = np.random.default_rng(seed)
    sizes = LENGTHS + ORACLE_LENGTHS + [int(np.exp(rng.uniform(np.log(20), np.log(3000)))) for _ in range(count)]
    if long_curves:
        sizes += [30000, 300000]
    sigs = []
    for b, n in enumerate(sizes):
        span = rng.uniform(0.5, 3.0) * n * rng.choice([0.1, 1.0, 10.0])
        t = np.sort(rng.uniform(0.0, span, n)) + rng.choice([-1.0, 1.0]) * rng.uniform(0, 1) * rng.choice([10.0, 1e6])
        if b == TIED_CURVE:
            t = np.round(t, 0)
        period = span / rng.uniform(3.0, 40.0)
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


def stats():
    return _cabi.sl_ragged_stats()


@pytest.mark.parametrize("kw", [dict(), dict(dphi=0.37, n_periods=250), dict(dphi=2.0, n_periods=1500)],
                         ids=["default", "coarse", "fine"])
def test_each_curve_is_bit_identical_to_the_single_call(cat, kw):
    res = StringLength(**kw).batch(cat)
    assert res.peaks is None and len(res.periodograms) == len(cat)
    assert stats()[2] >= 2   # the 30 000- and 300 000-sample curves took the single call's route
    for b, s in enumerate(cat):
        one = StringLength(**kw)(s)
        got = res.periodograms[b]
        assert np.array_equal(got.values, one.values, equal_nan=True), b
        assert np.array_equal(got.frequency, one.frequency, equal_nan=True), b
        with np.errstate(divide="ignore", invalid="ignore"):
            want = _string_periods(s.baseline, kw.get("dphi", 0.1), kw.get("n_periods", 1000))
        assert np.array_equal(res.periods[b], want, equal_nan=True), b


def test_marked_periods_take_the_fallback():
    """Evenly sampled data at small integer periods crowd the phases: the ragged kernel marks those periods and the
    one-workgroup kernel works them off on the curve's slices, as in the single call."""
    rng = np.random.default_rng(3)
    t = np.arange(20001.0)
    even = TSeries(t, np.sin(2 * np.pi * t / 7.3) + 0.1 * rng.standard_normal(t.size))
    other = catalogue(4, long_curves=False)[4:8]
    scan = StringLength(dphi=1.0, n_periods=12000)
    res = scan.batch(other + [even])
    groups, marked, long_curves = stats()
    assert marked > 0 and long_curves == 0
    for b, s in enumerate(other + [even]):
        assert np.array_equal(res.periodograms[b].values, StringLength(dphi=1.0, n_periods=12000)(s).values,
                              equal_nan=True), b


def test_oracle_rows(cat):
    res = StringLength().batch(cat)
    for n in ORACLE_LENGTHS:
        b = len(LENGTHS) + ORACLE_LENGTHS.index(n)
        s = cat[b]
        assert s.size == n
        want = co.stringlength_scan(s.time, so.stringlength_scale(np.asarray(s.values, dtype=float)), res.periods[b])
        np.testing.assert_allclose(res.periodograms[b].values[::-1], want, rtol=1e-9)


def half_max_pair(fs, rank, by_prominence):
    try:
        return fs.periods_at_half_max(rank + 1, use_prominence=by_prominence)
    except IndexError:
        return None


@pytest.mark.parametrize("want_power", [False, True])
@pytest.mark.parametrize("by_prominence", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_peak_table_matches_the_host_methods(cat, k, by_prominence, want_power):
    sigs = [s for b, s in enumerate(cat) if b not in (NAN_CURVE, CONSTANT_CURVE) and s.size >= 2]
    res = StringLength().batch(sigs, peaks=k, by_prominence=by_prominence, want_power=want_power)
    assert (res.periodograms is None) == (not want_power)
    tab = res.peaks
    assert tab.index.shape == (len(sigs), k)
    compared = 0
    for b, s in enumerate(sigs):
        one = StringLength()(s)
        dips = one.find_dips()
        c = len(dips)
        assert tab.count[b] == c, b
        top = min(k, c)
        assert np.all(tab.index[b, top:] == -1) and np.all(np.isnan(tab.height[b, top:]))
        if c == 0:
            continue
        fs = -one
        found = fs.find_peaks()
        key = found.attrs["prominences"] if by_prominence else found.values
        order = np.argsort(key, kind="stable")[::-1]
        if len(np.unique(key)) < len(key):
            continue   # tied extrema: upstream leaves their order to argsort
        idx = found.attrs["indices"][order[:top]]
        assert np.array_equal(tab.index[b, :top], idx), b
        assert np.array_equal(tab.frequency[b, :top], one.frequency[idx]), b
        assert np.array_equal(tab.height[b, :top], one.values[idx]), b
        assert np.array_equal(tab.prominence[b, :top], found.attrs["prominences"][order[:top]]), b
        for r in range(top):
            pair = half_max_pair(fs, r, by_prominence)
            lo, hi = tab.period_lo[b, r], tab.period_hi[b, r]
            if pair is None:
                assert np.isnan(lo) or np.isnan(hi), (b, r)
            else:
                assert (lo, hi) == pair, (b, r)
        compared += 1
    assert compared >= len(sigs) // 2


def same_result(a, b):
    for pa, pb in zip(a.periodograms, b.periodograms):
        assert np.array_equal(pa.values, pb.values, equal_nan=True)
    for name in ("count", "index", "height", "prominence", "period_lo", "period_hi"):
        assert np.array_equal(getattr(a.peaks, name), getattr(b.peaks, name), equal_nan=True), name


def test_device_slots_are_bit_identical(cat):
    sigs = cat[1:]   # (the 1-sample curve has no baseline, so no frequency step and no peak table)
    one = StringLength(device=0).batch(sigs, peaks=3)
    three = StringLength(devices=(0, 0, 0)).batch(sigs, peaks=3)
    same_result(one, three)


BUDGET_CHILD = r"""
import pickle, sys
sys.path.insert(0, sys.argv[1] + "/tests")
from periodicity_amd import _cabi
from test_sl_batch_gpu import catalogue
from periodicity_amd.phase import StringLength, _string_periods
cat = [s for s in catalogue(long_curves=False)[1:] if s.size <= 5000]
r = StringLength().batch(cat, peaks=3)
out = {"groups": _cabi.sl_ragged_stats()[0], "rows": [p.values for p in r.periodograms],
       "table": {k: getattr(r.peaks, k) for k in ("count", "index", "height", "prominence", "period_lo", "period_hi")}}
sys.stdout.buffer.write(pickle.dumps(out))
"""


def run_child(budget_gb):
    """One batch in a child process, so that PDC_WORK_BUDGET_GB (read once per process) reaches no other test."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("PDC_WORK_BUDGET_GB", None)
    if budget_gb is not None:
        env["PDC_WORK_BUDGET_GB"] = repr(budget_gb)
    proc = subprocess.run([sys.executable, "-c", BUDGET_CHILD, root], env=env, capture_output=True, timeout=600,
                          cwd=root)
    assert proc.returncode == 0, proc.stderr.decode()[-2000:]
    return pickle.loads(proc.stdout)


def test_budget_groups_are_bit_identical():
    sigs = [s for s in catalogue(long_curves=False)[1:] if s.size <= 5000]   # (the child's catalogue)

    def group_bytes(curves):   # (about: inputs, rows and the workspace; the peak table is small)
        offsets = np.concatenate([[0], np.cumsum([s.size for s in curves])]).astype(np.int64)
        poff = np.arange(len(curves) + 1, dtype=np.int64) * 1000
        lib = _cabi.lib()
        return 16 * offsets[-1] + 8 * poff[-1] + lib.pdc_stringlength_ragged_work_bytes(_cabi._ptr(offsets),
                                                                                        _cabi._ptr(poff), len(curves))

    whole, largest = group_bytes(sigs), group_bytes([max(sigs, key=lambda s: s.size)])
    assert whole > 1.15 * largest
    ref = run_child(None)
    small = run_child(float((whole + largest) / 2 / 2 ** 30))   # (above the largest curve's own group)
    assert ref["groups"] == 1 and small["groups"] > 1, (ref["groups"], small["groups"])
    for a, b in zip(ref["rows"], small["rows"]):
        assert np.array_equal(a, b, equal_nan=True)
    for key, a in ref["table"].items():
        assert np.array_equal(a, small["table"][key], equal_nan=True), key
