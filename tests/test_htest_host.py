"""HTest and ZTest without a GPU: the test-local oracle (tests/htest_oracle.py) against itself in 80-bit arithmetic, the
host classes, the C ABI's argument checks.  The reference has no such class - PARITY UNPINNED BY THE REFERENCE."""
import ctypes as C
import inspect

import numpy as np
import pytest

import htest_oracle as ho
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.spectral import GLS, HTest, ZTest

SEEDS = ho.SEEDS


def default_grid(t):
    return GLS()._grid(TSeries(t, np.ones_like(t)))


@pytest.mark.parametrize("n", [5, 63, 64, 65, 129])
def test_float64_and_longdouble_oracles_agree(n):
    t, w = ho.events(n, SEEDS[n])
    freq = default_grid(t)
    for weights in (w, None):
        z64 = ho.z2(t, weights, freq, 20, np.float64)
        z80 = ho.z2(t, weights, freq, 20, np.longdouble)
        err = np.abs(z64 - z80)
        print(f"N={n} weights={weights is not None}: max err / (1e-11 Z2 + 1e-12) = {float(np.max(err / (1e-11 * z80 + 1e-12))):.3e}")
        assert np.all(err <= 1e-11 * z80 + 1e-12)
        assert np.all(np.diff(z80, axis=0) >= 0)          # cumulative in m


@pytest.mark.parametrize("n", list(SEEDS))
def test_the_values_decide_the_harmonics_of_the_test_inputs(n):
    """The GPU tests compare ``harmonics`` only where the best and the second-best candidate are more than twice the
    value gate apart, and may leave out 1 % of a case's bins: on these inputs that rule leaves out (almost) nothing."""
    t, w = ho.events(n, SEEDS[n])
    freq = default_grid(t)
    for weights in (w, None):
        left_out = int(np.sum(~ho.decided(ho.z2(t, weights, freq, 20))))
        print(f"N={n} weights={weights is not None}: {left_out} of {freq.size} bins left out")
        assert left_out <= 0.01 * freq.size


def test_a_pure_tone_picks_one_harmonic():
    """Evenly spaced phases with weights 1 + cos: C_1 = N / 2 and every higher harmonic vanishes, so Z2_1 = N / 3
    (sum w**2 = 1.5 N) and every further harmonic only pays its penalty of 4."""
    n = 400
    x = (np.arange(n) + 0.5) / n
    t = (np.arange(n) % 50 + x) * 7.3
    order = np.argsort(t)
    Z = ho.z2(t[order], (1 + np.cos(2 * np.pi * x))[order], np.array([1 / 7.3]), 20)
    h, m = ho.h_and_m(Z)
    assert m[0] == 1 and h[0] == Z[0, 0] and abs(Z[0, 0] - n / 3) <= 1e-9 * n
    assert Z[19, 0] - Z[0, 0] <= 1e-9 * n


def test_class_signatures_and_validation(monkeypatch):
    for cls, name, default in ((HTest, "max_harmonics", 20), (ZTest, "nharm", 2)):
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters)[:4] == ["self", "fmin", "fmax", "n"]
        assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in (name, "device"))
        assert sig.parameters[name].default == default and sig.parameters["n"].default == 5
        assert list(inspect.signature(cls.__call__).parameters) == ["self", "signal", "weights"]
        for bad in (0, 21, -1, 2.5, True):
            with pytest.raises(ValueError):
                cls(**{name: bad})
        obj = cls(0.01, 0.4, 3, device=1, **{name: 7})
        assert (obj.fmin, obj.fmax, obj.n, obj.device, getattr(obj, name)) == (0.01, 0.4, 3, 1, 7)
        assert not hasattr(obj, "batch") and not hasattr(obj, "bootstrap")

    def no_library_call(*args, **kwargs):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_cabi, "htest_scan", no_library_call)
    t, w = ho.events(64, 3)
    for cls in (HTest, ZTest):
        for call in (lambda: cls()(t, w[:-1]), lambda: cls()(TSeries(t, np.ones(64)), w[:5]), lambda: cls()(t, w.reshape(8, 8)),
                     lambda: cls()(t.reshape(8, 8)), lambda: cls()(t[:1])):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(AssertionError, match="the library was called"):   # a valid call does reach the binding
            cls()(t, w)


def test_the_grid_is_that_of_gls_on_the_sorted_events(monkeypatch):
    seen = {}

    def record(t, w, f0, delta, nf, **kw):
        seen.update(t=t, w=w, f0=f0, delta=delta, nf=nf, **kw)
        return np.zeros(nf), np.ones(nf, dtype=np.int32), np.zeros(nf)

    monkeypatch.setattr(_cabi, "htest_scan", record)
    t, w = ho.events(65, 4)
    order = np.random.default_rng(0).permutation(65)
    h = HTest(n=3, max_harmonics=9)
    p = h(t[order], w[order])                                  # a raw array IS the list of arrival times
    assert isinstance(p, FSeries) and h.periodogram is p and isinstance(h.z2, FSeries)
    assert np.array_equal(h.frequency, GLS(n=3)._grid(TSeries(t, np.ones(65)))) and np.array_equal(p.frequency, h.frequency)
    assert np.array_equal(seen["t"], t) and np.array_equal(seen["w"], w)     # sorted, weights follow their events
    assert np.array_equal(h.signal.time, t) and np.array_equal(h.weights, w) and h.harmonics.dtype == np.int32
    assert seen["nharm"] == 9 and set(seen["want"]) == {"h", "m", "z2"}
    assert (seen["f0"], seen["delta"], seen["nf"]) == _cabi.grid_params(h.frequency)
    z = ZTest(0.02, 0.3, nharm=1)
    z(TSeries(t, np.arange(65.0)))                             # a TSeries contributes its time stamps only
    assert np.array_equal(seen["t"], t) and seen["w"] is None and z.weights is None
    assert seen["nharm"] == 1 and tuple(seen["want"]) == ("z2",) and seen["f0"] == 0.02


def test_fap():
    from scipy.stats import chi2
    z = np.array([0.0, 1.0, 7.5, 40.0])
    for nharm in (1, 2, 20):
        np.testing.assert_allclose(ZTest(nharm=nharm).fap(z), chi2.sf(z, 2 * nharm), rtol=1e-14)
    assert ZTest(nharm=1).fap(2 * np.log(10.0)) == pytest.approx(0.1, rel=1e-12)      # Rayleigh: exp(-Z2 / 2)
    h = np.array([-3.0, 0.0, 1.0, 23.0, 109.0])
    np.testing.assert_allclose(HTest().fap(h), np.minimum(1.0, np.exp(-0.4 * h)), rtol=1e-15)
    assert HTest.fap(-3.0) == 1.0 and HTest.fap(0.0) == 1.0


def test_tile_bins():
    bins = [_cabi.htest_tile_bins(k) for k in range(1, 21)]
    assert all(b > 0 for b in bins) and all(b1 >= b0 for b0, b1 in zip(bins, bins[1:]))
    assert _cabi.htest_tile_bins(0) == -1 and _cabi.htest_tile_bins(21) == -1


def raw_scan(**kw):
    """``pdc_htest_scan`` itself, every argument by name."""
    t, w = ho.events(31, 7)
    h, m, z = np.empty(64), np.empty(64, dtype=np.int32), np.empty(64)
    a = dict(t=t, w=w, n=31, f0=0.01, delta=0.01, j_begin=0, nf=50, nharm=20, parts=0, h=h, m=m, z2=z, device=0)
    a.update(kw)
    P = _cabi._ptr
    _cabi.check(_cabi.lib().pdc_htest_scan(P(a["t"]), P(a["w"]), a["n"], a["f0"], a["delta"], a["j_begin"], a["nf"], a["nharm"],
                                           a["parts"], P(a["h"]), P(a["m"]), P(a["z2"]), a["device"]))


BAD = [dict(n=0), dict(n=-1), dict(nf=-1), dict(j_begin=-1), dict(nharm=0), dict(nharm=21), dict(parts=-1), dict(delta=0.0),
       dict(delta=-0.1), dict(delta=float("nan")), dict(delta=float("inf")), dict(h=None, m=None, z2=None),
       dict(nf=(1 << 31) * 1024), dict(t=None)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(b) for b in BAD])
def test_the_library_rejects_bad_arguments_before_it_looks_for_a_device(bad):
    with pytest.raises(ValueError, match="htest"):
        raw_scan(**bad)


def test_cabi_symbols_and_loud_failure_without_a_device():
    names = ("pdc_htest_scan", "pdc_htest_scan_dev", "pdc_htest_tile_bins", "pdc_htest_last_dispatch")
    assert all(s in _cabi.PROTOTYPES and hasattr(_cabi.lib(), s) for s in names)
    t, w = ho.events(31, 7)
    with pytest.raises(ValueError):
        _cabi.htest_scan(t, w[:-1], 0.01, 0.01, 50)
    with pytest.raises(ValueError):
        _cabi.htest_scan(t, w, 0.01, 0.01, 50, want=("h", "power"))
    raw_scan(nf=0, device=10 ** 6)                             # nothing to do: OK without touching any device
    if _cabi.device_count() == 0:
        for call in (lambda: _cabi.htest_scan(t, w, 0.01, 0.01, 50), lambda: HTest()(t, w), lambda: ZTest()(t)):
            with pytest.raises(RuntimeError):                  # no GPU: loud, never a CPU answer
                call()
