"""WWZ without a GPU: the test-local oracle (tests/wwz_oracle.py) against the project's exact GLS oracle, the host class
and its argument rules, the WWZMap fields, the size functions of the C ABI.  The reference has no such statistic -
PARITY UNPINNED BY THE REFERENCE."""
import inspect

import numpy as np
import pytest

import mhgls_oracle as mo
import wwz_oracle as wo
from oracle import scan_oracle as so
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.spectral import GLS
from periodicity_amd.timefrequency import WWZ, WWZMap


def test_oracle_without_a_window_is_the_exact_gls_power(golden_dir):
    """decay = 0: every window weight is 1, Neff = N and WWZ = (N - 3) p / (2 (1 - p)) with p the floating-mean GLS
    power, checked at 1e-12 relative.  Bins whose fit is singular (the Nyquist bin of integer times) are left out as
    tests/mhgls_oracle.py leaves them out.  The exact power is a float64 formed from sums of size 1: its rounding,
    1.1e-16, enters the expected WWZ as 1.1e-16 (N - 3) / (2 (1 - p)^2).  So the bins next to the peak of this noiseless
    sine (1 - p < 1e-3) are left out too, and the gate has the floor 1e-14 = 1.1e-16 x 48.5 x 2 for the bins whose
    power is zero to rounding (p = 4e-32 occurs)."""
    g = np.load(f"{golden_dir}/g2_sine100.npz")
    t = np.arange(100.0)
    freq, exact = so.gls(t, g["values"], sums="exact")
    p = np.asarray(exact, dtype=np.longdouble)
    keep = (mo.cond(t, g["values"], None, freq, 1) <= mo.COND_LIMIT) & (1 - p >= 1e-3)
    assert keep.mean() >= 0.95
    with np.errstate(divide="ignore"):
        want = 97 * p / (2 * (1 - p))
    for tau in (0.0, 50.0, 1e3):   # without a window the shift does not enter
        z, _, neff = wo.planes(t, g["values"], None, freq, [tau], decay=0.0)
        z, neff = z[0], neff[0]
        assert np.max(np.abs(neff - 100)) <= 1e-12
        assert np.all(np.abs(z[keep] - want[keep]) <= 1e-12 * np.abs(want[keep]) + 1e-14)
    assert int(np.nanargmax(z)) == int(g["argmax"])


def test_float64_and_longdouble_oracles_agree_far_inside_the_gate():
    t, y, err, freq, tau = wo.chirp_curve()
    for e in (None, err):
        for decay in (wo.FOSTER, 0.005):
            exact = wo.planes(t, y, e, freq, tau, decay)
            double = wo.planes(t, y, e, freq, tau, decay, dtype=np.float64)
            for got, want in zip(double, exact):
                worst, left_out = wo.compare(got, want, exact[2])
                assert worst <= 1e-3 and left_out <= wo.LEFT_OUT_CAP


def test_oracle_amplitude_of_a_clean_sinusoid():
    t = np.sort(np.random.default_rng(1).uniform(0, 50, 400))
    y = 3.0 + 0.7 * np.sin(2 * np.pi * 0.4 * t + 0.3)
    z, a, neff = wo.planes(t, y, None, [0.4], [25.0])
    assert abs(float(a[0, 0]) - 0.7) <= 1e-12 and float(neff[0, 0]) > 6 and float(z[0, 0]) > 1e15


def test_reductions_follow_nanargmax():
    wwz = np.array([[1.0, 5.0, 5.0, np.nan], [np.nan, 2.0, 9.0, 1.0], [1.0, 2.0, 3.0, 4.0]])
    neff = np.array([[9.0, 9.0, 9.0, 9.0], [9.0, 9.0, 1.0, 9.0], [1.0, 1.0, 1.0, 1.0]])
    bins, rz, ra, best = wo.reductions(wwz, 2 * wwz, neff)
    assert bins.tolist() == [1, 1, -1]
    assert rz[:2].tolist() == [5.0, 2.0] and np.isnan(rz[2]) and ra[0] == 10.0
    assert best == (5.0, 0, 1)
    assert wo.reductions(wwz, wwz, neff, min_neff=10)[3][1:] == (-1, -1)


def _fake_scan(calls):
    def scan(t, y, dy, f0, delta, nf, tau, decay, min_neff, want_planes=True, device=None):
        calls.append(dict(t=t, y=y, dy=dy, f0=f0, delta=delta, nf=nf, tau=np.array(tau), decay=decay,
                          min_neff=min_neff, want_planes=want_planes, device=device))
        ntau = len(tau)
        plane = np.arange(ntau * nf, dtype=float).reshape(ntau, nf) if want_planes else None
        bins = np.full(ntau, nf - 1, dtype=np.int64)
        bins[0] = -1
        return dict(wwz=plane, amp=plane, neff=plane, ridge_bin=bins, ridge_wwz=np.arange(ntau, dtype=float),
                    ridge_amp=np.arange(ntau, dtype=float) / 2, best=(float(ntau - 1), ntau - 1, nf - 1), visited=7)
    return scan


def test_class_signature_and_validation(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("reached the library")

    monkeypatch.setattr(_cabi, "wwz_scan", no_device)
    sig = inspect.signature(WWZ.__init__)
    assert list(sig.parameters)[:4] == ["self", "fmin", "fmax", "n"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("decay", "min_neff", "device"))
    assert sig.parameters["decay"].default == 1 / (8 * np.pi ** 2) and sig.parameters["min_neff"].default == 6.0
    call = inspect.signature(WWZ.__call__)
    assert list(call.parameters) == ["self", "signal", "err", "taus", "want_planes"]
    assert call.parameters["taus"].default == 64 and call.parameters["want_planes"].default is True
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            WWZ(decay=bad)
    with pytest.raises(ValueError):
        WWZ(min_neff=np.nan)
    t, y, err, _, _ = wo.chirp_curve()
    s = TSeries(t, y)
    for kw in (dict(err=err[:-1]), dict(taus=0), dict(taus=[]), dict(taus=[1.0, np.nan]), dict(taus=[[1.0, 2.0]]),
               dict(taus=[np.inf])):
        with pytest.raises(ValueError):
            WWZ()(s, **kw)
    with pytest.raises(ValueError):
        WWZ()(TSeries(t[:3], y[:3]))
    w = WWZ(0.05, 0.45, 3, decay=0.005, min_neff=4, device=1)
    assert (w.fmin, w.fmax, w.n, w.decay, w.min_neff, w.device) == (0.05, 0.45, 3, 0.005, 4.0, 1)
    assert np.array_equal(w._grid(s), GLS(0.05, 0.45, 3)._grid(s))   # GLS's grid, unchanged
    assert not hasattr(WWZ, "batch")


def test_taus_rule_and_map_fields(monkeypatch):
    calls = []
    monkeypatch.setattr(_cabi, "wwz_scan", _fake_scan(calls))
    t, y, err, _, _ = wo.chirp_curve()
    s = TSeries(t, y)
    w = WWZ(0.05, 0.45, 5, min_neff=5, device=2)
    m = w(s, err, taus=7)
    assert isinstance(m, WWZMap) and w.map is m
    c = calls[-1]
    assert np.array_equal(c["tau"], np.linspace(t[0], t[-1], 7)) and np.array_equal(m.tau, c["tau"])
    freq = GLS(0.05, 0.45, 5)._grid(s)
    assert np.array_equal(m.frequency, freq) and c["nf"] == freq.size and c["f0"] == freq[0]
    assert np.array_equal(c["f0"] + np.arange(c["nf"]) * c["delta"], freq)
    assert (c["decay"], c["min_neff"], c["device"], c["want_planes"]) == (1 / (8 * np.pi ** 2), 5.0, 2, True)
    assert c["dy"] is not None and np.array_equal(c["dy"], err)
    assert m.wwz.shape == m.amplitude.shape == m.neff.shape == (7, freq.size)
    assert m.ridge_bin.tolist() == [-1] + [freq.size - 1] * 6
    assert np.isnan(m.ridge_frequency[0]) and np.isnan(m.ridge_period[0])
    assert np.all(m.ridge_frequency[1:] == freq[-1]) and np.all(m.ridge_period[1:] == 1 / freq[-1])
    assert np.array_equal(m.ridge_wwz, np.arange(7.0)) and np.array_equal(m.ridge_amplitude, np.arange(7.0) / 2)
    assert m.best == (c["tau"][6], freq[-1], 6.0, 3.0)
    assert (m.best.tau, m.best.frequency, m.best.wwz, m.best.amplitude) == m.best and m.visited == 7
    given = [30.0, 10.0, 10.0]   # an array: taken as it is, any order, duplicates kept
    m = w(s, taus=given, want_planes=False)
    assert np.array_equal(calls[-1]["tau"], given) and calls[-1]["dy"] is None and calls[-1]["want_planes"] is False
    assert m.wwz is None and m.amplitude is None and m.neff is None and m.ridge_bin.size == 3
    m = w(s, taus=np.int64(1))
    assert np.array_equal(m.tau, [t[0]])


def test_map_without_an_eligible_cell():
    out = dict(wwz=None, amp=None, neff=None, ridge_bin=np.array([-1, -1]), ridge_wwz=np.full(2, np.nan),
               ridge_amp=np.full(2, np.nan), best=(np.nan, -1, -1), visited=0)
    m = WWZMap(np.array([0.1, 0.2]), np.array([0.0, 1.0]), out)
    assert all(np.isnan(v) for v in m.best) and np.all(np.isnan(m.ridge_frequency)) and np.all(np.isnan(m.ridge_period))


def test_size_functions_and_loud_failure_without_a_device():
    for name in ("pdc_wwz_scan", "pdc_wwz_scan_dev", "pdc_wwz_tile_bins", "pdc_wwz_work_bytes", "pdc_wwz_last_dispatch"):
        assert name in _cabi.PROTOTYPES and hasattr(_cabi.lib(), name)
    tile = _cabi.wwz_tile_bins()
    assert tile >= 256 and tile % 256 == 0
    small = _cabi.wwz_work_bytes(1000, tile, 4)
    assert small >= 1002 * 48
    assert _cabi.wwz_work_bytes(1000, tile + 1, 4) > small            # one more tile: more (tau, tile) cells
    assert _cabi.wwz_work_bytes(1000, tile, 400) > small
    assert _cabi.wwz_work_bytes(2000, tile, 4) >= small + 1000 * 48   # the records
    for bad in ((3, 10, 1), (100, 0, 1), (100, 10, 0), (-1, 10, 1), (100, 1 << 40, 1 << 40)):
        assert _cabi.wwz_work_bytes(*bad) == -1
    t, y, err, freq, tau = wo.chirp_curve()
    f0, delta, nf = _cabi.grid_params(freq)
    # arguments the library refuses before it looks for a device
    good = dict(t=t, y=y, dy=err, f0=f0, delta=delta, nf=nf, tau=tau, decay=wo.FOSTER)
    for kw in (dict(f0=-0.1), dict(f0=np.nan), dict(delta=0.0), dict(delta=np.inf), dict(nf=0), dict(t=t[:3], y=y[:3], dy=None),
               dict(tau=np.array([])), dict(decay=0.0), dict(decay=-1.0), dict(decay=np.nan), dict(min_neff=np.nan),
               dict(t=t[::-1].copy()), dict(t=np.where(np.arange(t.size) == 5, np.nan, t)),
               dict(tau=np.array([1.0, np.nan])), dict(tau=np.array([np.inf]))):
        with pytest.raises(ValueError):
            _cabi.wwz_scan(**{**good, **kw})
    with pytest.raises(ValueError):
        _cabi.wwz_scan(**{**good, "y": y[:-1]})
    if _cabi.device_count() == 0:
        with pytest.raises((RuntimeError, ValueError)):      # no GPU: fails loudly, never a CPU answer
            _cabi.wwz_scan(**good)
        with pytest.raises((RuntimeError, ValueError)):
            WWZ(0.05, 0.45)(TSeries(t, y), err, taus=5)
