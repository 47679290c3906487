"""The Keplerian periodogram without a GPU: the test-local oracle (tests/kepler_oracle.py) against itself in float64 and
against the closed-form GLS power, the share of cells the keep rule leaves out on every parity input of
tests/test_kepler_gpu.py, the recovery of the injected orbit, the host class and its argument rules, the size functions
of the C ABI.  The reference has no such statistic - PARITY UNPINNED BY THE REFERENCE."""
import functools
import inspect

import numpy as np
import pytest

import kepler_oracle as ko
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.spectral import GLS, KeplerianGLS


@functools.lru_cache(maxsize=None)
def curve_and_anomalies(n, offset=0.0):
    curve = ko.kepler_curve(n, offset)
    t, _, _, freq, ecc, m0 = curve
    return curve, ko.anomalies(t, freq, ecc, m0)


def test_float64_and_longdouble_oracles_agree_far_inside_the_gate():
    for n in (24, 40):
        (t, y, err, freq, ecc, m0), nu = curve_and_anomalies(n)
        exact, cond = ko.cube(t, y, err, freq, ecc, m0, nu=nu)
        double, _ = ko.cube(t, y, err, freq, ecc, m0, dtype=np.float64)
        worst, left_out = ko.compare(double, exact, cond)
        print(f"n={n}: float64 / gate = {worst:.2e}, largest cond {cond.max():.2e}, left out {left_out:.4f}")
        assert worst <= 1e-3 and left_out == 0.0


@pytest.mark.parametrize("n", [24, 40, 63, 64, 65, 129])
def test_left_out_share_of_every_parity_input(n):
    """All four weighted / fit_mean combinations of every curve the GPU file scans, and the Julian-date offset."""
    cases = [(n, 0.0)] + ([(40, 2450000.0)] if n == 40 else [])
    for n_, offset in cases:
        (t, y, err, freq, ecc, m0), nu = curve_and_anomalies(n_, offset)
        for e in (None, err):
            for fit_mean in (True, False):
                _, cond = ko.cube(t, y, e, freq, ecc, m0, fit_mean, nu=nu)
                left_out = float(np.mean(cond > ko.COND_LIMIT))
                print(f"n={n_} offset={offset:g} weighted={e is not None} fit_mean={fit_mean}: largest cond "
                      f"{cond.max():.2e}, left out {left_out:.4f}")
                assert left_out <= ko.LEFT_OUT_CAP


def test_left_out_share_of_the_small_parity_inputs():
    """The many-cycles curve and the seam inputs (24 samples): the cell counts around a cell group of up to 8."""
    t, y, err, freq, ecc, m0 = ko.many_cycles_curve()
    assert freq[-1] * (t[-1] - t[0]) > 9e4
    cases = {"1e5 cycles": (t, y, err, freq, ecc, m0), "no trace": ko.no_trace_case(), "slabs": ko.slab_case()}
    cases.update({f"nf={nf}": ko.tile_seam_case(nf) for nf in (255, 256, 257)})
    cases.update({f"{count} cells": ko.cell_seam_case(count) for count in (1, 2, 3, 4, 5, 7, 8, 9, 17)})
    for label, (t, y, err, freq, ecc, m0) in cases.items():
        _, cond = ko.cube(t, y, err, freq, ecc, m0)
        left_out = float(np.mean(cond > ko.COND_LIMIT))
        print(f"{label}: largest cond {cond.max():.2e}, left out {left_out:.4f}")
        assert left_out <= ko.LEFT_OUT_CAP


def test_circular_row_is_the_gls_power():
    for n in (24, 40):
        (t, y, err, freq, ecc, m0), nu = curve_and_anomalies(n)
        for e in (None, err):
            for fit_mean in (True, False):
                exact, _ = ko.cube(t, y, e, freq, ecc, m0, fit_mean, nu=nu)
                gls = ko.gls_power(t, y, e, freq, fit_mean)
                assert ecc[0] == 0.0
                assert np.max(np.abs(exact[:, 0, :] - gls[:, None])) <= 1e-15


def test_oracle_recovers_the_injected_orbit():
    for n, kepler_peak, gls_peak in ((40, 0.969, 0.685), (65, 0.973, 0.715)):
        (t, y, err, freq, ecc, m0), nu = curve_and_anomalies(n)
        exact, _ = ko.cube(t, y, err, freq, ecc, m0, nu=nu)
        power, cell, best = ko.reductions(exact.astype(np.float64))
        assert best[1] == ko.BEST_BIN and ecc[best[2] // m0.size] == pytest.approx(ko.BEST_ECC)
        assert abs(freq[best[1]] - 1 / ko.PERIOD) <= 0.0005
        assert best[0] == pytest.approx(kepler_peak, abs=5e-4)
        assert float(ko.gls_power(t, y, err, freq).max()) == pytest.approx(gls_peak, abs=5e-4)
        orbit = ko.fit(t, y, err, freq[best[1]], ecc[best[2] // m0.size], m0[best[2] % m0.size])
        assert abs(orbit["K"] - ko.SEMI_AMPLITUDE) <= 5 and abs(orbit["gamma"] - 100) <= 3


def test_reductions_follow_nanargmax():
    cells = np.array([[[1.0, 5.0], [5.0, np.nan]], [[np.nan, np.nan], [np.nan, np.nan]], [[9.0, 2.0], [9.0, 1.0]]])
    power, cell, best = ko.reductions(cells)
    assert cell.tolist() == [1, -1, 0] and cell.dtype == np.int32
    assert power[0] == 5.0 and np.isnan(power[1]) and best == (9.0, 2, 0)
    assert ko.reductions(np.full((2, 1, 3), np.nan))[2][1:] == (-1, -1)


def test_class_signature_and_validation(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("reached the library")

    monkeypatch.setattr(_cabi, "kepler_scan", no_device)
    monkeypatch.setattr(_cabi, "lib", no_device)
    sig = inspect.signature(KeplerianGLS.__init__)
    assert list(sig.parameters)[:5] == ["self", "fmin", "fmax", "n", "psd"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("ecc", "n_phase", "device"))
    assert sig.parameters["ecc"].default == 10 and sig.parameters["n_phase"].default == 32
    call = inspect.signature(KeplerianGLS.__call__)
    assert list(call.parameters) == ["self", "signal", "err", "fit_mean", "want_cube"]
    assert call.parameters["fit_mean"].default is True and call.parameters["want_cube"].default is False
    k = KeplerianGLS(0.02, 0.1, 3, ecc=4, n_phase=8, device=1)
    assert np.array_equal(k.ecc, np.linspace(0, 0.9, 4)) and np.array_equal(k.m0, np.arange(8) / 8)
    assert (k.fmin, k.fmax, k.n, k.psd, k.device) == (0.02, 0.1, 3, False, 1)
    k = KeplerianGLS(ecc=[0.95, 0.0, 0.3], n_phase=[0.5, 0.0])   # arrays are taken as they are, any order
    assert k.ecc.tolist() == [0.95, 0.0, 0.3] and k.m0.tolist() == [0.5, 0.0]
    assert KeplerianGLS(ecc=1, n_phase=1).ecc.tolist() == [0.0]
    for bad in (dict(ecc=0), dict(ecc=-1), dict(ecc=[0.96]), dict(ecc=[-0.1]), dict(ecc=[np.nan]), dict(ecc=[]),
                dict(ecc=[[0.1]]), dict(ecc=True), dict(ecc=2.5), dict(n_phase=0), dict(n_phase=[1.0]),
                dict(n_phase=[-0.1]), dict(n_phase=[np.nan]), dict(n_phase=[np.inf]), dict(n_phase=[]),
                dict(ecc=256, n_phase=256)):
        with pytest.raises(ValueError):
            KeplerianGLS(**bad)
    t, y, _, _, _, _ = ko.kepler_curve(24)
    s = TSeries(t, y)
    assert np.array_equal(KeplerianGLS(0.02, 0.1, 3)._grid(s), GLS(0.02, 0.1, 3)._grid(s))   # GLS's grid, unchanged
    for name in ("bootstrap", "fap", "fal", "batch"):
        with pytest.raises(NotImplementedError):
            getattr(KeplerianGLS(), name)()


def _fake_scan(calls):
    def scan(t, y, dy, f0, delta, nf, ecc, m0, fit_mean=True, psd=False, want_cube=False, want_bins=True, device=None):
        calls.append(dict(t=t, y=y, dy=dy, f0=f0, delta=delta, nf=nf, ecc=ecc, m0=m0, fit_mean=fit_mean, psd=psd,
                          want_cube=want_cube, device=device))
        cell = np.full(nf, 1 * m0.size + 2, dtype=np.int32)
        cell[0] = -1
        power = np.linspace(0.1, 0.5, nf)
        power[0] = np.nan
        return dict(power=power, cell=cell, cube=np.zeros((nf, ecc.size, m0.size)) if want_cube else None,
                    best=(0.5, nf - 1, int(cell[-1])))
    return scan


def test_class_fields_and_orbit(monkeypatch):
    """The class hands the library GLS's grid and its lists, and turns cells into eccentricities and phases; orbit() and
    model() refit on the host at the chosen bin's cell and reproduce a noiseless orbit."""
    calls = []
    monkeypatch.setattr(_cabi, "kepler_scan", _fake_scan(calls))
    t = np.sort(np.random.default_rng(3).uniform(0, 200, 50))
    freq = GLS(0.05, 0.058, 5)._grid(TSeries(t, t))
    f, e, m0, K, omega, gamma = freq[-1], 0.3, 0.25, 12.0, 2.2, -40.0   # the last bin; e and m0 are cell (1, 2) below
    y = ko.signal(t, period=1 / f, e=e, omega=omega, K=K, t_peri=t[0] + m0 / f) + gamma
    k = KeplerianGLS(0.05, 0.058, 5, ecc=[0.0, 0.3, 0.6], n_phase=8, device=2)
    p = k(TSeries(t, y), err=np.full(50, 2.0), want_cube=True)
    c = calls[-1]
    assert np.array_equal(p.frequency, freq) and np.array_equal(c["f0"] + np.arange(c["nf"]) * c["delta"], freq)
    assert (c["fit_mean"], c["psd"], c["want_cube"], c["device"]) == (True, False, True, 2)
    assert k.cube.shape == (freq.size, 3, 8) and np.array_equal(k.cell, np.r_[-1, np.full(freq.size - 1, 10)])
    assert np.isnan(k.eccentricity[0]) and np.isnan(k.periastron_phase[0]) and np.isnan(p.values[0])
    assert np.all(k.eccentricity[1:] == 0.3) and np.all(k.periastron_phase[1:] == 0.25)
    assert k.best == (freq[-1], 0.3, 0.25, 0.5) and k.best.e == 0.3 and k.best.m0 == 0.25
    orbit = k.orbit()
    assert set(orbit) == {"period", "K", "e", "omega", "gamma", "t_peri"}
    assert orbit["period"] == pytest.approx(1 / f) and orbit["e"] == 0.3 and orbit["t_peri"] == pytest.approx(t[0] + m0 / f)
    assert orbit["K"] == pytest.approx(K, rel=1e-9) and orbit["omega"] == pytest.approx(omega, rel=1e-9)
    assert orbit["gamma"] == pytest.approx(gamma, rel=1e-9)
    assert k.orbit(f0=f) == orbit
    tf = np.linspace(0, 200, 17)
    model = k.model(tf)
    assert np.max(np.abs(model.values - (ko.signal(tf, period=1 / f, e=e, omega=omega, K=K, t_peri=t[0] + m0 / f) + gamma))) <= 1e-8
    with pytest.raises(ValueError):
        k.orbit(f0=freq[0])   # that bin has no cell
    k(TSeries(t, y))
    assert k.cube is None and calls[-1]["dy"] is None and calls[-1]["want_cube"] is False


def test_size_functions_and_loud_failure_without_a_device(monkeypatch):
    for name in ("pdc_kepler_scan", "pdc_kepler_scan_dev", "pdc_kepler_anomaly", "pdc_kepler_cell_group",
                 "pdc_kepler_tile_bins", "pdc_kepler_work_bytes", "pdc_kepler_last_dispatch"):
        assert name in _cabi.PROTOTYPES and hasattr(_cabi.lib(), name)
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    kc = _cabi.kepler_cell_group()
    assert 1 <= kc <= 64 and _cabi.kepler_tile_bins() == 256
    small = _cabi.kepler_work_bytes(1000, 256, 2, kc)
    assert small >= 1000 * 24
    assert _cabi.kepler_work_bytes(1000, 257, 2, kc) > small             # one more tile
    assert _cabi.kepler_work_bytes(1000, 256, 2, kc + 1) > small         # one more cell group
    assert _cabi.kepler_work_bytes(2000, 256, 2, kc) >= small + 1000 * 24   # the records
    for bad in ((3, 10, 1, 1), (100, 0, 1, 1), (100, 10, 0, 1), (100, 10, 1, 0), (-1, 10, 1, 1), (100, 10, 256, 256),
                (100, 10, 65536, 1), (100, 1 << 45, 1, 1)):
        assert _cabi.kepler_work_bytes(*bad) == -1
    assert _cabi.kepler_work_bytes(100, 10, 255, 257) > 0                 # 65535 cells are in range
    assert _cabi.kepler_work_bytes(100, 1 << 36, 1024, 32, want_cube=True) == -1   # the cube out of range
    # a budget cuts the grid into slabs of whole tiles: a smaller budget, a smaller workspace, never under one tile
    big = (1000, 1_000_000, 20, 32)
    free = _cabi.kepler_work_bytes(*big)
    assert free > 1 << 30
    sizes = {}
    for gb in ("1", "0.25", "0.0001"):
        monkeypatch.setenv("PDC_WORK_BUDGET_GB", gb)
        sizes[gb] = _cabi.kepler_work_bytes(*big)
    assert sizes["0.0001"] < sizes["0.25"] < sizes["1"] < free
    assert sizes["1"] <= 1 << 30 and sizes["0.25"] <= 1 << 28
    assert sizes["0.0001"] >= 1000 * 24 + 256 * 12 * (640 // kc)         # one tile's rows stay
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "1")
    assert _cabi.kepler_work_bytes(1000, 256, 2, kc) == small             # a scan that fits is not touched
    monkeypatch.delenv("PDC_WORK_BUDGET_GB")
    assert _cabi.kepler_work_bytes(*big) == free
    assert _cabi.kepler_last_dispatch()[1:] == (0, 0) or _cabi.device_count() > 0   # zeros before the first scan

    t, y, err, freq, ecc, m0 = ko.kepler_curve(24)
    f0, delta, nf = _cabi.grid_params(freq)
    # arguments the library refuses before it looks for a device
    good = dict(t=t, y=y, dy=err, f0=f0, delta=delta, nf=nf, ecc=ecc, m0=m0)
    for kw in (dict(f0=-0.1), dict(f0=np.nan), dict(delta=0.0), dict(delta=np.inf), dict(nf=0),
               dict(t=t[:3], y=y[:3], dy=None), dict(ecc=np.array([])), dict(m0=np.array([])), dict(ecc=np.array([0.96])),
               dict(ecc=np.array([-1e-9])), dict(ecc=np.array([0.1, np.nan])), dict(m0=np.array([1.0])),
               dict(m0=np.array([-0.25])), dict(m0=np.array([np.nan])), dict(ecc=np.zeros(256), m0=np.zeros(256)),
               dict(t=np.where(np.arange(t.size) == 5, np.nan, t))):
        with pytest.raises(ValueError):
            _cabi.kepler_scan(**{**good, **kw})
    with pytest.raises(ValueError):
        _cabi.kepler_scan(**{**good, "y": y[:-1]})
    with pytest.raises(ValueError, match="every output is NULL"):
        _cabi.check(_cabi.lib().pdc_kepler_scan(_cabi._ptr(t), _cabi._ptr(y), _cabi._ptr(err), t.size, f0, delta, nf,
                                                _cabi._ptr(ecc), ecc.size, _cabi._ptr(m0), m0.size, 1, 0, None, None, None,
                                                None, None, 0))
    for phase, e in (([0.1], [0.96]), ([0.1], [-0.1]), ([np.nan], [0.1]), ([np.inf], [0.1]), ([0.1], [np.nan])):
        with pytest.raises(ValueError):
            _cabi.kepler_anomaly(phase, e)
    with pytest.raises(ValueError):
        _cabi.kepler_anomaly([0.1, 0.2], [0.1])
    assert _cabi.kepler_anomaly([], [])[0].size == 0   # nothing to do: no device is looked for
    if _cabi.device_count() == 0:
        with pytest.raises((RuntimeError, ValueError)):      # no GPU: fails loudly, never a CPU answer
            _cabi.kepler_scan(**good)
        with pytest.raises((RuntimeError, ValueError)):
            KeplerianGLS(0.02, 0.1)(TSeries(t, y), err)
