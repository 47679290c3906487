"""MultiHarmonicGLS without a GPU: the test-local oracle (tests/mhgls_oracle.py) against the project's exact GLS
oracle and against itself in 80-bit arithmetic, the host class, the C ABI.  The reference has no such class -
PARITY UNPINNED BY THE REFERENCE."""
import inspect

import numpy as np
import pytest

import mhgls_oracle as mo
from oracle import scan_oracle as so
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.spectral import GLS, MultiHarmonicGLS

CURVES = [(12, 2), (31, 3), (64, 4), (65, 5), (200, 6), (1000, 7)]


def test_oracle_with_one_term_is_the_exact_gls_power(golden_dir):
    g = np.load(f"{golden_dir}/g2_sine100.npz")
    t = np.arange(100.0)
    freq, exact = so.gls(t, g["values"], sums="exact")
    assert np.array_equal(freq, g["frequency"])
    keep = mo.cond(t, g["values"], None, freq, 1) <= mo.COND_LIMIT
    assert keep.mean() >= 0.95
    got = mo.power(t, g["values"], None, freq, 1)
    assert np.max(np.abs(got[keep] - exact[keep])) <= 1e-12
    assert int(np.nanargmax(np.where(keep, got, np.nan))) == int(g["argmax"])


@pytest.mark.parametrize("n,seed", CURVES[:5])
def test_float64_and_longdouble_oracles_agree_on_kept_bins(n, seed):
    t, y, err = mo.curve(n, seed)
    freq = GLS()._grid(TSeries(t, y))
    for nterms in (1, 2, 3, 4)[:2 if n == 12 else 4]:
        for fit_mean in (True, False):
            for e in (err, None):
                keep = mo.cond(t, y, e, freq, nterms, fit_mean) <= mo.COND_LIMIT
                assert 1 - keep.mean() <= 0.05, (nterms, fit_mean, 1 - keep.mean())
                p64 = mo.power(t, y, e, freq, nterms, fit_mean, dtype=np.float64)
                p80 = mo.power(t, y, e, freq, nterms, fit_mean, dtype=np.longdouble)
                assert np.max(np.abs(p64[keep] - p80[keep])) <= 1e-11
                assert np.all((p80[keep] >= 0) & (p80[keep] <= 1 + 1e-12))   # a share of the weighted variance


def test_oracle_psd_normalisation():
    t, y, err = mo.curve(64, 4)
    freq = GLS()._grid(TSeries(t, y))[5:40]
    w = err ** -2.0 / np.sum(err ** -2.0)
    yy = np.dot(w, (y - np.dot(w, y)) ** 2)
    a, b = mo.power(t, y, err, freq, 3), mo.power(t, y, err, freq, 3, psd=True)
    assert np.allclose(np.asarray(b / a, dtype=float), 0.5 * np.sum(err ** -2.0) * yy, rtol=1e-12)


def test_class_signature_and_validation():
    assert issubclass(MultiHarmonicGLS, GLS)
    sig = inspect.signature(MultiHarmonicGLS.__init__)
    assert list(sig.parameters)[:5] == ["self", "fmin", "fmax", "n", "psd"]
    assert list(inspect.signature(GLS.__init__).parameters)[:5] == ["self", "fmin", "fmax", "n", "psd"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("nterms", "device"))
    assert sig.parameters["nterms"].default == 2
    for bad in (0, 5, -1, 2.5):
        with pytest.raises(ValueError):
            MultiHarmonicGLS(nterms=bad)
    m = MultiHarmonicGLS(0.01, 0.4, 3, True, nterms=4, device=0)
    assert (m.fmin, m.fmax, m.n, m.psd, m.nterms, m.device) == (0.01, 0.4, 3, True, 4, 0)
    for call in (lambda: m.bootstrap(10), lambda: m.fap(0.5), lambda: m.fal(0.01), lambda: m.batch([np.ones(20)])):
        with pytest.raises(NotImplementedError):
            call()
    t, y, _ = mo.curve(31, 3)
    assert np.array_equal(m._grid(TSeries(t, y)), GLS(0.01, 0.4, 3)._grid(TSeries(t, y)))   # GLS's grid, unchanged


@pytest.mark.parametrize("fit_mean", [True, False])
def test_model_is_the_weighted_least_squares_fit(fit_mean):
    """``model`` needs only the attributes a call leaves behind: set them by hand, compare with lstsq on the same
    design built around another time origin (the fit does not depend on it)."""
    t, y, err = mo.curve(200, 6)
    m = MultiHarmonicGLS(nterms=3)
    m.signal, m.err, m.fit_mean = TSeries(t, y), err, fit_mean
    tf = np.linspace(t[0], t[-1], 57)

    def design(times):
        arg = 2 * np.pi * times / 6.3
        cols = [np.ones_like(arg)] if fit_mean else []
        for h in (1, 2, 3):
            cols += [np.sin(h * arg), np.cos(h * arg)]
        return np.stack(cols, axis=1)

    coef = np.linalg.lstsq(design(t) / err[:, None], y / err, rcond=None)[0]
    got = m.model(tf, 1 / 6.3)
    assert isinstance(got, TSeries)
    assert np.max(np.abs(got.values - design(tf) @ coef)) <= 1e-9


def test_cabi_symbols_and_loud_failure_without_a_device():
    assert "pdc_mhgls_scan" in _cabi.PROTOTYPES and "pdc_mhgls_scan_dev" in _cabi.PROTOTYPES
    lib = _cabi.lib()
    assert hasattr(lib, "pdc_mhgls_scan") and hasattr(lib, "pdc_mhgls_scan_dev")
    t, y, err = mo.curve(31, 3)
    # arguments the library refuses before it looks for a device
    for kw in (dict(nterms=0), dict(nterms=5), dict(delta=0.0), dict(delta=float("nan")), dict(delta=-0.1), dict(n=8, nterms=4)):
        n = kw.pop("n", 31)
        args = dict(f0=0.01, delta=0.01, nf=50, nterms=2)
        args.update(kw)
        with pytest.raises(ValueError):
            _cabi.mhgls_scan(t[:n], y[:n], err[:n], **args)
    with pytest.raises(ValueError):
        _cabi.mhgls_scan(t, y[:-1], None, 0.01, 0.01, 50)
    if _cabi.device_count() == 0:
        with pytest.raises((RuntimeError, ValueError)):      # no GPU: the class fails loudly, never a CPU answer
            MultiHarmonicGLS()(TSeries(t, y), err)
        with pytest.raises((RuntimeError, ValueError)):
            _cabi.mhgls_scan(t, y, err, 0.01, 0.01, 50)
