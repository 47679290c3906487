"""MultiHarmonicGLS on the GPU (csrc/mhgls.hip through the class and the C ABI) against the test-local oracle
(tests/mhgls_oracle.py: direct cos / sin per pair, Cholesky in float64, itself held to the 80-bit evaluation at 1e-11
by tests/test_mhgls_host.py).  The reference has no such class - PARITY UNPINNED BY THE REFERENCE.

M is nearly singular at the lowest few frequencies, where the harmonics are almost constant over the baseline: only
bins whose condition number - computed by the oracle, never by the device - is at most 1e6 are compared in value, a
test fails when more than 5 % of its bins are left out, and a left-out bin must still be NaN or finite."""
import functools

import numpy as np
import pytest

import mhgls_oracle as mo
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.spectral import GLS, MultiHarmonicGLS

pytestmark = pytest.mark.gpu

SEEDS = {12: 2, 31: 3, 64: 4, 65: 5, 200: 6, 1000: 7}   # 64 / 65 straddle the 64-sample chunk of the rotation tables


def max_terms(n):
    return 2 if n == 12 else 4


@functools.lru_cache(maxsize=None)
def curve(n):
    return mo.curve(n, SEEDS[n])


@functools.lru_cache(maxsize=None)
def normal_equations(n, with_err, fit_mean, nf=None):
    """The oracle's normal equations of the LARGEST model of curve ``n``, evaluated once: the design of a smaller
    ``nterms`` is a leading block of the same columns."""
    t, y, err = curve(n)
    return mo.normal_equations(t, y, err if with_err else None, grid(n, nf), max_terms(n), fit_mean)


def grid(n, nf=None):
    t, y, _ = curve(n)
    if nf is None:
        return GLS()._grid(TSeries(t, y))
    freq = gls_with_bins(n, nf)._grid(TSeries(t, y))
    assert freq.size == nf
    return freq


def gls_with_bins(n, nf, cls=GLS, **kw):
    """An explicit ``fmax`` that gives ``nf`` bins on curve ``n``."""
    t, _, _ = curve(n)
    df = 1.0 / (t[-1] - t[0]) / 5
    return cls(fmax=0.5 * df + (nf - 1.5) * df, **kw)


def oracle(n, nterms, with_err, fit_mean, psd=False, nf=None):
    """(exact power, kept bins) of one case."""
    M, b, YY, W = normal_equations(n, with_err, fit_mean, nf)
    d = 2 * nterms + (1 if fit_mean else 0)
    M, b = M[:, :d, :d], b[:, :d]
    keep = mo.cond_from(M) <= mo.COND_LIMIT
    assert 1 - keep.mean() <= 0.05, f"{100 * (1 - keep.mean()):.1f} % of the bins left out"
    return mo.power_from(M, b, YY, W, psd), keep


def assert_meets_oracle(label, got, exact, keep):
    err = np.abs(got[keep] - exact[keep])
    gate = 1e-6 * np.abs(exact[keep]) + 1e-9   # Tier E: <= 1e-6 relative in fp64
    print(f"{label}: bins {got.size} kept {int(keep.sum())} max |err| {err.max():.3e} max err/gate {np.max(err / gate):.3e}")
    assert np.all(err <= gate), (label, float(np.max(err / gate)))
    assert int(np.argmax(np.where(keep, got, -np.inf))) == int(np.argmax(np.where(keep, exact, -np.inf))), label
    assert not np.any(np.isinf(got[~keep])), label   # left-out bins: NaN or finite


CASES = [(n, h, fm, we) for n in SEEDS for h in range(1, max_terms(n) + 1) for fm in (True, False) for we in (True, False)]


@pytest.mark.parametrize("n,nterms,fit_mean,with_err", CASES)
def test_parity_with_the_oracle(n, nterms, fit_mean, with_err):
    t, y, err = curve(n)
    e = err if with_err else None
    for psd in ((False, True) if n == 64 else (False,)):
        m = MultiHarmonicGLS(psd=psd, nterms=nterms)
        p = m(TSeries(t, y), e, fit_mean)
        assert isinstance(p, FSeries) and np.array_equal(p.frequency, grid(n)) and m.periodogram is p
        assert m.signal.size == n and (m.err is e if with_err else np.all(m.err == 1.0))
        exact, keep = oracle(n, nterms, with_err, fit_mean, psd)
        assert_meets_oracle(f"parity N={n} nterms={nterms} fit_mean={int(fit_mean)} err={int(with_err)} psd={int(psd)}",
                            p.values, exact, keep)


@pytest.mark.parametrize("n", [65, 200, 1000])
def test_one_term_is_gls(n):
    t, y, err = curve(n)
    for fit_mean in (True, False):
        got = MultiHarmonicGLS(nterms=1)(TSeries(t, y), err, fit_mean)
        want = GLS()(TSeries(t, y), err, fit_mean)
        _, keep = oracle(n, 1, True, fit_mean)
        np.testing.assert_allclose(got.values[keep], want.values[keep], rtol=1e-9, atol=0)
        assert int(np.nanargmax(got.values)) == int(np.nanargmax(want.values))


@pytest.mark.parametrize("nf", [1023, 1024, 1025])
def test_tile_seams(nf):
    """A tile is 1024 frequencies: grids one short of it, exact, and one over, every kept bin."""
    t, y, err = curve(200)
    for nterms in (1, 2, 3, 4):
        p = gls_with_bins(200, nf, MultiHarmonicGLS, nterms=nterms)(TSeries(t, y), err)
        assert p.size == nf
        exact, keep = oracle(200, nterms, True, True, nf=nf)
        assert_meets_oracle(f"seam nf={nf} nterms={nterms}", p.values, exact, keep)


@pytest.mark.parametrize("nterms", [1, 2, 3, 4])
def test_slab_of_the_grid_reproduces_the_full_call(nterms):
    t, y, err = curve(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    full = _cabi.mhgls_scan(t, y, err, f0, delta, nf, nterms)
    part = _cabi.mhgls_scan(t, y, err, f0, delta, 257, nterms, j_begin=nf // 3)
    assert nf // 3 + 257 <= nf
    np.testing.assert_allclose(part, full[nf // 3:nf // 3 + 257], rtol=1e-9, atol=0)   # another tile phase: to rounding


def eclipse(n=300, period=7.3):
    rng = np.random.default_rng(11)
    t = np.sort(rng.uniform(0, 3.0 * n, n))
    err = np.full(n, 0.1)
    y = 10.0 - 1.0 * ((t / period) % 1.0 < 0.08) + err * rng.standard_normal(n)
    return t, y, err


def test_finds_the_period_of_an_eclipse_and_models_it():
    """A box dip of depth 1 over 8 % of the phase: its power is spread over many harmonics, four of them in one fit
    put the highest peak at the period."""
    t, y, err = eclipse()
    m = MultiHarmonicGLS(nterms=4)
    p = m(TSeries(t, y), err)
    print(f"eclipse: MultiHarmonicGLS(nterms=4) peak at {p.period_at_highest_peak:.4f}, GLS peak at "
          f"{GLS()(TSeries(t, y), err).period_at_highest_peak:.4f} (period 7.3)")
    assert abs(p.period_at_highest_peak - 7.3) <= 0.01 * 7.3
    tf = np.linspace(t[0], t[0] + 14.6, 101)
    arg = lambda times, h: 2 * np.pi * h * np.asarray(times) / 7.3
    design = lambda times: np.stack([np.ones_like(times)] + [f(arg(times, h)) for h in (1, 2, 3, 4) for f in (np.cos, np.sin)], axis=1)
    coef = np.linalg.lstsq(design(t) / err[:, None], y / err, rcond=None)[0]
    assert np.max(np.abs(m.model(tf, 1 / 7.3).values - design(tf) @ coef)) <= 1e-9


def test_class_conveniences():
    t, y, err = curve(65)
    m = MultiHarmonicGLS(nterms=2)
    raw = m(y)                                              # raw arrays are wrapped as GLS wraps them
    assert raw.size == m._grid(TSeries(values=y)).size and np.all(m.err == 1.0)
    m(TSeries(t, y), err)
    win = m.window()                                        # inherited: an all-ones signal, no floating mean
    assert isinstance(win, FSeries) and win.size == m.frequency.size
    with pytest.raises(ValueError):
        m(TSeries(t, y), err[:-1])
    with pytest.raises(ValueError):
        MultiHarmonicGLS(nterms=4)(TSeries(t[:9], y[:9]))   # nine columns need ten samples
    bad = y.copy()
    bad[7] = np.nan                                         # NaN in the data propagates, it is not an error
    assert np.all(np.isnan(m(TSeries(t, bad), err).values))


def test_hygiene_no_allocation_on_a_repeated_or_rejected_call():
    t, y, err = curve(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    first = _cabi.mhgls_scan(t, y, err, f0, delta, nf, 3)
    counts = _cabi.alloc_counts()
    again = _cabi.mhgls_scan(t, y, err, f0, delta, nf, 3)
    assert _cabi.alloc_counts() == counts and np.array_equal(first, again)
    with pytest.raises(ValueError):
        _cabi.mhgls_scan(t[:8], y[:8], err[:8], f0, delta, nf, 4)
    assert _cabi.alloc_counts() == counts
