"""MultibandGLS on the GPU (csrc/mbgls.hip through the class and the C ABI) against the test-local oracle
(tests/mbgls_oracle.py: the full (B + 2H) design with direct cos / sin per pair, Cholesky in float64, itself held to the
80-bit evaluation at 1e-11 by tests/test_mbgls_host.py).  The reference has no such class - PARITY UNPINNED BY THE
REFERENCE.

M is nearly singular at the lowest few frequencies, where the harmonics are almost constant over the baseline: only
bins whose condition number - computed by the oracle on the full M, never by the device - is at most 1e6 are compared in
value (Tier E: |delta| <= 1e-6 |exact| + 1e-9, plus the argmax over those bins), a test fails when more than 5 % of its
bins are left out, and a left-out bin must still be NaN or finite."""
import functools

import numpy as np
import pytest

import mbgls_oracle as mb
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.spectral import GLS, MultibandGLS, MultiHarmonicGLS

pytestmark = pytest.mark.gpu

BANDS = (1, 2, 3, 6)


def shapes(n):
    """(bands, largest nterms) of curve ``n``: twelve samples carry at most 3 offsets and 2 harmonics."""
    return (BANDS[:3], 2) if n == 12 else (BANDS, 3)


@functools.lru_cache(maxsize=None)
def curve(n, B):
    return mb.curve(n, B)


def gls_with_bins(n, nf, cls=GLS, **kw):
    """An explicit ``fmax`` that gives ``nf`` bins on curve ``n``."""
    t = curve(n, 1)[0]
    df = 1.0 / (t[-1] - t[0]) / 5
    return cls(fmax=0.5 * df + (nf - 1.5) * df, **kw)


def grid(n, nf=None):
    t, y = curve(n, 1)[:2]
    if nf is None:
        return GLS()._grid(TSeries(t, y))
    freq = gls_with_bins(n, nf)._grid(TSeries(t, y))
    assert freq.size == nf
    return freq


@functools.lru_cache(maxsize=None)
def normal_equations(n, B, with_err, fit_mean, nf=None, labels=None):
    """The oracle's normal equations of the LARGEST model of a case, evaluated once: the design of a smaller ``nterms``
    is a leading block of the same columns.  ``labels``: a hand-made label array (as a tuple) in place of the curve's."""
    t, y, err, band = curve(n, B)
    if labels is not None:
        y, band = curve(n, 1)[1] + 0.5 * np.array(labels), np.array(labels)
    return mb.normal_equations(t, y, err if with_err else None, band, B, grid(n, nf), shapes(n)[1], fit_mean)


def oracle(n, B, nterms, with_err, fit_mean, psd=False, nf=None, labels=None):
    """(exact power, kept bins) of one case."""
    M, b, YY, W = normal_equations(n, B, with_err, fit_mean, nf, labels)
    d = mb.columns(B, nterms, fit_mean)
    M, b = M[:, :d, :d], b[:, :d]
    keep = mb.cond_from(M) <= mb.COND_LIMIT
    assert 1 - keep.mean() <= 0.05, f"{100 * (1 - keep.mean()):.1f} % of the bins left out"
    return mb.power_from(M, b, YY, W, psd), keep


def assert_meets_oracle(label, got, exact, keep):
    err = np.abs(got[keep] - exact[keep])
    gate = 1e-6 * np.abs(exact[keep]) + 1e-9   # Tier E: <= 1e-6 relative in fp64
    print(f"{label}: bins {got.size} kept {int(keep.sum())} max |err| {err.max():.3e} max err/gate {np.max(err / gate):.3e}")
    assert np.all(err <= gate), (label, float(np.max(err / gate)))
    assert int(np.argmax(np.where(keep, got, -np.inf))) == int(np.argmax(np.where(keep, exact, -np.inf))), label
    assert not np.any(np.isinf(got[~keep])), label   # left-out bins: NaN or finite


CASES = [(n, B, h) for n in mb.SEEDS for B in shapes(n)[0] for h in range(1, shapes(n)[1] + 1)]


@pytest.mark.parametrize("n,B,nterms", CASES)
def test_parity_with_the_oracle(n, B, nterms):
    t, y, err, band = curve(n, B)
    for fit_mean in (True, False):
        for with_err in (True, False):
            e = err if with_err else None
            for psd in ((False, True) if n == 64 else (False,)):
                m = MultibandGLS(psd=psd, nterms=nterms)
                p = m(TSeries(t, y), band, e, fit_mean)
                assert isinstance(p, FSeries) and np.array_equal(p.frequency, grid(n)) and m.periodogram is p
                assert m.signal.size == n and (m.err is e if with_err else np.all(m.err == 1.0))
                assert m.fit_mean is fit_mean and np.array_equal(m.bands, np.arange(B))
                assert m.band_index.dtype == np.int32 and np.array_equal(m.band_index, band)
                exact, keep = oracle(n, B, nterms, with_err, fit_mean, psd)
                assert_meets_oracle(f"parity N={n} B={B} nterms={nterms} fit_mean={int(fit_mean)} err={int(with_err)} "
                                    f"psd={int(psd)}", p.values, exact, keep)


def runs(*lengths):
    """Labels 0, 1, ... in contiguous runs of the given lengths."""
    return tuple(int(v) for v in np.repeat(np.arange(len(lengths)), lengths))


SEAMS = {
    "a band of one sample": runs(1, 199),
    "one sample in the middle": tuple(1 if i == 77 else 0 for i in range(200)),
    "bands of 63, 64, 65 and 8": runs(63, 64, 65, 8),
    "bands of 65, 64, 63 and 8": runs(65, 64, 63, 8),
    "a boundary mid-chunk": runs(100, 100),
    "interleaved input order": tuple(i % 3 for i in range(200)),
    "interleaved blocks": tuple((i // 7) % 4 for i in range(200)),
}


@pytest.mark.parametrize("name", list(SEAMS))
def test_band_segment_seams(name):
    """The chunk loop runs band by band over records grouped by band: stretches of 1, 63, 64 and 65 samples, a band
    that ends mid-chunk, and bands whose samples are interleaved in the input."""
    labels = SEAMS[name]
    B = max(labels) + 1
    t, _, err = curve(200, 1)[:3]
    y = curve(200, 1)[1] + 0.5 * np.array(labels)
    for nterms in (1, 2, 3):
        p = MultibandGLS(nterms=nterms)(TSeries(t, y), np.array(labels), err)
        exact, keep = oracle(200, B, nterms, True, True, labels=labels)
        assert_meets_oracle(f"band seam ({name}) nterms={nterms}", p.values, exact, keep)


@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_tile_seams(nterms):
    """Grids one short of a tile, exact, and one over, every kept bin."""
    tile = _cabi.mbgls_tile_bins(nterms)
    t, y, err, band = curve(200, 3)
    for nf in (tile - 1, tile, tile + 1):
        p = gls_with_bins(200, nf, MultibandGLS, nterms=nterms)(TSeries(t, y), band, err)
        assert p.size == nf
        exact, keep = oracle(200, 3, nterms, True, True, nf=nf)
        assert_meets_oracle(f"tile seam nf={nf} nterms={nterms}", p.values, exact, keep)


@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_slab_of_the_grid_reproduces_the_full_call(nterms):
    t, y, err, band = curve(200, 3)
    f0, delta, nf = _cabi.grid_params(grid(200))
    full = _cabi.mbgls_scan(t, y, err, band, 3, f0, delta, nf, nterms)
    part = _cabi.mbgls_scan(t, y, err, band, 3, f0, delta, 257, nterms, j_begin=nf // 3)
    assert nf // 3 + 257 <= nf
    np.testing.assert_allclose(part, full[nf // 3:nf // 3 + 257], rtol=1e-9, atol=0)   # another tile phase: to rounding


@pytest.mark.parametrize("n", [65, 200])
def test_identities(n):
    t, y, err, band = curve(n, 3)
    one = np.zeros(n, dtype=int)
    for nterms in (1, 2, 3):
        _, keep1 = oracle(n, 1, nterms, True, True)
        _, keep0 = oracle(n, 1, nterms, True, False)
        _, keep3 = oracle(n, 3, nterms, True, True)
        mh = MultiHarmonicGLS(nterms=nterms)
        m = MultibandGLS(nterms=nterms)
        # one band is the multi-harmonic periodogram
        y1 = curve(n, 1)[1]
        np.testing.assert_allclose(m(TSeries(t, y1), one, err).values[keep1], mh(TSeries(t, y1), err).values[keep1],
                                   rtol=1e-9, atol=0)
        # without fit_mean the labels do not enter
        want = mh(TSeries(t, y), err, fit_mean=False).values[keep0]
        np.testing.assert_allclose(m(TSeries(t, y), band, err, fit_mean=False).values[keep0], want, rtol=1e-9, atol=0)
        np.testing.assert_allclose(m(TSeries(t, y), one, err, fit_mean=False).values[keep0], want, rtol=1e-9, atol=0)
        # the bands relabelled, and a constant added to each
        base = m(TSeries(t, y), band, err).values[keep3]
        np.testing.assert_allclose(m(TSeries(t, y), np.array([2, 0, 1])[band], err).values[keep3], base, rtol=1e-9, atol=0)
        np.testing.assert_allclose(m(TSeries(t, y + np.array([3.0, -1.5, 40.0])[band]), band, err).values[keep3], base,
                                   rtol=1e-9, atol=0)
    _, keep = oracle(n, 1, 1, True, True)
    y1 = curve(n, 1)[1]
    np.testing.assert_allclose(MultibandGLS(nterms=1)(TSeries(t, y1), one, err).values[keep],
                               GLS()(TSeries(t, y1), err).values[keep], rtol=1e-9, atol=0)


def test_science_case_sparse_multiband_photometry():
    """Six bands of twelve epochs each: the device finds the period the oracle finds, the model is the least-squares fit,
    and the fitted offsets are the bands' 0.4 apart."""
    t, y, err, band = mb.sparse_fixture()
    m = MultibandGLS(fmin=0.5, fmax=3.0)
    p = m(TSeries(t, y), band, err)
    assert p.size == 4964
    exact = np.asarray(mb.power(t, y, err, band, 6, p.frequency, 1, dtype=np.float64))
    keep = mb.cond(t, y, err, band, 6, p.frequency, 1) <= mb.COND_LIMIT
    assert 1 - keep.mean() <= 0.05
    assert_meets_oracle("sparse fixture", p.values, exact, keep)
    assert int(np.nanargmax(p.values)) == int(np.nanargmax(exact))
    period = 1 / p.frequency[np.nanargmax(p.values)]
    print(f"sparse fixture: period {period:.6f}, power {np.nanmax(p.values):.4f}")
    assert abs(period - mb.SPARSE_PERIOD) <= 1e-3 * mb.SPARSE_PERIOD
    tf = np.linspace(t[0], t[0] + 2 * mb.SPARSE_PERIOD, 101)
    series = lambda times: np.stack([np.cos(2 * np.pi * np.asarray(times) / mb.SPARSE_PERIOD),
                                     np.sin(2 * np.pi * np.asarray(times) / mb.SPARSE_PERIOD)], axis=1)
    onehot = (band[:, None] == np.arange(6)[None, :]).astype(float)
    coef = np.linalg.lstsq(np.hstack([onehot, series(t)]) / err[:, None], y / err, rcond=None)[0]
    for b in range(6):
        assert np.max(np.abs(m.model(tf, b, 1 / mb.SPARSE_PERIOD).values - (coef[b] + series(tf) @ coef[6:]))) <= 1e-9
    offsets = m.band_offsets(1 / mb.SPARSE_PERIOD)
    assert list(offsets) == list(range(6))
    assert np.all(np.abs(np.diff([offsets[b] for b in range(6)]) - 0.4) <= 0.1)


def test_class_conveniences():
    t, y, err, band = curve(65, 3)
    m = MultibandGLS(nterms=2)
    names = np.array(["g", "r", "i"])[band]                  # string labels: mapped through np.unique (g, i, r)
    p = m(TSeries(t, y), names, err)
    assert list(m.bands) == ["g", "i", "r"] and np.array_equal(m.band_index, np.array([0, 2, 1])[band])
    _, keep = oracle(65, 3, 2, True, True)
    np.testing.assert_allclose(p.values[keep], m(TSeries(t, y), band, err).values[keep], rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        m(TSeries(t, y), band, err[:-1])
    with pytest.raises(ValueError):
        m(TSeries(t, y), band[:-1], err)
    with pytest.raises(ValueError):
        MultibandGLS(nterms=3)(TSeries(t[:9], y[:9]), np.arange(9) % 3)   # nine columns need ten samples
    bad = y.copy()
    bad[7] = np.nan                                          # NaN in the data propagates, it is not an error
    assert np.all(np.isnan(m(TSeries(t, bad), band, err).values))


def dev_scan(t, y, err, labels, n_bands, f0, delta, nf, nterms):
    """One ``pdc_mbgls_scan_dev`` call on the null stream with buffers of its own."""
    lib = _cabi.lib()
    DB = _cabi.DeviceBuffer
    bufs = [DB.from_array(a) for a in (t, y, err, np.asarray(labels, dtype=np.int32))] + [DB(nf * 8)]
    try:
        _cabi.check(lib.pdc_mbgls_scan_dev(0, None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, t.size, n_bands,
                                           f0, delta, 0, nf, nterms, 1, 0, bufs[4].ptr))
        _cabi.check(lib.pdc_device_sync(0))
        return bufs[4].to_array(np.float64, nf)
    finally:
        for b in bufs:
            b.free()


def test_dev_entry_gives_the_bits_of_the_host_entry():
    t, y, err, band = curve(65, 3)
    f0, delta, nf = _cabi.grid_params(grid(65))
    assert np.array_equal(dev_scan(t, y, err, band, 3, f0, delta, nf, 2), _cabi.mbgls_scan(t, y, err, band, 3, f0, delta, nf, 2),
                          equal_nan=True)


def test_dev_entry_with_a_label_out_of_range_is_all_nan():
    """The `_dev` form cannot look at the labels: one outside 0 .. B - 1 never indexes memory (the prologue only compares
    labels with band numbers and counts the matches), it raises a flag and every bin is NaN.  One small call."""
    t, y, err, band = curve(65, 3)
    f0, delta, nf = _cabi.grid_params(grid(65))
    wrong = band.copy()
    wrong[40] = 3
    assert np.all(np.isnan(dev_scan(t, y, err, wrong, 3, f0, delta, nf, 2)))


def test_hygiene_no_allocation_on_a_repeated_or_rejected_call():
    t, y, err, band = curve(200, 6)
    f0, delta, nf = _cabi.grid_params(grid(200))
    first = _cabi.mbgls_scan(t, y, err, band, 6, f0, delta, nf, 3)
    counts = _cabi.alloc_counts()
    again = _cabi.mbgls_scan(t, y, err, band, 6, f0, delta, nf, 3)
    assert _cabi.alloc_counts() == counts and np.array_equal(first, again, equal_nan=True)
    with pytest.raises(ValueError):
        _cabi.mbgls_scan(t[:8], y[:8], err[:8], band[:8], 6, f0, delta, nf, 3)
    assert _cabi.alloc_counts() == counts
