"""MultibandGLS without a GPU: the test-local oracle (tests/mbgls_oracle.py) against itself in 80-bit arithmetic, against
the multi-harmonic oracle with one band and against ``np.linalg.lstsq``, the science case the class exists for, the C ABI
and everything it refuses before it looks for a device.  The reference has no such class - PARITY UNPINNED BY THE
REFERENCE."""
import numpy as np
import pytest

import mbgls_oracle as mb
import mhgls_oracle as mo
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.spectral import GLS, MultibandGLS

INVALID, NODEVICE = -1, -2
BANDS = (1, 2, 3, 6)


def shapes(n):
    """(bands, largest nterms) of curve ``n``: twelve samples carry at most 3 offsets and 2 harmonics."""
    return (BANDS[:3], 2) if n == 12 else (BANDS, 3)


@pytest.mark.parametrize("n", [12, 31, 64, 65, 200])
def test_float64_and_longdouble_oracles_agree_on_kept_bins(n):
    bands, hmax = shapes(n)
    for B in bands:
        t, y, err, band = mb.curve(n, B)
        freq = GLS()._grid(TSeries(t, y))
        for fit_mean in (True, False):
            for e in (err, None):
                M64, b64, YY64, W64 = mb.normal_equations(t, y, e, band, B, freq, hmax, fit_mean, np.float64)
                M80, b80, YY80, W80 = mb.normal_equations(t, y, e, band, B, freq, hmax, fit_mean, np.longdouble)
                for nterms in range(1, hmax + 1):
                    d = mb.columns(B, nterms, fit_mean)
                    keep = mb.cond_from(M64[:, :d, :d]) <= mb.COND_LIMIT
                    assert 1 - keep.mean() <= 0.05, (B, nterms, fit_mean, 1 - keep.mean())
                    p64 = mb.power_from(M64[:, :d, :d], b64[:, :d], YY64, W64)
                    p80 = mb.power_from(M80[:, :d, :d], b80[:, :d], YY80, W80)
                    assert np.max(np.abs(p64[keep] - p80[keep])) <= 1e-11
                    assert np.all((p80[keep] >= 0) & (p80[keep] <= 1 + 1e-12))   # a share of the weighted variance
                    assert not np.any(np.isinf(np.asarray(p64[~keep], dtype=float)))   # left out: NaN or finite


@pytest.mark.parametrize("n", [31, 65, 200])
def test_one_band_is_the_multi_harmonic_oracle(n):
    t, y, err, band = mb.curve(n, 1)
    assert np.all(band == 0)
    freq = GLS()._grid(TSeries(t, y))
    for nterms in (1, 2, 3):
        for fit_mean in (True, False):
            keep = mo.cond(t, y, err, freq, nterms, fit_mean) <= mo.COND_LIMIT
            got = mb.power(t, y, err, band, 1, freq, nterms, fit_mean)
            want = mo.power(t, y, err, freq, nterms, fit_mean)
            assert np.max(np.abs(got[keep] - want[keep])) <= 1e-12


def test_power_is_the_chi_square_drop_of_a_least_squares_fit():
    """On ten bins: 1 - chi2_min / chi2_0 from np.linalg.lstsq on the raw values, chi2_0 being that of the model of one
    weighted mean per band."""
    t, y, err, band = mb.curve(200, 3)
    freq = GLS()._grid(TSeries(t, y))
    pick = np.linspace(20, freq.size - 1, 10).astype(int)
    assert np.all(mb.cond(t, y, err, band, 3, freq[pick], 2) <= mb.COND_LIMIT)
    got = np.asarray(mb.power(t, y, err, band, 3, freq[pick], 2, dtype=np.float64))
    onehot = (band[:, None] == np.arange(3)[None, :]).astype(float)
    chi2 = lambda A: np.sum(((y - A @ np.linalg.lstsq(A / err[:, None], y / err, rcond=None)[0]) / err) ** 2)
    for j, f in enumerate(freq[pick]):
        arg = 2 * np.pi * f * t
        A = np.hstack([onehot, np.stack([np.cos(arg), np.sin(arg), np.cos(2 * arg), np.sin(2 * arg)], axis=1)])
        assert abs(got[j] - (1 - chi2(A) / chi2(onehot))) <= 1e-10


def test_a_constant_added_per_band_changes_nothing():
    t, y, err, band = mb.curve(65, 3)
    freq = GLS()._grid(TSeries(t, y))
    keep = mb.cond(t, y, err, band, 3, freq, 2) <= mb.COND_LIMIT
    a = mb.power(t, y, err, band, 3, freq, 2)
    b = mb.power(t, y + np.array([3.0, -1.5, 40.0])[band], err, band, 3, freq, 2)
    assert np.max(np.abs(a[keep] - b[keep])) <= 1e-12


def test_sparse_multiband_curve_needs_the_multiband_statistic():
    """Six bands of twelve epochs: the multiband oracle peaks at the period, the merged curve with one mean does not."""
    t, y, err, band = mb.sparse_fixture()
    freq = GLS(fmin=0.5, fmax=3.0)._grid(TSeries(t, y))
    assert freq.size == 4964
    multi = np.asarray(mb.power(t, y, err, band, 6, freq, 1, dtype=np.float64))
    merged = np.asarray(mo.power(t, y, err, freq, 1, dtype=np.float64))
    p_multi, p_merged = 1 / freq[np.nanargmax(multi)], 1 / freq[np.nanargmax(merged)]
    print(f"sparse fixture: multiband peak {p_multi:.6f} (power {np.nanmax(multi):.3f}), merged peak {p_merged:.6f} "
          f"(power {np.nanmax(merged):.3f})")
    assert abs(p_multi - mb.SPARSE_PERIOD) <= 1e-3 * mb.SPARSE_PERIOD
    assert abs(p_merged - mb.SPARSE_PERIOD) > 1e-3 * mb.SPARSE_PERIOD


def test_class_signature_and_validation():
    assert issubclass(MultibandGLS, GLS)
    for bad in (0, 4):
        with pytest.raises(ValueError):
            MultibandGLS(nterms=bad)
    m = MultibandGLS(0.01, 0.4, 3, True, nterms=3, device=0)
    assert (m.fmin, m.fmax, m.n, m.psd, m.nterms, m.device) == (0.01, 0.4, 3, True, 3, 0)
    assert MultibandGLS().nterms == 1
    for call in (lambda: m.bootstrap(10), lambda: m.fap(0.5), lambda: m.fal(0.01), lambda: m.batch([np.ones(20)]),
                 lambda: m.window()):
        with pytest.raises(NotImplementedError):
            call()
    t, y, err, band = mb.curve(31, 3)
    with pytest.raises(ValueError):
        m(TSeries(t, y), band[:-1], err)   # labels of another length, refused before the library is called


def test_model_and_offsets_are_the_weighted_least_squares_fit():
    """``model`` and ``band_offsets`` need only the attributes a call leaves behind: set by hand, compared with lstsq on
    the same design built around another time origin (the fit does not depend on it)."""
    t, y, err, band = mb.curve(200, 3)
    labels = np.array(["g", "i", "r"])
    m = MultibandGLS(nterms=2)
    m.signal, m.err, m.fit_mean, m.bands, m.band_index = TSeries(t, y), err, True, labels, band.astype(np.int32)
    tf = np.linspace(t[0], t[-1], 57)
    arg = lambda times: 2 * np.pi * np.asarray(times) / 6.3
    series = lambda times: np.stack([f(h * arg(times)) for h in (1, 2) for f in (np.sin, np.cos)], axis=1)
    onehot = (band[:, None] == np.arange(3)[None, :]).astype(float)
    coef = np.linalg.lstsq(np.hstack([onehot, series(t)]) / err[:, None], y / err, rcond=None)[0]
    for b, label in enumerate(labels):
        got = m.model(tf, label, 1 / 6.3)
        assert isinstance(got, TSeries) and np.max(np.abs(got.values - (coef[b] + series(tf) @ coef[3:]))) <= 1e-9
    offsets = m.band_offsets(1 / 6.3)
    assert list(offsets) == ["g", "i", "r"] and np.allclose([offsets[k] for k in labels], coef[:3], atol=1e-9)
    with pytest.raises(ValueError):
        m.model(tf, "z", 1 / 6.3)


def test_symbols_and_tile_bins():
    names = ("pdc_mbgls_scan", "pdc_mbgls_scan_dev", "pdc_mbgls_tile_bins")
    assert all(s in _cabi.PROTOTYPES and hasattr(_cabi.lib(), s) for s in names)
    for nterms in (1, 2, 3):
        tile = _cabi.mbgls_tile_bins(nterms)
        assert tile > 0 and tile % 256 == 0
    assert _cabi.mbgls_tile_bins(0) == -1 and _cabi.mbgls_tile_bins(4) == -1


T = np.array([0.0, 1.1, 2.3, 3.2, 4.7, 5.1, 6.4, 7.9])
Y = np.array([1.0, 0.4, -0.3, 0.8, 1.2, -0.9, 0.1, 0.6])
DY = np.full(8, 0.1)
BAND = np.array([0, 1, 0, 1, 1, 0, 0, 1], dtype=np.int32)
OUT = np.empty(64)
VALID = dict(t=T, y=Y, dy=DY, band=BAND, n=8, n_bands=2, f0=0.01, delta=0.01, j_begin=0, nf=4, nterms=1, fit_mean=1, psd=0,
             power=OUT, device=0)
REJECTED = [
    (dict(t=None), "mbgls: NULL argument"),
    (dict(y=None), "mbgls: NULL argument"),
    (dict(band=None), "mbgls: NULL argument"),
    (dict(power=None), "mbgls: NULL argument"),
    (dict(n=-1), "mbgls: negative size"),
    (dict(nf=-1), "mbgls: negative size"),
    (dict(j_begin=-1), "mbgls: negative size"),
    (dict(nterms=0), "mbgls: nterms must be 1 .. 3 (got 0)"),
    (dict(nterms=4), "mbgls: nterms must be 1 .. 3 (got 4)"),
    (dict(n_bands=0), "mbgls: n_bands must be 1 .. 32 (got 0)"),
    (dict(n_bands=33), "mbgls: n_bands must be 1 .. 32 (got 33)"),
    (dict(delta=0.0), "mbgls: the grid step must be finite and positive"),
    (dict(delta=-0.1), "mbgls: the grid step must be finite and positive"),
    (dict(delta=float("nan")), "mbgls: the grid step must be finite and positive"),
    (dict(band=np.array([0, 1, 0, 2, 1, 0, 0, 1], dtype=np.int32)), "mbgls: band[3] = 2 is not a label in 0 .. 1"),
    (dict(band=np.array([0, -1, 0, 1, 1, 0, 0, 1], dtype=np.int32)), "mbgls: band[1] = -1 is not a label in 0 .. 1"),
    (dict(n_bands=3), "mbgls: band 2 has no samples"),
    (dict(band=np.ones(8, dtype=np.int32)), "mbgls: band 0 has no samples"),
    (dict(nterms=3), "mbgls: 8 parameters are fitted, at least 9 samples are needed (got 8)"),
    (dict(n=4, nterms=2, fit_mean=0), "mbgls: 4 parameters are fitted, at least 5 samples are needed (got 4)"),
]


def call(**changed):
    args = dict(VALID)
    assert set(changed) <= set(args)
    args.update(changed)
    lib = _cabi.lib()
    status = lib.pdc_mbgls_scan(*[_cabi._ptr(v) if isinstance(v, np.ndarray) else v for v in args.values()])
    return status, lib.pdc_last_error().decode()


@pytest.mark.parametrize("changed,text", REJECTED, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(REJECTED)])
def test_a_bad_call_is_refused_with_its_text_before_any_device(changed, text):
    # device 99 exists nowhere: a call that reached the device table would say so (or PDC_ERR_NODEVICE) instead
    assert call(device=99, **changed) == (INVALID, text)


def test_the_binding_raises_value_error_for_what_the_library_refuses():
    common = dict(f0=0.01, delta=0.01, nf=4, device=99)
    for kw in (dict(nterms=0), dict(nterms=4), dict(n_bands=0), dict(n_bands=33), dict(n_bands=3), dict(delta=0.0),
               dict(delta=float("nan")), dict(nterms=3), dict(band=np.where(BAND == 1, 2, 0))):
        args = dict(band=BAND, n_bands=2, **common)
        args.update(kw)
        with pytest.raises(ValueError, match="mbgls: "):
            _cabi.mbgls_scan(T, Y, DY, **args)
    for t, y, dy, band in ((T, Y[:-1], None, BAND), (T, Y, DY[:-1], BAND), (T, Y, DY, BAND[:-1])):
        with pytest.raises(ValueError):
            _cabi.mbgls_scan(t, y, dy, band, 2, **common)


def test_without_a_device_a_valid_call_fails_loudly():
    if _cabi.device_count() != 0:
        return   # (a device is visible: tests/test_mbgls_gpu.py runs the valid calls)
    status, message = call()
    assert status == NODEVICE and message
    t, y, err, band = mb.curve(31, 3)
    with pytest.raises(RuntimeError):      # the class fails loudly, never a CPU answer
        MultibandGLS()(TSeries(t, y), band, err)
