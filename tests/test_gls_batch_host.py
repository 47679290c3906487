"""GLS.batch on the host side (no GPU needed): the per-curve grids it hands the ragged kernel, its input
validation, and that without a device the call fails in the library (never a CPU answer)."""
import numpy as np
import pytest

from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.spectral import BGLST, GLS


def curves(count=12, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(count):
        n = int(rng.integers(2, 400))
        t = np.sort(rng.uniform(0.0, rng.uniform(5.0, 900.0), n)) + rng.uniform(-1e3, 1e3)
        out.append(TSeries(t, np.sin(2 * np.pi * t / rng.uniform(1.0, 50.0)) + rng.normal(0, 0.1, n)))
    return out


def rebuilt(f0, delta, nf):
    j = np.arange(nf, dtype=np.float64)
    return f0 + j * delta   # numpy's own arange fill: start + j*step, two roundings


@pytest.mark.parametrize("kw", [{}, {"fmin": 0.01, "fmax": 0.7, "n": 3}, {"n": 11}])
def test_ragged_grids_reproduce_the_single_call_grid(kw):
    gls = GLS(**kw)
    sigs = curves()
    grids, f0, delta, f_offsets = gls._ragged_grids(sigs)
    assert f_offsets[0] == 0 and np.all(np.diff(f_offsets) >= 0)
    for b, s in enumerate(sigs):
        want = gls._grid(s)
        assert np.array_equal(grids[b], want)
        nf = int(f_offsets[b + 1] - f_offsets[b])
        assert nf == want.size
        assert delta[b] > 0 and np.isfinite(f0[b])
        assert np.array_equal(rebuilt(f0[b], delta[b], nf), want)


def test_ragged_grids_of_fewer_than_two_bins_keep_a_positive_step():
    gls = GLS(fmin=0.2, fmax=0.19, n=5)   # arange(0.2, 0.19 + df, df): one bin
    s = TSeries(np.arange(10.0), np.cos(np.arange(10.0)))
    grids, f0, delta, f_offsets = gls._ragged_grids([s])
    assert grids[0].size == 1 and f_offsets[1] == 1 and delta[0] > 0 and f0[0] == grids[0][0]
    gls = GLS(fmin=0.5, fmax=0.1, n=5)
    grids, f0, delta, f_offsets = gls._ragged_grids([s])
    assert grids[0].size == 0 and f_offsets[1] == 0 and delta[0] > 0


def test_validation_happens_on_the_host(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("reached the library")

    monkeypatch.setattr(_cabi, "gls_scan_ragged", no_device)
    monkeypatch.setattr(_cabi, "gls_ragged_peaks", no_device)
    sigs = curves(3)
    with pytest.raises(ValueError):
        GLS().batch([])
    with pytest.raises(ValueError):
        GLS().batch(sigs, errs=[None, None])
    with pytest.raises(ValueError):
        GLS().batch(sigs, errs=[None, np.ones(3), None])   # wrong length for curve 1
    with pytest.raises(ValueError):
        GLS().batch(sigs, want_power=False)                 # nothing requested
    with pytest.raises(ValueError):
        GLS().batch(sigs, peaks=1025)
    with pytest.raises(NotImplementedError, match="fft"):
        GLS(method="fft").batch(sigs)
    with pytest.raises(NotImplementedError):
        BGLST().batch(sigs)


def test_library_rejects_bad_ragged_descriptions_before_any_device_work():
    t = np.arange(6.0)
    y = np.cos(t)
    good = dict(offsets=[0, 3, 6], f0=[0.1, 0.2], delta=[0.01, 0.02], f_offsets=[0, 4, 9])
    for bad, match in [({"offsets": [1, 3, 6]}, "must be 0"), ({"f_offsets": [0, 5, 4]}, "non-decreasing"),
                       ({"delta": [0.01, 0.0]}, "delta > 0"), ({"f0": [np.nan, 0.2]}, "finite"),
                       ({"delta": [np.inf, 0.1]}, "finite")]:
        args = dict(good, **bad)
        with pytest.raises(ValueError, match=match):
            _cabi.gls_scan_ragged(t, y, None, args["offsets"], args["f0"], args["delta"], args["f_offsets"])
        with pytest.raises(ValueError, match=match):
            _cabi.gls_ragged_peaks(t, y, None, args["offsets"], args["f0"], args["delta"], args["f_offsets"], k=2)
    with pytest.raises(ValueError, match="k must be"):
        _cabi.gls_ragged_peaks(t, y, None, k=0, **good)
    with pytest.raises(ValueError, match="too large"):
        # 2^31 tiles of 1024 bins: refused from the description alone
        _cabi.gls_scan_ragged(t, y, None, [0, 6], [0.1], [1e-9], [0, (1 << 41)], want_power=False, want_peaks=True)


def test_work_bytes_grow_with_the_peak_table():
    lib = _cabi.lib()
    base = lib.pdc_gls_ragged_work_bytes(10_000, 8, 25_000, 4_000, 0)
    assert base >= 10_000 * 48
    assert lib.pdc_gls_ragged_work_bytes(10_000, 8, 25_000, 4_000, 5) >= base + 8 * 4_000 * 8 + 8 * 5 * 5 * 8
    assert lib.pdc_gls_ragged_work_bytes(-1, 8, 25_000, 4_000, 0) == -1


def test_without_a_device_the_batch_raises_from_the_library():
    if _cabi.device_count() > 0:   # (a GPU box: the same call computes)
        assert all(np.isfinite(p.values).all() for p in GLS().batch(curves(4)).periodograms)
        return
    with pytest.raises(RuntimeError, match="libperiodicity_hip"):
        GLS().batch(curves(4))
    with pytest.raises(RuntimeError, match="libperiodicity_hip"):
        GLS().batch(curves(4), peaks=3, want_power=False)
