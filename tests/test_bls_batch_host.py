"""BLS.batch on the host side (no GPU needed): argument validation before any library call, the assembly of a BLSBatch
from the binding's outputs, the library's own checks (they come before any device work), and that without a device the
call fails in the library (never a CPU answer)."""
import numpy as np
import pytest

from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.phase import BLS, BLSBatch, PhaseBatch, _pdm_periods


def curves(count=5, seed=9):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(count):
        n = int(rng.integers(12, 200))
        t = np.sort(rng.uniform(0.0, rng.uniform(20.0, 900.0), n)) + rng.uniform(-1e3, 1e3)
        out.append(TSeries(t, 10.0 - ((t / 7.3) % 1 < 0.05) + 0.1 * rng.standard_normal(n)))
    return out


def test_arguments_are_checked_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("reached the library")

    monkeypatch.setattr(_cabi, "bls_scan_ragged", no_library)
    sigs = curves()
    with pytest.raises(ValueError, match="errs has 2 entries for 5 signals"):
        BLS().batch(sigs, [None, None])
    with pytest.raises(ValueError, match="incompatible lengths"):
        BLS().batch(sigs, [None, np.ones(len(sigs[1]) + 1), None, None, None])
    with pytest.raises(ValueError, match="at least one signal"):
        BLS().batch([])
    for k in (-1, 1025):
        with pytest.raises(ValueError, match="peaks must be 0 .. 1024"):
            BLS().batch(sigs, peaks=k)
    with pytest.raises(ValueError, match="curve 1: a peak table needs a period grid of one sign"):
        BLS(p_max=30.0).batch([sigs[0], TSeries(np.array([0.0, 0.0]), np.array([1.0, 2.0]))], peaks=2)
    with pytest.raises(ValueError, match="curve 0: a peak table needs a period grid of one sign"):
        BLS(p_min=-2.0, p_max=30.0).batch(sigs[:3], peaks=2)


def fake_binding(seen):
    """A stand-in for _cabi.bls_scan_ragged that records its arguments and returns made-up rows: curve 0 has its
    maximum at period index 3 (and again, equal, at 7), curve 1 has no finite power."""
    def fake(t, y, dy, offsets, start, step, stop, p_offsets, n_bins, len_min, len_max, min_points=5, dips_only=False,
             k=0, by_prominence=False, want_power=True, device=None, devices=None):
        seen.update(locals())
        total, nb = int(p_offsets[-1]), len(offsets) - 1
        rng = np.random.default_rng(1)
        rows = {"power": rng.uniform(0.1, 0.5, total), "depth": rng.normal(0, 1, total),
                "start_bin": rng.integers(0, n_bins, total).astype(np.int32),
                "box_bins": rng.integers(len_min, len_max + 1, total).astype(np.int32)}
        rows["power"][[3, 7]] = 0.9
        rows["start_bin"][3], rows["box_bins"][3] = n_bins - 1, 4       # a box that wraps past phase 1
        rows["power"][5] = np.nan                                        # a period without a box
        rows["depth"][5], rows["start_bin"][5], rows["box_bins"][5] = np.nan, -1, -1
        lo, hi = int(p_offsets[1]), int(p_offsets[2])
        rows["power"][lo:hi] = rows["depth"][lo:hi] = np.nan
        rows["start_bin"][lo:hi] = rows["box_bins"][lo:hi] = -1
        best = {name: np.zeros(nb, dtype=rows[src].dtype) for name, src in
                (("power", "power"), ("depth", "depth"), ("start_bin", "start_bin"), ("box_bins", "box_bins"))}
        best["index"] = np.full(nb, -1, dtype=np.int64)
        for b in range(nb):
            row = rows["power"][p_offsets[b]:p_offsets[b + 1]]
            if np.any(~np.isnan(row)):
                best["index"][b] = int(np.nanargmax(row))
                for name in ("power", "depth", "start_bin", "box_bins"):
                    best[name][b] = rows[name][p_offsets[b] + best["index"][b]]
            else:   # what the device writes there; the Python side must not read the junk a binding could leave
                best["power"][b] = best["depth"][b] = np.nan
                best["start_bin"][b] = best["box_bins"][b] = -1
        return (rows if want_power else None), best, None
    return fake


def test_batch_is_assembled_from_the_binding_outputs(monkeypatch):
    seen = {}
    monkeypatch.setattr(_cabi, "bls_scan_ragged", fake_binding(seen))
    sigs = curves(3)
    errs = [np.full(len(sigs[0]), 0.2), None, np.full(len(sigs[2]), 0.3)]
    scan = BLS(n_bins=50, q_min=0.02, q_max=0.12, n_periods=40, min_points=3, dips_only=True)
    assert scan.devices is None
    scan.devices = (0, 0)
    res = scan.batch(sigs, errs)
    assert isinstance(res, BLSBatch) and isinstance(res, PhaseBatch) and len(res) == 3 and res.peaks is None
    # what reaches the binding: the object's parameters, ones for a missing err, no period array
    assert (seen["n_bins"], seen["len_min"], seen["len_max"], seen["min_points"], seen["dips_only"]) == (50, 1, 6, 3, True)
    assert tuple(seen["devices"]) == (0, 0) and seen["k"] == 0 and seen["want_power"] is True
    assert np.array_equal(seen["dy"], np.concatenate([errs[0], np.ones(len(sigs[1])), errs[2]]))
    assert np.array_equal(seen["offsets"], np.concatenate([[0], np.cumsum([len(s) for s in sigs])]))
    assert np.array_equal(seen["p_offsets"], [0, 40, 80, 120])
    for b, s in enumerate(sigs):
        periods = _pdm_periods(s, None, None, 40, 1)[0]
        assert np.array_equal(res.periods[b], periods)
        fs = FSeries(1 / periods, res.power[b])
        assert np.array_equal(res.periodograms[b].frequency, fs.frequency)
        assert np.array_equal(res.periodograms[b].values, fs.values, equal_nan=True)
        # the single call's formulas and NaN rules, per period
        found = ~np.isnan(res.start_bin[b])
        assert np.array_equal(np.isnan(res.box_bins[b]), ~found)
        assert np.array_equal(res.duration[b], res.box_bins[b] / 50 * periods, equal_nan=True)
        assert np.array_equal(res.transit_time[b], ((res.start_bin[b] + res.box_bins[b] / 2) / 50 % 1) * periods,
                              equal_nan=True)
        assert res.power[b].shape == res.depth[b].shape == (40,)
    assert np.isnan(res.start_bin[0][5]) and np.isnan(res.duration[0][5]) and np.isnan(res.transit_time[0][5])
    # curve 0: the first of two equal maxima, a wrapping box; curve 1: nothing finite
    best = res.best
    assert sorted(best) == ["depth", "duration", "index", "period", "power", "transit_time"]
    assert best["index"].tolist()[:2] == [3, -1] and best["index"].dtype == np.int64
    assert best["period"][0] == res.periods[0][3] and best["power"][0] == 0.9 and best["depth"][0] == res.depth[0][3]
    assert best["duration"][0] == 4 / 50 * res.periods[0][3]
    assert best["transit_time"][0] == ((49 + 4 / 2) / 50 % 1) * res.periods[0][3]
    for name in ("period", "power", "depth", "duration", "transit_time"):
        assert np.isnan(best[name][1]), name
        assert best[name][2] == (res.periods[2] if name == "period" else getattr(res, name)[2])[best["index"][2]], name


def test_rows_may_stay_on_the_device_without_a_peak_table(monkeypatch):
    """want_power=False with peaks=0 is a request (``best`` is always produced): the call reaches the binding."""
    seen = {}
    monkeypatch.setattr(_cabi, "bls_scan_ragged", fake_binding(seen))
    res = BLS(n_periods=16).batch(curves(2), want_power=False)
    assert seen["want_power"] is False and seen["k"] == 0 and seen["dy"] is None
    assert res.periodograms is None and res.power is None and res.duration is None and res.peaks is None
    assert res.best["index"].tolist() == [3, -1] and res.best["period"][0] == res.periods[0][3]


def test_an_empty_curve_has_an_empty_grid(monkeypatch):
    seen = {}
    monkeypatch.setattr(_cabi, "bls_scan_ragged", fake_binding(seen))
    sigs = curves(2)
    res = BLS(n_periods=16).batch([sigs[0], sigs[1], TSeries(np.empty(0), np.empty(0))])
    assert np.array_equal(seen["p_offsets"], [0, 16, 32, 32]) and np.array_equal(seen["offsets"][-2:], [seen["t"].size] * 2)
    assert res.periods[2].size == 0 and res.power[2].size == 0 and res.best["index"][2] == -1
    assert np.isnan(res.best["period"][2]) and np.isnan(res.best["transit_time"][2])


def test_library_rejects_bad_descriptions_before_any_device_work():
    t = np.arange(6.0)
    y = np.cos(t)
    good = dict(offsets=[0, 3, 6], start=[1.0, 2.0], step=[0.1, 0.2], stop=[1.3, 2.8], p_offsets=[0, 4, 9])
    shape = dict(n_bins=50, len_min=1, len_max=5, min_points=1)
    for bad, match in [({"offsets": [1, 3, 6]}, "must be 0"), ({"p_offsets": [0, 5, 4]}, "non-decreasing"),
                       ({"offsets": [0, 7, 6]}, "non-decreasing"), ({"n_bins": 1}, "n_bins must be 2 .. 2048"),
                       ({"n_bins": 2049}, "n_bins"), ({"len_max": 50}, "box lengths"), ({"len_min": 0}, "box lengths"),
                       ({"min_points": 0}, "min_points")]:
        args = dict(good, **shape)
        args.update(bad)
        with pytest.raises(ValueError, match=match):
            _cabi.bls_scan_ragged(t, y, None, **args)
    with pytest.raises(ValueError, match="k must be"):
        _cabi.bls_scan_ragged(t, y, None, k=1025, **good, **shape)
    with pytest.raises(ValueError, match="incompatible lengths"):
        _cabi.bls_scan_ragged(t, y, np.ones(5), **good, **shape)
    # the device-resident entry: the same checks, then "no output requested" - all before a device is looked for
    lib = _cabi.lib()
    off, poff = np.array([0, 3, 6], dtype=np.int64), np.array([0, 4, 9], dtype=np.int64)
    grid = [np.array(good[k]) for k in ("start", "step", "stop")]
    nulls = [None] * 10
    status = lib.pdc_bls_scan_ragged_dev(0, None, None, None, None, _cabi._ptr(off), 2, *[_cabi._ptr(g) for g in grid],
                                         _cabi._ptr(poff), 50, 1, 5, 1, 0, *nulls, 0, None, 0)
    assert status == -1 and b"no output requested" in lib.pdc_last_error()
    status = lib.pdc_bls_scan_ragged_dev(0, None, None, None, None, _cabi._ptr(off), 2, *[_cabi._ptr(g) for g in grid],
                                         _cabi._ptr(poff), 50, 1, 50, 1, 0, *nulls, 0, None, 0)
    assert status == -1 and b"box lengths" in lib.pdc_last_error()
    groups = _cabi.bls_ragged_groups()
    assert isinstance(groups, int) and groups >= 0


def test_work_bytes_cover_records_rows_and_the_peak_table():
    lib = _cabi.lib()
    base = lib.pdc_bls_ragged_work_bytes(8, 30_000, 25_000, 0, 0)
    assert base >= 30_000 * 24 + 25_000 * (8 + 8 + 4 + 4) + 8 * 32
    assert lib.pdc_bls_ragged_work_bytes(8, 30_000, 25_000, 4_000, 5) >= base + 8 * 4_000 * 8 + 8 * 5 * 5 * 8
    assert lib.pdc_bls_ragged_work_bytes(8, 60_000, 25_000, 0, 0) >= base + 30_000 * 24 - 256   # (sizes round to 256)
    assert lib.pdc_bls_ragged_work_bytes(0, 30_000, 25_000, 0, 0) == -1
    assert lib.pdc_bls_ragged_work_bytes(8, -1, 25_000, 0, 0) == -1


def test_without_a_device_the_batch_raises_from_the_library():
    if _cabi.device_count() > 0:   # (a GPU box: the same call computes)
        assert np.all(BLS(n_periods=32).batch(curves(3)).best["index"] >= 0)
        return
    with pytest.raises(RuntimeError, match="libperiodicity_hip"):
        BLS().batch(curves(3))
    with pytest.raises(RuntimeError, match="libperiodicity_hip"):
        BLS().batch(curves(3), peaks=3, want_power=False)
