"""The batch front ends of GLS, PDM, AOV, ConditionalEntropy and StringLength on the host side (no GPU needed): every
argument that reaches the ragged bindings of ``_cabi`` is what the single call's own rules give for each curve, computed
here independently of the batch code, and the returned object is assembled from the binding's outputs."""
import numpy as np
import pytest

from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.phase import (AOV, PDM, ConditionalEntropy, PhaseBatch, StringLength, StringLengthBatch,
                                   _pdm_periods, _quarter_scaled, _string_periods)
from periodicity_amd.spectral import GLS, GLSBatch, PeakTable

SIZES, N_PERIODS = (5, 17, 40), 7


def catalogue():
    rng = np.random.default_rng(15)
    sigs = []
    for n in SIZES:
        t = np.sort(rng.uniform(0.0, rng.uniform(30.0, 400.0), n)) + rng.uniform(-50.0, 50.0)
        sigs.append(TSeries(t, 12.0 + np.sin(t / 3.1) + 0.2 * rng.standard_normal(n)))
    return sigs


def fake_table(nb, k):
    """One peak per curve at bin 1 with a crossing on its low side only; the rest is padding."""
    table = _cabi._topk_outputs(nb, k)
    table["count"][:] = 1
    for name in ("indices", "half_lo", "half_hi"):
        table[name][:] = -1
    table["heights"][:] = table["prominences"][:] = np.nan
    table["indices"][:, 0], table["half_lo"][:, 0] = 1, 2
    table["heights"][:, 0] = np.arange(nb) + 0.5
    table["prominences"][:, 0] = 0.25
    return table


def fake_rows(total):
    return np.random.default_rng(3).uniform(0.1, 0.9, total)


def fake_linspace_binding(seen, leading):
    """A stand-in for _cabi.phase_scan_ragged / stringlength_scan_ragged with that function's own parameter list."""
    def body(args):
        seen.update(args)
        out = fake_rows(int(args["p_offsets"][-1])) if args["want_power"] else None
        return out, (fake_table(len(args["offsets"]) - 1, args["k"]) if args["k"] else None)

    if leading == "phase":
        def fake(kind, t, x, offsets, start, step, stop, p_offsets, nb, nc, sigma=None, significant=None, k=0,
                 by_prominence=False, want_power=True, device=None, devices=None):
            return body(locals())
    else:
        def fake(t, m, offsets, start, step, stop, p_offsets, k=0, by_prominence=False, want_power=True, device=None,
                 devices=None):
            return body(locals())
    return fake


def linspace_description(grids_of):
    """start, step, stop of np.linspace(a, b, N_PERIODS) per curve, from numpy itself."""
    start, step, stop = [], [], []
    for a, b in grids_of:
        values, delta = np.linspace(a, b, N_PERIODS, retstep=True)
        start.append(values[0])
        stop.append(values[-1])
        step.append(delta)
    return np.array(start), np.array(step), np.array(stop)


def check_common(seen, sigs, peaks, by_prominence, want_power, device, devices):
    assert np.array_equal(seen["t"], np.concatenate([s.time for s in sigs]))
    assert np.array_equal(seen["offsets"], [0, 5, 22, 62])
    assert seen["k"] == peaks and seen["by_prominence"] is by_prominence and seen["want_power"] is want_power
    assert seen["device"] == device
    assert seen["devices"] is None if devices is None else tuple(seen["devices"]) == devices


def check_table(res, table_of_b, peaks):
    """res.peaks holds the binding's table; its frequencies are those of the FSeries each single call returns."""
    if not peaks:
        assert res.peaks is None
        return
    assert isinstance(res.peaks, PeakTable) and res.peaks.index.shape == (len(SIZES), peaks)
    want = fake_table(len(SIZES), peaks)
    assert np.array_equal(res.peaks.count, want["count"]) and np.array_equal(res.peaks.index, want["indices"])
    assert np.array_equal(res.peaks.height, want["heights"], equal_nan=True)
    assert np.array_equal(res.peaks.prominence, want["prominences"], equal_nan=True)
    for b in range(len(SIZES)):
        frequency = table_of_b(b)
        assert res.peaks.frequency[b, 0] == frequency[1] and res.peaks.period[b, 0] == 1.0 / frequency[1]
        assert res.peaks.period_lo[b, 0] == 1.0 / frequency[2] and np.isnan(res.peaks.period_hi[b, 0])
        assert np.all(np.isnan(res.peaks.frequency[b, 1:]))


CASES = [(0, False, True, None, None), (3, True, True, 2, (1, 1)), (2, False, False, None, (0,))]


@pytest.mark.parametrize("peaks,by_prominence,want_power,device,devices", CASES)
@pytest.mark.parametrize("kind", ["pdm", "aov", "ce"])
def test_phase_batches_pass_the_single_calls_inputs(monkeypatch, kind, peaks, by_prominence, want_power, device, devices):
    seen = {}
    monkeypatch.setattr(_cabi, "phase_scan_ragged", fake_linspace_binding(seen, "phase"))
    sigs = catalogue()
    scan = {"pdm": PDM(nb=4, nc=3, n_periods=N_PERIODS, do_subharmonic=True, device=device, devices=devices),
            "aov": AOV(n_bins=6, n_periods=N_PERIODS, device=device, devices=devices),
            "ce": ConditionalEntropy(n_phase=8, n_mag=4, n_periods=N_PERIODS, device=device, devices=devices)}[kind]
    res = scan.batch(sigs, peaks=peaks, by_prominence=by_prominence, want_power=want_power)
    assert type(res) is PhaseBatch and len(res) == 3
    check_common(seen, sigs, peaks, by_prominence, want_power, device, devices)
    periods = [_pdm_periods(s, None, None, N_PERIODS, 1)[0] for s in sigs]
    start, step, stop = linspace_description([(2 * s.median_dt, s.baseline) for s in sigs])
    for name, want in (("start", start), ("step", step), ("stop", stop), ("p_offsets", [0, 7, 14, 21])):
        assert np.array_equal(seen[name], want), name
    assert (seen["kind"], seen["nb"], seen["nc"]) == {"pdm": (0, 4, 3), "aov": (1, 6, 1), "ce": (2, 8, 4)}[kind]
    if kind == "ce":   # ConditionalEntropy.__call__'s magnitude bins
        bins = []
        for s in sigs:
            low, high = np.nanmin(s.values), np.nanmax(s.values)
            bins.append(np.minimum(np.floor((s.values - low) / (high - low) * 4), 3).astype(float))
        assert np.array_equal(seen["x"], np.concatenate(bins))
    else:
        assert np.array_equal(seen["x"], np.concatenate([s.values for s in sigs]))
    if kind == "pdm":
        assert np.array_equal(seen["sigma"], [np.var(s.values, ddof=1) for s in sigs])
        assert np.array_equal(seen["significant"], [1 - 11 / n ** 0.8 for n in SIZES])
    else:
        assert seen["sigma"] is None and seen["significant"] is None
    for b, p in enumerate(periods):
        assert np.array_equal(res.periods[b], p)
    if want_power:
        out = fake_rows(21)
        for b, p in enumerate(periods):
            single = FSeries(1 / p, out[7 * b:7 * b + 7])
            assert np.array_equal(res.periodograms[b].frequency, single.frequency)
            assert np.array_equal(res.periodograms[b].values, single.values)
    else:
        assert res.periodograms is None
    check_table(res, lambda b: FSeries(1 / periods[b], np.zeros(7)).frequency, peaks)


@pytest.mark.parametrize("peaks,by_prominence,want_power,device,devices", CASES)
def test_stringlength_batch_passes_the_single_calls_inputs(monkeypatch, peaks, by_prominence, want_power, device, devices):
    seen = {}
    monkeypatch.setattr(_cabi, "stringlength_scan_ragged", fake_linspace_binding(seen, "string"))
    sigs = catalogue()
    scan = StringLength(dphi=0.2, n_periods=N_PERIODS, device=device, devices=devices)
    res = scan.batch(sigs, peaks=peaks, by_prominence=by_prominence, want_power=want_power)
    assert type(res) is StringLengthBatch and isinstance(res, PhaseBatch) and len(res) == 3
    check_common(seen, sigs, peaks, by_prominence, want_power, device, devices)
    assert np.array_equal(seen["m"], np.concatenate([_quarter_scaled(s.values) for s in sigs]))
    # _string_periods: 1 / np.linspace(count * s, s, count), s = dphi / baseline
    start, step, stop = linspace_description([(N_PERIODS * (0.2 / s.baseline), 0.2 / s.baseline) for s in sigs])
    for name, want in (("start", start), ("step", step), ("stop", stop), ("p_offsets", [0, 7, 14, 21])):
        assert np.array_equal(seen[name], want), name
    periods = [_string_periods(s.baseline, 0.2, N_PERIODS) for s in sigs]
    for b, p in enumerate(periods):
        assert np.array_equal(res.periods[b], p)
    if want_power:
        out = fake_rows(21)
        for b, p in enumerate(periods):
            single = FSeries(1 / p, out[7 * b:7 * b + 7])
            assert np.array_equal(res.periodograms[b].frequency, single.frequency)
            assert np.array_equal(res.periodograms[b].values, single.values)
    else:
        assert res.periodograms is None
    check_table(res, lambda b: FSeries(1 / periods[b], np.zeros(7)).frequency, peaks)


@pytest.mark.parametrize("peaks,by_prominence,want_power,device,devices", CASES)
def test_gls_batch_passes_the_single_calls_inputs(monkeypatch, peaks, by_prominence, want_power, device, devices):
    seen = {}

    def fake_scan(t, y, dy, offsets, f0, delta, f_offsets, fit_mean=True, psd=False, want_power=True, want_peaks=False,
                  device=None, devices=None):
        seen.update(locals(), k=0, by_prominence=by_prominence)   # (this entry has no table arguments)
        return fake_rows(int(f_offsets[-1])), None, None

    def fake_peaks(t, y, dy, offsets, f0, delta, f_offsets, k=1, by_prominence=False, fit_mean=True, psd=False,
                   want_power=False, device=None, devices=None):
        seen.update(locals())
        out = fake_table(len(offsets) - 1, k)
        out["power"] = fake_rows(int(f_offsets[-1])) if want_power else None
        return out

    monkeypatch.setattr(_cabi, "gls_scan_ragged", fake_scan)
    monkeypatch.setattr(_cabi, "gls_ragged_peaks", fake_peaks)
    sigs = catalogue()
    errs = [np.full(5, 0.3), None, np.linspace(0.1, 0.4, 40)]
    scan = GLS(n=4, psd=True, device=device, devices=devices)
    res = scan.batch(sigs, errs, False, peaks=peaks, by_prominence=by_prominence, want_power=want_power)
    assert isinstance(res, GLSBatch) and len(res) == 3
    check_common(seen, sigs, peaks, by_prominence, want_power, device, devices)
    assert seen["fit_mean"] is False and seen["psd"] is True
    assert np.array_equal(seen["y"], np.concatenate([s.values for s in sigs]))
    assert np.array_equal(seen["dy"], np.concatenate([errs[0], np.ones(17), errs[2]]))
    grids = [scan._grid(s) for s in sigs]
    assert all(g.size > 3 for g in grids)
    assert np.array_equal(seen["f0"], [g[0] for g in grids])
    assert np.array_equal(seen["delta"], [g[1] - g[0] for g in grids])
    f_offsets = np.concatenate([[0], np.cumsum([g.size for g in grids])])
    assert np.array_equal(seen["f_offsets"], f_offsets)
    for b, g in enumerate(grids):
        assert np.array_equal(res.frequency[b], g)
    if want_power:
        out = fake_rows(int(f_offsets[-1]))
        for b, g in enumerate(grids):
            assert np.array_equal(res.periodograms[b].frequency, g)
            assert np.array_equal(res.periodograms[b].values, out[f_offsets[b]:f_offsets[b + 1]])
    else:
        assert res.periodograms is None
    check_table(res, lambda b: grids[b], peaks)


def test_gls_batch_without_errors_passes_no_dy(monkeypatch):
    seen = {}

    def fake_scan(t, y, dy, offsets, f0, delta, f_offsets, fit_mean=True, psd=False, want_power=True, want_peaks=False,
                  device=None, devices=None):
        seen.update(locals())
        return fake_rows(int(f_offsets[-1])), None, None

    monkeypatch.setattr(_cabi, "gls_scan_ragged", fake_scan)
    sigs = catalogue()
    GLS(devices=()).batch(sigs)
    assert seen["dy"] is None and seen["devices"] is None and seen["fit_mean"] is True and seen["psd"] is False
    GLS().batch(sigs, [None, None, None])
    assert seen["dy"] is None
