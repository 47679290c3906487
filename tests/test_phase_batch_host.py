"""PDM.batch / AOV.batch / ConditionalEntropy.batch on the host side (no GPU needed): the per-curve grid
description the ragged kernel rebuilds, argument validation before any device work, and that without a device
the call fails in the library (never a CPU answer)."""
import numpy as np
import pytest

from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.phase import AOV, PDM, ConditionalEntropy, _linspace_at, _linspace_steps


def curves(count=6, seed=4):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(count):
        n = int(rng.integers(5, 300))
        t = np.sort(rng.uniform(0.0, rng.uniform(5.0, 900.0), n)) + rng.uniform(-1e3, 1e3)
        out.append(TSeries(t, np.sin(2 * np.pi * t / rng.uniform(1.0, 50.0)) + rng.normal(0, 0.1, n)))
    return out


@pytest.mark.parametrize("count", [1, 2, 1000])
def test_grid_description_rebuilds_linspace_bit_for_bit(count):
    rng = np.random.default_rng(count)
    starts = rng.uniform(1e-3, 10.0, 300) * 10.0 ** rng.integers(-3, 4, 300)
    stops = starts + rng.uniform(0.0, 1e3, 300) * 10.0 ** rng.integers(-3, 3, 300)
    stops[:5] = starts[:5]                       # one-point ranges
    stops[5:10] = starts[5:10] - 1.0             # descending ones
    counts = np.full(300, count)
    step = _linspace_steps(starts, stops, counts)
    for b in range(300):
        want = np.linspace(starts[b], stops[b], count)
        got = _linspace_at(starts[b], step[b], stops[b], count, np.arange(count))
        assert np.array_equal(got, want), b


def test_arguments_are_checked_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("reached the library")

    monkeypatch.setattr(_cabi, "phase_scan_ragged", no_device)
    sigs = curves()
    for make in (PDM, AOV, ConditionalEntropy):
        with pytest.raises(ValueError):
            make().batch([])
        with pytest.raises(ValueError):
            make().batch(sigs, want_power=False)        # nothing requested
        with pytest.raises(ValueError):
            make().batch(sigs, peaks=1025)
        with pytest.raises(ValueError):
            make().batch(sigs, peaks=-1)
    with pytest.raises(ValueError, match="65280"):
        ConditionalEntropy().batch([sigs[0], TSeries(np.arange(65281.0), np.cos(np.arange(65281.0)))])
    with pytest.raises(ValueError, match="curve 1"):  # a constant curve has no magnitude bins
        ConditionalEntropy().batch([sigs[0], TSeries(np.arange(9.0), np.ones(9))])
    with pytest.raises(ValueError, match="curve 1: a peak table needs a period grid of one sign"):
        PDM(p_max=30.0).batch([sigs[0], TSeries(np.array([0.0, 0.0]), np.array([1.0, 2.0]))], peaks=2)
    with pytest.raises(ValueError, match="curve 0: a peak table needs a period grid of one sign"):
        AOV(p_min=-2.0, p_max=30.0).batch(sigs[:3], peaks=2)
    with pytest.raises(ValueError, match="curve 2"):  # one trial period: no sub-harmonic averaging
        PDM(p_min=1.0, p_max=2.0, n_periods=None, do_subharmonic=True).batch(
                [sigs[0], sigs[1], TSeries(np.array([0.0, 0.4]), np.array([1.0, 2.0]))])


def test_fseries_order_of_descending_and_ascending_grids():
    """The table's bin j of an ascending grid is period index P - 1 - j, of a descending one period index j: the order
    FSeries(1 / periods) puts them in."""
    from periodicity_amd.core import FSeries
    from periodicity_amd.phase import PhaseBatch
    start, stop, count = np.array([0.3, 40.0, 2.0]), np.array([40.0, 0.3, 2.0]), np.array([500, 500, 7])
    step = _linspace_steps(start, stop, count)
    p_off = np.concatenate([[0], np.cumsum(count)])
    res = PhaseBatch(start, step, stop, p_off, np.arange(p_off[-1], dtype=float), None)
    for b in range(3):
        fs = FSeries(1 / res.periods[b], np.zeros(count[b]))
        bins = np.arange(count[b])
        assert np.array_equal(res._frequency_at(np.full(count[b], b), bins), fs.frequency)


def test_library_rejects_bad_descriptions():
    t = np.arange(6.0)
    x = np.cos(t)
    good = dict(offsets=[0, 3, 6], start=[1.0, 2.0], step=[0.1, 0.2], stop=[1.3, 2.8], p_offsets=[0, 4, 9])
    for bad, match in [({"offsets": [1, 3, 6]}, "must be 0"), ({"p_offsets": [0, 5, 4]}, "non-decreasing"),
                       ({"offsets": [0, 7, 6]}, "non-decreasing")]:
        args = dict(good, **bad)
        with pytest.raises(ValueError, match=match):
            _cabi.phase_scan_ragged(1, t, x, args["offsets"], args["start"], args["step"], args["stop"],
                                    args["p_offsets"], 10, 1)
    with pytest.raises(ValueError, match="sigma"):
        _cabi.phase_scan_ragged(0, t, x, nb=5, nc=2, **good)
    with pytest.raises(ValueError, match="kind"):
        _cabi.phase_scan_ragged(3, t, x, nb=5, nc=2, **good)
    with pytest.raises(ValueError, match="k must be"):
        _cabi.phase_scan_ragged(1, t, x, nb=10, nc=1, k=1025, **good)
    with pytest.raises(ValueError, match="two trial periods"):
        _cabi.phase_scan_ragged(1, t, x, [0, 3, 6], [1.0, 2.0], [0.1, 0.2], [1.0, 2.8], [0, 1, 6], 10, 1,
                                significant=[0.5, 0.5])
    with pytest.raises(ValueError, match="histogram bins"):
        _cabi.phase_scan_ragged(2, t, np.zeros(6), nb=40, nc=8, **good)


def test_work_bytes_grow_with_the_peak_table():
    lib = _cabi.lib()
    base = lib.pdc_phase_ragged_work_bytes(8, 25_000, 4_000, 0)
    assert base >= 25_000 * 8
    assert lib.pdc_phase_ragged_work_bytes(8, 25_000, 4_000, 5) >= base + 8 * 4_000 * 8 + 8 * 5 * 5 * 8
    assert lib.pdc_phase_ragged_work_bytes(0, 25_000, 4_000, 0) == -1


def test_without_a_device_the_batch_raises_from_the_library():
    if _cabi.device_count() > 0:   # (a GPU box: the same call computes)
        assert all(np.isfinite(p.values).any() for p in PDM().batch(curves(4)).periodograms)
        return
    for make in (PDM, AOV, ConditionalEntropy):
        with pytest.raises(RuntimeError, match="libperiodicity_hip"):
            make().batch(curves(4))
        with pytest.raises(RuntimeError, match="libperiodicity_hip"):
            make().batch(curves(4), peaks=3, want_power=False)
