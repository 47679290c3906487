"""StringLength.batch on the host side (no GPU needed): the per-curve grid description the ragged kernels rebuild,
argument validation before any device work, and that without a device the call fails in the library (never a CPU
answer)."""
import numpy as np
import pytest

from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.phase import StringLength, StringLengthBatch, _linspace_at, _string_grid, _string_periods


def curves(count=6, seed=4):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(count):
        n = int(rng.integers(5, 300))
        t = np.sort(rng.uniform(0.0, rng.uniform(5.0, 900.0), n)) + rng.uniform(-1e3, 1e3)
        out.append(TSeries(t, np.sin(2 * np.pi * t / rng.uniform(1.0, 50.0)) + rng.normal(0, 0.1, n)))
    return out


@pytest.mark.parametrize("count", [1, 2, 1000])
@pytest.mark.parametrize("dphi", [0.1, 0.37, 1.0, 3])
def test_grid_description_rebuilds_string_periods_bit_for_bit(count, dphi):
    rng = np.random.default_rng(count)
    baselines = rng.uniform(1e-3, 10.0, 300) * 10.0 ** rng.integers(-3, 7, 300)
    start, step, stop = _string_grid(baselines, dphi, count)
    for b in range(baselines.size):
        want = _string_periods(baselines[b], dphi, count)
        got = 1 / _linspace_at(start[b], step[b], stop[b], count, np.arange(count))
        assert np.array_equal(got, want), b


def test_periods_and_table_frequencies_follow_the_single_call():
    baselines = np.array([3.0, 750.5, 1e6])
    start, step, stop = _string_grid(baselines, 0.1, 1000)
    p_off = np.arange(4) * 1000
    res = StringLengthBatch(start, step, stop, p_off, np.zeros(3000), None)
    for b in range(3):
        periods = _string_periods(baselines[b], 0.1, 1000)
        assert np.array_equal(res.periods[b], periods)
        fs = FSeries(1 / periods, np.zeros(1000))
        assert np.array_equal(res._frequency_at(np.full(1000, b), np.arange(1000)), fs.frequency)
        assert np.array_equal(res.periodograms[b].frequency, fs.frequency)


def test_arguments_are_checked_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("reached the library")

    monkeypatch.setattr(_cabi, "stringlength_scan_ragged", no_device)
    sigs = curves()
    with pytest.raises(ValueError):
        StringLength().batch([])
    with pytest.raises(ValueError):
        StringLength().batch(sigs, want_power=False)        # nothing requested
    with pytest.raises(ValueError):
        StringLength().batch(sigs, peaks=1025)
    with pytest.raises(ValueError):
        StringLength().batch(sigs, peaks=-1)
    with pytest.raises(ValueError, match="non-negative"):
        StringLength(n_periods=-1).batch(sigs)
    with pytest.raises(ValueError, match="curve 2"):        # the single call cannot scale an empty curve either
        StringLength().batch(sigs[:2] + [TSeries(np.zeros(0), np.zeros(0))])
    with pytest.raises(ValueError, match="curve 1: a peak table"):   # no baseline: no frequency step
        StringLength().batch([sigs[0], TSeries(np.array([5.0]), np.array([1.0]))], peaks=2)


def test_object_attributes_are_left_alone(monkeypatch):
    monkeypatch.setattr(_cabi, "stringlength_scan_ragged", lambda *a, **k: (np.zeros(int(a[6][-1])), None))
    scan = StringLength()
    scan(curves(1)[0]) if _cabi.device_count() > 0 else None
    before = {k: v for k, v in vars(scan).items()}
    res = scan.batch(curves(3))
    assert isinstance(res, StringLengthBatch) and len(res) == 3
    assert vars(scan).keys() == before.keys() and all(vars(scan)[k] is v for k, v in before.items())


def test_library_rejects_bad_descriptions():
    t = np.arange(6.0)
    m = np.cos(t)
    good = dict(offsets=[0, 3, 6], start=[1.0, 2.0], step=[-0.1, -0.2], stop=[0.7, 1.2], p_offsets=[0, 4, 9])
    for bad, match in [({"offsets": [1, 3, 6]}, "must be 0"), ({"p_offsets": [0, 5, 4]}, "non-decreasing"),
                       ({"offsets": [0, 7, 6]}, "non-decreasing")]:
        args = dict(good, **bad)
        with pytest.raises(ValueError, match=match):
            _cabi.stringlength_scan_ragged(t, m, args["offsets"], args["start"], args["step"], args["stop"],
                                           args["p_offsets"])
    with pytest.raises(ValueError, match="k must be"):
        _cabi.stringlength_scan_ragged(t, m, k=1025, **good)
    assert _cabi.lib().pdc_stringlength_ragged_work_bytes(None, None, 2) == -1


def test_without_a_device_the_batch_raises_from_the_library():
    if _cabi.device_count() > 0:   # (a GPU box: the same call computes)
        assert all(np.isfinite(p.values).any() for p in StringLength().batch(curves(4)).periodograms)
        return
    with pytest.raises(RuntimeError, match="libperiodicity_hip"):
        StringLength().batch(curves(4))
    with pytest.raises(RuntimeError, match="libperiodicity_hip"):
        StringLength().batch(curves(4), peaks=3, want_power=False)
