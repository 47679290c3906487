"""WPS without a GPU: the oracle against itself (float64 literal recipe and float64 tap sum against the long-double
literal recipe), the product's tap builder against numpy's resampling rule, the product's wavelet table against the
oracle's, ``TFSeries``, the class's argument errors and its marginals' plumbing with ``_cabi.wps_scan`` replaced by the
oracle, the size functions and the C entry's refusals before any device is looked for.
PARITY UNPINNED BY THE REFERENCE (tests/wps_oracle.py)."""
import numpy as np
import pytest

import wps_oracle as wo
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TFSeries, TSeries
from periodicity_amd.timefrequency import WPS, cmor_table

SHAPES = (50, 257, 1000)


def centred(n):
    t, y = wo.curve(n)
    return t, y - np.mean(y)


@pytest.mark.parametrize("n", SHAPES)
def test_float64_recipes_meet_the_long_double_oracle(n):
    """The literal recipe in float64 cancels in its diff: up to 1.6e-14 of max|coef| measured, gated at 1e-13.  The tap
    sum has no cancellation: gated by the rounding budget the GPU tests use, per cell and per part."""
    _, x = centred(n)
    for s in wo.SCALES:
        exact = wo.literal(x, s)
        top = np.max(np.abs(exact))
        literal = wo.literal(x, s, np.complex128)
        assert literal.dtype == np.complex128
        assert np.max(np.abs(literal - exact)) <= 1e-13 * top, (n, s)
        taps = wo.tap_sum(x, s)
        bound, count = wo.budget(x, s)
        assert count <= wo.POINTS + 1
        for part in (np.real, np.imag):
            worst = np.max(np.abs(part(taps) - part(exact)) / bound)
            assert worst <= 1.0, (n, s, float(worst))


def test_the_table_is_the_oracles_bit_for_bit():
    table, step, span = cmor_table()
    _, ostep, otable = wo.table()
    assert table.dtype == np.complex128 and table.tobytes() == otable.tobytes()
    assert step == ostep and span == wo.UPPER - wo.LOWER


@pytest.mark.parametrize("s", wo.TAP_SCALES)
def test_tap_builder_follows_the_numpy_rule(s):
    """The positions where the filter changes, the table entries on either side and the filter's length, from the
    function the device runs, against ``(arange(...) / (s step)).astype(int)``.  63.9375 puts s * step within an ulp of
    1, where the floor lands on either side."""
    _, step, span = cmor_table()
    position, before, after, length = _cabi.wps_taps(s, step, span)
    m, obefore, oafter, olength = wo.change_points(s)
    assert length == olength
    assert np.array_equal(position, m)
    assert np.array_equal(before, obefore) and np.array_equal(after, oafter)
    assert position.size <= wo.POINTS + 1
    if olength + 1 <= wo.POINTS + 1:   # every filter position is a tap
        assert np.array_equal(position, np.arange(olength + 1))


def test_tap_builder_on_a_sweep_of_scales():
    _, step, span = cmor_table()
    rng = np.random.default_rng(5)
    for s in np.concatenate([np.exp(rng.uniform(np.log(1 / 16), np.log(3000), 60)), 63.9375 * np.arange(1, 9)]):
        position, before, after, length = _cabi.wps_taps(s, step, span)
        m, obefore, oafter, olength = wo.change_points(s)
        assert length == olength and np.array_equal(position, m), s
        assert np.array_equal(before, obefore) and np.array_equal(after, oafter), s


def test_tap_builder_refuses_what_it_cannot_serve():
    _, step, span = cmor_table()
    for s in (0.0, -1.0, np.nan, np.inf, 2.0 ** 25):
        with pytest.raises(ValueError):
            _cabi.wps_taps(s, step, span)
    assert _cabi.wps_taps(1 / 32, step, span)[3] < 2   # served, and too short for the transform


# ---- TFSeries ----------------------------------------------------------------------------------------------------------
def grid():
    time = np.arange(5.0)
    frequency = np.array([0.5, 0.25, 0.125])
    values = np.arange(15.0).reshape(3, 5)
    return TFSeries(time, frequency, values)


def test_tfseries_coordinates_and_values():
    tf = grid()
    assert tf.shape == (3, 5) and len(tf) == 3 and tf.median_dt == 1.0
    assert np.array_equal(tf.period, [2.0, 4.0, 8.0]) and np.array_equal(tf.frequency, [0.5, 0.25, 0.125])
    other = tf.copy()
    other.values = np.zeros((3, 5))
    assert tf.values[1, 1] == 6.0 and other.values[1, 1] == 0.0
    with pytest.raises(ValueError):
        other.values = np.zeros((5, 3))
    with pytest.raises(ValueError):
        TFSeries(np.arange(4.0), tf.frequency, tf.values)


def test_tfseries_indexing():
    tf = grid()
    assert tf[1, 2] == 7.0
    row = tf[1]
    assert isinstance(row, TSeries) and np.array_equal(row.values, tf.values[1]) and np.array_equal(row.time, tf.time)
    col = tf[:, 2]
    assert isinstance(col, FSeries) and np.array_equal(np.sort(col.values), [2.0, 7.0, 12.0])
    assert col.values[np.argmax(col.frequency)] == 2.0   # (an FSeries sorts by frequency: the value follows its label)
    keep = np.array([True, False, True])
    sub = tf[keep]
    assert isinstance(sub, TFSeries) and sub.shape == (2, 5) and np.array_equal(sub.frequency, [0.5, 0.125])
    late = tf[:, tf.time >= 3]
    assert isinstance(late, TFSeries) and late.shape == (3, 2) and np.array_equal(late.values, tf.values[:, 3:])
    both = tf[keep, tf.time >= 3]
    assert both.shape == (2, 2) and np.array_equal(both.values, tf.values[[0, 2]][:, 3:])


def test_tfseries_means_skip_nan():
    tf = grid()
    holes = tf.values.copy()
    holes[0, 0] = np.nan
    holes[2, :] = np.nan
    tf.values = holes
    with pytest.warns(RuntimeWarning):   # numpy's "mean of empty slice" for the all-NaN row
        over_time = tf.mean("time")
    assert isinstance(over_time, FSeries)
    by_frequency = dict(zip(over_time.frequency, over_time.values))
    assert by_frequency[0.5] == np.mean([1.0, 2.0, 3.0, 4.0]) and by_frequency[0.25] == 7.0
    assert np.isnan(by_frequency[0.125])
    over_frequency = tf.mean("frequency")
    assert isinstance(over_frequency, TSeries) and np.array_equal(over_frequency.values, [5.0, 3.5, 4.5, 5.5, 6.5])
    assert tf.mean() == np.nanmean(holes)
    with pytest.raises(ValueError):
        tf.mean("period")


# ---- the class ---------------------------------------------------------------------------------------------------------
def oracle_scan(x, t, periods, scales, table, step, span, corr, want_planes=True, want_coefs=False, device=None):
    """What ``_cabi.wps_scan`` returns, from the float64 literal recipe and numpy's reductions."""
    assert table.tobytes() == wo.table()[2].tobytes() and corr == np.exp2(0.5)
    coefs, plane = wo.spectrum(x, scales, np.complex128)
    mask = wo.mask_coi(t, periods)
    gwps, sav, mg, ms, gc, sc = wo.marginals(plane, mask)
    return {"spectrum": plane if want_planes else None, "coefs": coefs if want_coefs else None, "gwps": gwps, "sav": sav,
            "masked_gwps": mg, "masked_sav": ms, "gwps_count": gc.astype(np.int64), "sav_count": sc.astype(np.int64)}


def test_gwps_of_a_sinusoid_peaks_at_its_period(monkeypatch):
    monkeypatch.setattr(_cabi, "wps_scan", oracle_scan)
    t = 0.02 * np.arange(2000)
    periods = np.linspace(0.5, 5, 46)
    wps = WPS(periods)
    spectrum = wps(TSeries(t, np.sin(2 * np.pi * t / 2)))
    assert isinstance(spectrum, TFSeries) and spectrum.shape == (46, 2000)
    assert np.array_equal(spectrum.frequency, 1.0 / periods)   # the order given
    gwps = wps.gwps()
    assert isinstance(gwps, FSeries) and gwps.pmax() == pytest.approx(2.0, abs=1e-12)
    assert wps.masked_gwps().pmax() == pytest.approx(2.0, abs=1e-12)
    assert np.allclose(wps.scales, periods / 0.02) and np.allclose(wps.power.values, spectrum.values * wps.scales[:, None])


def test_marginals_with_and_without_a_range(monkeypatch):
    monkeypatch.setattr(_cabi, "wps_scan", oracle_scan)
    t, y = wo.curve(300)
    periods = np.array([0.05, 0.3, 1.0, 4.0])
    wps = WPS(periods)
    wps(TSeries(t, y), want_coefs=True)
    plane = wps.spectrum.values
    assert wps.coefs.shape == plane.shape and wps.coefs.dtype == np.complex128
    mask = wps.mask_coi
    assert np.array_equal(mask, wo.mask_coi(t, periods)) and mask.any() and not mask.all()
    assert np.array_equal(np.isnan(wps.masked_spectrum.values), ~mask)
    assert np.array_equal(wps.gwps_count, mask.sum(axis=1)) and np.array_equal(wps.sav_count, mask.sum(axis=0))
    assert np.isnan(wps.masked_gwps().values).sum() == (mask.sum(axis=1) == 0).sum() > 0
    # a range that keeps everything gives the whole-plane marginal (here both come from numpy: to the last bit)
    everything = wps.gwps(tmin=t[0])
    assert np.array_equal(everything.values, wps.gwps().values)
    inner = wps.sav(pmin=0.2, pmax=2.0)
    assert isinstance(inner, TSeries) and np.allclose(inner.values, plane[1:3].mean(axis=0))
    late = wps.masked_gwps(tmin=t[150])
    with pytest.warns(RuntimeWarning):   # numpy's "mean of empty slice": the longest period has no cell in the cone
        want = np.nanmean(np.where(mask, plane, np.nan)[:, 150:], axis=1)
    order = np.argsort(wps.frequency, kind="stable")
    assert np.allclose(late.values, want[order], equal_nan=True)
    border = wps.coi(50)
    assert isinstance(border, TSeries) and np.all(np.diff(border.time) >= 0)


def test_without_planes_ranges_are_refused(monkeypatch):
    monkeypatch.setattr(_cabi, "wps_scan", oracle_scan)
    t, y = wo.curve(120)
    wps = WPS([0.1, 0.5])
    assert wps(TSeries(t, y), want_planes=False) is None
    assert wps.spectrum is None and wps.masked_spectrum is None and wps.coefs is None
    assert wps.gwps().size == 2 and wps.sav().size == 120 and wps.masked_sav().size == 120
    for call in (lambda: wps.gwps(tmin=1.0), lambda: wps.masked_gwps(tmax=4.0), lambda: wps.sav(pmin=0.2),
                 lambda: wps.masked_sav(pmax=0.2), lambda: wps.power):
        with pytest.raises(ValueError):
            call()


def test_argument_errors(monkeypatch):
    def never(*args, **kwargs):
        raise AssertionError("the scan must not be reached")
    monkeypatch.setattr(_cabi, "wps_scan", never)
    t, y = wo.curve(100)
    with pytest.raises(ValueError, match="too small"):   # L < 2: a period of less than dt / 16
        WPS([0.02 / 17])(TSeries(t, y))
    for bad in (np.nan, np.inf):
        broken = y.copy()
        broken[40] = bad
        with pytest.raises(ValueError, match="finite"):
            WPS([0.5])(TSeries(t, broken))
    for periods in ([], [[1.0, 2.0]], [1.0, -2.0], [0.0], [np.nan]):
        with pytest.raises(ValueError):
            WPS(periods)
    with pytest.raises(ValueError):
        WPS([0.5])(TSeries(t[:1], y[:1]))


# ---- the C entry -------------------------------------------------------------------------------------------------------
def test_sizes_without_a_gpu(monkeypatch):
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    assert _cabi.wps_tile() >= 64
    big = _cabi.wps_work_bytes(65536, 512)
    assert 0 < big < 65536 * 512 * 8   # below one plane
    assert 0 < _cabi.wps_work_bytes(1500, 200) < big
    assert _cabi.wps_work_bytes(0, 5) == -1 and _cabi.wps_work_bytes(5, 0) == -1
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "0.03125")   # 32 MiB: fewer column partials
    assert _cabi.wps_work_bytes(65536, 512) <= 32 << 20


def test_refusals_before_any_device():
    table, step, span = cmor_table()
    t, x = centred(64)
    periods = np.array([0.1, 0.5])
    scales = periods / 0.02
    corr = np.exp2(0.5)
    good = dict(x=x, t=t, periods=periods, scales=scales, table=table, step=step, span=span, corr=corr)

    def scan(**change):
        args = dict(good, **change)
        return _cabi.wps_scan(args["x"], args["t"], args["periods"], args["scales"], args["table"], args["step"],
                              args["span"], args["corr"], device=0)
    broken = x.copy()
    broken[3] = np.nan
    late = t.copy()
    late[5] = np.inf
    dented = table.copy()
    dented[7] = np.nan
    for change, text in ((dict(x=broken), "x[3]"), (dict(t=late), "t[5]"), (dict(scales=np.array([5.0, 1 / 32])), "scales[1]"),
                         (dict(scales=np.array([np.nan, 5.0])), "scales[0]"), (dict(periods=np.array([0.1, np.inf])), "periods[1]"),
                         (dict(step=0.0), "step"), (dict(span=-1.0), "span"), (dict(table=dented), "table"),
                         (dict(corr=np.nan), "factor")):
        with pytest.raises(ValueError) as info:
            scan(**change)
        assert text in str(info.value), (change.keys(), str(info.value))
    with pytest.raises(ValueError):
        scan(t=t[:10])
    with pytest.raises(ValueError):
        scan(table=table[:100])
    if _cabi.device_count() == 0:   # no CPU fallback: a valid call fails loudly
        with pytest.raises(RuntimeError):
            scan()
