"""The device-resident ragged entries (pdc_*_scan_ragged_dev) against their host entries: the rows bit for bit, the
pitched copy as periodicity_hip.h documents it for each entry (FSeries order; negated for PDM and StringLength, as is for
GLS and BLS power) with an untouched NaN pad, in a workspace of exactly pdc_*_ragged_work_bytes bytes."""
import ctypes as C

import numpy as np
import pytest

from periodicity_amd import _cabi
from periodicity_amd.phase import _linspace_steps

pytestmark = pytest.mark.gpu

SIZES = (37, 64, 150)
CASES = ("rows", "pitched", "both")
DEV = 0


class Curves:
    """Three curves of 37, 64 and 150 samples; `rows`: their grid lengths (0, 5 and one tile + 3, or 70 where the tile
    is one row)."""

    def __init__(self, rows, keep=(0, 1, 2)):
        rng = np.random.default_rng(41)
        t, y, dy = [], [], []
        for n in SIZES:
            tb = np.sort(rng.uniform(0.0, 0.9 * n, n)) + rng.uniform(-20.0, 20.0)
            t.append(tb)
            y.append(10.0 + np.sin(tb / 2.3) - 0.8 * ((tb / 5.1) % 1 < 0.1) + 0.1 * rng.standard_normal(n))
            dy.append(rng.uniform(0.05, 0.2, n))
        t, y, dy = ([a[b] for b in keep] for a in (t, y, dy))
        self.count = np.array([rows[b] for b in keep], dtype=np.int64)
        self.B = len(keep)
        self.spans = np.array([a[-1] - a[0] for a in t])
        self.each_y = y
        self.t, self.y, self.dy = np.concatenate(t), np.concatenate(y), np.concatenate(dy)
        self.offsets = np.concatenate([[0], np.cumsum([a.size for a in t])]).astype(np.int64)
        self.roff = np.concatenate([[0], np.cumsum(self.count)]).astype(np.int64)
        self.total, self.pitch = int(self.roff[-1]), int(self.count.max()) + 2

    def period_grid(self):
        """linspace(1.5, span / 2, rows) per curve: start, step, stop."""
        start, stop = np.full(self.B, 1.5), self.spans / 2
        return start, _linspace_steps(start, stop, self.count), stop

    def split(self, flat):
        return [flat[self.roff[b]:self.roff[b + 1]] for b in range(self.B)]


class Device:
    """A stream and the buffers of one test, freed at its end."""

    def __init__(self):
        self.lib, self.held = _cabi.lib(), []
        sp = C.c_void_p()
        _cabi.check(self.lib.pdc_stream_create(DEV, C.byref(sp)))
        self.stream = sp.value

    def up(self, a):
        self.held.append(_cabi.DeviceBuffer.from_array(a, DEV))
        return self.held[-1]

    def new(self, nbytes):
        self.held.append(_cabi.DeviceBuffer(max(int(nbytes), 8), DEV))
        return self.held[-1]

    def sync(self):
        _cabi.check(self.lib.pdc_stream_sync(DEV, self.stream))

    def close(self):
        self.sync()
        for b in self.held:
            b.free()
        _cabi.check(self.lib.pdc_stream_destroy(DEV, self.stream))


@pytest.fixture
def dev():
    d = Device()
    yield d
    d.close()


def outputs(dev, c, case):
    """(rows buffer | None, NaN-filled pitched buffer | None) of a case."""
    rows = dev.new(c.total * 8) if case in ("rows", "both") else None
    pitched = dev.up(np.full(c.B * c.pitch, np.nan)) if case in ("pitched", "both") else None
    return rows, pitched


def check_rows(c, rows, want):
    if rows is not None:
        assert np.array_equal(rows.to_array(np.float64, c.total), want, equal_nan=True)


def check_pitched(c, pitched, want_rows):
    """want_rows[b]: curve b's row as the pitched copy holds it; everything behind it is still the caller's NaN."""
    if pitched is None:
        return
    got = pitched.to_array(np.float64, c.B * c.pitch).reshape(c.B, c.pitch)
    for b, want in enumerate(want_rows):
        assert want.size == c.count[b]
        assert np.array_equal(got[b, :want.size], want, equal_nan=True), b
        assert np.isnan(got[b, want.size:]).all(), b


def fseries(rows, reverse):
    return [r[::-1] if rev else r for r, rev in zip(rows, reverse)]


def ptr(buf):
    return None if buf is None else buf.ptr


# ---- GLS: fit_mean = 1, psd = 0, with dy; the tile is 1024 bins ------------------------------------------------------
@pytest.fixture(scope="module")
def gls():
    c = Curves((0, 5, 1024 + 3))
    c.f0 = 0.4 / c.spans
    c.delta = np.array([0.013, 0.007, 0.0004])
    c.power, c.amax, c.argmax = _cabi.gls_scan_ragged(c.t, c.y, c.dy, c.offsets, c.f0, c.delta, c.roff, True, False,
                                                      want_power=True, want_peaks=True, device=DEV)
    return c


@pytest.mark.parametrize("case", CASES + ("peaks",))
def test_gls_dev_entry_matches_the_host_entry(dev, gls, case):
    c, p = gls, _cabi._ptr
    wb = dev.lib.pdc_gls_ragged_work_bytes(c.t.size, c.B, c.total, 0, 0)
    work = dev.new(wb)
    rows, pitched = outputs(dev, c, "rows" if case == "peaks" else case)
    amax, argmax = (dev.new(c.B * 8), dev.new(c.B * 8)) if case == "peaks" else (None, None)
    t, y, dy = dev.up(c.t), dev.up(c.y), dev.up(c.dy)
    _cabi.check(dev.lib.pdc_gls_scan_ragged_dev(DEV, dev.stream, t.ptr, y.ptr, dy.ptr, p(c.offsets), c.B, p(c.f0),
                                                p(c.delta), p(c.roff), 1, 0, ptr(rows), ptr(pitched), c.pitch, ptr(amax),
                                                ptr(argmax), work.ptr, wb))
    dev.sync()
    check_rows(c, rows, c.power)
    check_pitched(c, pitched, c.split(c.power))
    if case == "peaks":
        assert np.array_equal(amax.to_array(np.float64, c.B), c.amax, equal_nan=True)
        assert np.array_equal(argmax.to_array(np.int64, c.B), c.argmax)
        assert c.argmax[0] == -1 and np.isnan(c.amax[0]) and (c.argmax[1:] >= 0).all()


# ---- PDM: the tile is 64 periods; the pitched copy is negated and in FSeries order -----------------------------------
def pdm_curves(keep, significant):
    c = Curves((0, 5, 64 + 3), keep)
    c.grid = c.period_grid()
    c.sigma = np.array([np.var(v, ddof=1) for v in c.each_y])
    c.significant = np.array([1 - 11 / v.size ** 0.8 for v in c.each_y]) if significant else None
    c.out = _cabi.phase_scan_ragged(0, c.t, c.y, c.offsets, *c.grid, c.roff, 5, 2, sigma=c.sigma,
                                    significant=c.significant, device=DEV)[0]
    return c


@pytest.fixture(scope="module")
def pdm():
    return pdm_curves((0, 1, 2), False)


@pytest.fixture(scope="module")
def pdm_sub():
    return pdm_curves((1, 2), True)   # (sub-harmonic averaging needs at least two trial periods)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("which", ["pdm", "pdm_sub"])
def test_pdm_dev_entry_matches_the_host_entry(dev, request, which, case):
    c, p = request.getfixturevalue(which), _cabi._ptr
    wb = dev.lib.pdc_phase_ragged_work_bytes(c.B, c.total, 0, 0)
    work = dev.new(wb)
    rows, pitched = outputs(dev, c, case)
    t, x = dev.up(c.t), dev.up(c.y)
    start, step, stop = c.grid
    _cabi.check(dev.lib.pdc_phase_scan_ragged_dev(0, DEV, dev.stream, t.ptr, x.ptr, p(c.offsets), c.B, p(start), p(step),
                                                  p(stop), p(c.roff), p(c.sigma), p(c.significant), 5, 2, ptr(rows),
                                                  ptr(pitched), c.pitch, work.ptr, wb))
    dev.sync()
    check_rows(c, rows, c.out)
    check_pitched(c, pitched, fseries([-r for r in c.split(c.out)], stop > start))


# ---- StringLength: the tile is one period; the pitched copy is negated and in FSeries order --------------------------
@pytest.fixture(scope="module")
def sl():
    c = Curves((0, 5, 70))
    c.m = np.concatenate([(v - v.max()) / (2 * (v.max() - v.min())) + 0.25 for v in c.each_y])
    stop = 0.1 / c.spans                      # _string_periods: 1 / linspace(count * s, s, count), s = dphi / baseline
    start = c.count * stop
    c.grid = (start, _linspace_steps(start, stop, c.count), stop)
    c.out = _cabi.stringlength_scan_ragged(c.t, c.m, c.offsets, *c.grid, c.roff, device=DEV)[0]
    return c


@pytest.mark.parametrize("case", CASES)
def test_stringlength_dev_entry_matches_the_host_entry(dev, sl, case):
    c, p = sl, _cabi._ptr
    wb = dev.lib.pdc_stringlength_ragged_work_bytes(p(c.offsets), p(c.roff), c.B)
    work = dev.new(wb)
    rows, pitched = outputs(dev, c, case)
    t, m = dev.up(c.t), dev.up(c.m)
    start, step, stop = c.grid
    _cabi.check(dev.lib.pdc_stringlength_scan_ragged_dev(DEV, dev.stream, t.ptr, m.ptr, p(c.offsets), c.B, p(start),
                                                         p(step), p(stop), p(c.roff), ptr(rows), ptr(pitched), c.pitch,
                                                         work.ptr, wb))
    dev.sync()
    check_rows(c, rows, c.out)
    check_pitched(c, pitched, fseries([-r for r in c.split(c.out)], start > stop))


# ---- BLS with dy: the tile is one period; the pitched copy is the power row in FSeries order -------------------------
BLS_SHAPE = (50, 1, 6, 3, 0)   # n_bins, len_min, len_max, min_points, dips_only
BLS_ROWS = (("power", np.float64), ("depth", np.float64), ("start_bin", np.int32), ("box_bins", np.int32))
BLS_BEST = (("index", np.int64),) + BLS_ROWS


@pytest.fixture(scope="module")
def bls():
    c = Curves((0, 5, 70))
    c.grid = c.period_grid()
    c.rows, c.best, _ = _cabi.bls_scan_ragged(c.t, c.y, c.dy, c.offsets, *c.grid, c.roff, *BLS_SHAPE[:4], False,
                                              device=DEV)
    return c


@pytest.mark.parametrize("case", CASES + ("best",))
def test_bls_dev_entry_matches_the_host_entry(dev, bls, case):
    c, p = bls, _cabi._ptr
    wb = dev.lib.pdc_bls_ragged_work_bytes(c.B, c.t.size, c.total, 0, 0)
    work = dev.new(wb)
    with_rows = case in ("rows", "both", "best")
    rows = [dev.new(c.total * np.dtype(kind).itemsize) if with_rows else None for _, kind in BLS_ROWS]
    best = [dev.new(c.B * np.dtype(kind).itemsize) if case == "best" else None for _, kind in BLS_BEST]
    pitched = dev.up(np.full(c.B * c.pitch, np.nan)) if case in ("pitched", "both") else None
    t, y, dy = dev.up(c.t), dev.up(c.y), dev.up(c.dy)
    start, step, stop = c.grid
    _cabi.check(dev.lib.pdc_bls_scan_ragged_dev(DEV, dev.stream, t.ptr, y.ptr, dy.ptr, p(c.offsets), c.B, p(start), p(step),
                                                p(stop), p(c.roff), *BLS_SHAPE, *[ptr(b) for b in rows + best],
                                                ptr(pitched), c.pitch, work.ptr, wb))
    dev.sync()
    if with_rows:
        for buf, (name, kind) in zip(rows, BLS_ROWS):
            assert np.array_equal(buf.to_array(kind, c.total), c.rows[name], equal_nan=True), name
    check_pitched(c, pitched, fseries(c.split(c.rows["power"]), stop > start))
    if case == "best":
        for buf, (name, kind) in zip(best, BLS_BEST):
            assert np.array_equal(buf.to_array(kind, c.B), c.best[name], equal_nan=True), name
        assert c.best["index"][0] == -1 and (c.best["index"][1:] >= 0).all()
