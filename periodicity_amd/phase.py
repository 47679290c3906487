"""Phase-folding period scans with the reference's callable API, computed on MI355X.

Drop-in for ``periodicity.phase`` (``/root/reference/src/periodicity/phase.py``):

* ``StringLength(dphi, n_periods, cores)(signal) -> FSeries``   (``phase.py:18-72``)
* ``PDM(nb, nc, p_min, p_max, n_periods, oversample, do_subharmonic, cores)(signal) -> FSeries``
  (``phase.py:75-195``)

Positional order, defaults and the attributes each call leaves behind (``.signal .m
.periodogram`` / ``.signal .t .x .sigma .periods .periodogram``) are the reference's.  Upstream maps
one Python task per trial period over a ``multiprocessing.Pool`` (``phase.py:69-70,185-186``);
here a whole period grid is ONE kernel launch (``csrc/stringlength.hip``, ``csrc/pdm.hip``), so
``cores`` is kept only for signature compatibility.  No scan is ever computed on the CPU.
"""
import operator
from multiprocessing import cpu_count

import numpy as np

from . import _cabi
from .core import FSeries, TSeries, _batch_errs, _batch_offsets, _batch_request, _batch_slots

MAX_CORES = cpu_count()

__all__ = ["StringLength", "PDM", "AOV", "ConditionalEntropy", "GregoryLoredo", "SuperSmoother", "BLS", "PhaseBatch",
           "StringLengthBatch", "BLSBatch"]


# ---- host-side grid / scaling rules (O(N) or O(n_periods) numpy, as upstream) -----------------------
def _coerce(signal):
    """Raw array-likes become ``TSeries(values=...)`` (``phase.py:62-63,160-161``); anything that
    already looks like a time series (ours or the reference's xarray-backed one) passes through."""
    looks_like_series = all(hasattr(signal, name) for name in ("time", "values", "baseline"))
    return signal if isinstance(signal, TSeries) or looks_like_series else TSeries(values=signal)


def _quarter_scaled(values):
    """Map the signal onto [-0.25, +0.25] — the intent stated at ``phase.py:65-66`` (NaN-aware
    extrema, ``core.py:202-240``)."""
    top, bottom = np.nanmax(values), np.nanmin(values)
    return (values - top) / (2 * (top - bottom)) + 0.25


def _string_periods(baseline, dphi, count):
    """``count`` trial periods equally spaced in FREQUENCY, from ``baseline / (dphi * count)`` up
    to ``baseline / dphi`` (``phase.py:67-68``)."""
    step = dphi / baseline
    return 1 / np.linspace(count * step, step, count)


def _pdm_limits(signal, p_min, p_max, count, oversample):
    """The limits and the number of trial periods of ``_pdm_periods``."""
    span = signal.baseline
    shortest = 2 * signal.median_dt if p_min is None else p_min
    longest = oversample * span if p_max is None else p_max
    if count is None:
        count = int((1 / shortest - 1 / longest) * oversample * span + 1)
    return shortest, longest, count


def _pdm_periods(signal, p_min, p_max, count, oversample):
    """Trial periods equally spaced in PERIOD (``phase.py:167-180``) and the limits used."""
    shortest, longest, count = _pdm_limits(signal, p_min, p_max, count, oversample)
    return np.linspace(shortest, longest, count), shortest, longest


def _linspace_steps(start, stop, count):
    """Per row, the ``step`` with which ``np.linspace(start, stop, count)`` fills its values: ``j * step + start``
    (two roundings), exactly ``stop`` at the last of two or more.  One value: ``0 * (stop - start) + start``, so the
    step is ``stop - start``.  (numpy divides the other way when the step underflows to zero; such a grid is
    refused.)"""
    start, stop = np.asarray(start, dtype=np.float64), np.asarray(stop, dtype=np.float64)
    count = np.asarray(count, dtype=np.int64)
    delta = stop - start
    with np.errstate(invalid="ignore", divide="ignore"):
        step = np.where(count > 1, delta / np.maximum(count - 1, 1).astype(np.float64), delta)
    bad = (count > 1) & (step == 0) & (delta != 0)
    if bad.any():
        raise ValueError(f"curve {int(np.flatnonzero(bad)[0])}: the period range is too narrow for its grid")
    return step


def _linspace_at(start, step, stop, count, j):
    """``np.linspace(start, stop, count)[j]`` from ``_linspace_steps`` (all arguments broadcast)."""
    j = np.asarray(j, dtype=np.int64)
    fill = j.astype(np.float64) * step + start
    return np.where((count > 1) & (j == count - 1), stop, fill)


def _check_fseries_order(start, step, stop, count):
    """The device writes the peak table's rows in FSeries order, which for a linspace grid of periods is the period
    index reversed (ascending grid: 1/p strictly decreasing) or kept (descending or constant grid: 1/p
    non-decreasing).  That holds when the periods share one sign and, on an ascending grid, no two neighbours round
    to the same reciprocal; any other grid (through zero, non-finite limits) is refused, naming the curve."""
    one_sign = ((start > 0) & (stop > 0)) | ((start < 0) & (stop < 0))
    ok = (count <= 1) | (start == stop) | (one_sign & np.isfinite(start) & np.isfinite(stop))
    if not ok.all():
        b = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"curve {b}: a peak table needs a period grid of one sign (p_min = {start[b]!r}, "
                         f"p_max = {stop[b]!r})")
    # ascending: ties of 1/p need neighbours within a few ulp of each other; check the (rare) fine grids exactly
    fine = np.flatnonzero((stop > start) & (count > 1) & (np.abs(step) < 1e-13 * np.maximum(abs(start), abs(stop))))
    for b in fine:
        p = _linspace_at(start[b], step[b], stop[b], count[b], np.arange(count[b]))
        if not np.all(1 / p[1:] < 1 / p[:-1]):
            raise ValueError(f"curve {int(b)}: neighbouring trial periods share a frequency; no peak table")


class PhaseBatch(object):
    """What ``PDM.batch``, ``AOV.batch`` and ``ConditionalEntropy.batch`` return: ``periods`` (one trial grid per
    curve, ``_pdm_periods``), ``periodograms`` (one ``FSeries(1 / periods, statistic)`` per curve, as the single
    call returns it, or None) and ``peaks`` (a :class:`~periodicity_amd.spectral.PeakTable`, or None)."""

    def __init__(self, start, step, stop, p_offsets, values, peaks):
        self._start, self._step, self._stop, self._p_offsets = start, step, stop, p_offsets
        self._periods = None
        self.peaks = peaks
        self.periodograms = None
        if values is not None:
            self.periodograms = [FSeries(1 / p, values[p_offsets[b]:p_offsets[b + 1]])
                                 for b, p in enumerate(self.periods)]

    @property
    def periods(self):
        if self._periods is None:
            count = np.diff(self._p_offsets)
            rows = np.repeat(np.arange(count.size), count)
            j = np.arange(self._p_offsets[-1], dtype=np.int64) - np.repeat(self._p_offsets[:-1], count)
            with np.errstate(divide="ignore", invalid="ignore"):
                flat = self._period_of(_linspace_at(self._start[rows], self._step[rows], self._stop[rows], count[rows], j))
            self._periods = np.split(flat, self._p_offsets[1:-1])
        return self._periods

    @staticmethod
    def _period_of(grid):
        """The trial periods of the linspace values ``grid``: themselves (a subclass's grids may be reciprocal)."""
        return grid

    def _frequency_at(self, rows, bins):
        """Frequency of bin ``bins`` of ``periodograms[rows]``: ascending frequency, so the period index reversed on
        an ascending grid and kept on a descending one (``_check_fseries_order``)."""
        count = np.diff(self._p_offsets)[rows]
        start, stop = self._start[rows], self._stop[rows]
        j = np.where(stop > start, count - 1 - bins, bins)
        return 1 / _linspace_at(start, self._step[rows], stop, count, j)

    def __len__(self):
        return self._p_offsets.size - 1


def _string_grid(baselines, dphi, count):
    """Per curve, the FREQUENCY linspace of ``_string_periods(baseline, dphi, count)``: ``(start, step, stop)`` with
    ``1 / _linspace_at(start, step, stop, count, j)`` equal to its ``j``-th period, bit for bit."""
    with np.errstate(divide="ignore", invalid="ignore"):
        stop = dphi / np.asarray(baselines, dtype=np.float64)
        start = count * stop
        return start, _linspace_steps(start, stop, np.full(stop.shape, count, dtype=np.int64)), stop


class StringLengthBatch(PhaseBatch):
    """What ``StringLength.batch`` returns: a :class:`PhaseBatch` whose grids are reciprocal linspaces
    (``_string_periods``): ``periods[b] = 1 / linspace(start[b], stop[b], P_b)``, and whose peak table's frequencies
    are ``FSeries(1 / periods).frequency``, i.e. ``1 / (1 / f)``."""

    @staticmethod
    def _period_of(grid):
        return 1 / grid

    def _frequency_at(self, rows, bins):
        """Frequency of bin ``bins`` of ``periodograms[rows]``: ascending frequency, so the index reversed on a
        descending frequency grid (the usual one) and kept otherwise."""
        count = np.diff(self._p_offsets)[rows]
        start, stop = self._start[rows], self._stop[rows]
        j = np.where(start > stop, count - 1 - bins, bins)
        return 1 / (1 / _linspace_at(start, self._step[rows], stop, count, j))


class BLSBatch(PhaseBatch):
    """What ``BLS.batch`` returns: a :class:`PhaseBatch` (``periods``, ``periodograms`` = one
    ``FSeries(1 / periods, power)`` per curve or None, ``peaks``) and, per curve and aligned with ``periods[b]``, the
    lists ``power``, ``depth``, ``start_bin``, ``box_bins``, ``duration``, ``transit_time`` of ``BLS.__call__`` (None
    without ``want_power``).  ``best`` is always there: a dict of ``[B]`` arrays ``index`` (``np.nanargmax`` of the
    power row in period order, -1 for a row without a finite power), ``period``, ``power``, ``depth``, ``duration``,
    ``transit_time`` (NaN where ``index`` is -1), from the maxima found on the device."""

    def __init__(self, start, step, stop, p_offsets, n_bins, rows, best, peaks):
        super().__init__(start, step, stop, p_offsets, None if rows is None else rows["power"], peaks)
        n_bins = int(n_bins)
        self.power = self.depth = self.start_bin = self.box_bins = self.duration = self.transit_time = None
        if rows is not None:
            periods = np.concatenate(self.periods) if len(self) else np.empty(0)
            found = rows["start_bin"] >= 0
            start_bin = np.where(found, rows["start_bin"], np.nan)
            box_bins = np.where(found, rows["box_bins"], np.nan)
            flat = {"power": rows["power"], "depth": rows["depth"], "start_bin": start_bin, "box_bins": box_bins,
                    "duration": box_bins / n_bins * periods,
                    "transit_time": ((start_bin + box_bins / 2) / n_bins % 1) * periods}
            for name, values in flat.items():
                setattr(self, name, np.split(values, p_offsets[1:-1]))
        index = np.asarray(best["index"], dtype=np.int64)
        found = index >= 0
        count = np.diff(p_offsets)
        with np.errstate(invalid="ignore"):
            period = np.where(found, _linspace_at(start, step, stop, count, np.where(found, index, 0)), np.nan)
        start_bin = np.where(found, best["start_bin"], np.nan)
        box_bins = np.where(found, best["box_bins"], np.nan)
        self.best = {"index": np.where(found, index, -1), "period": period,
                     "power": np.where(found, best["power"], np.nan), "depth": np.where(found, best["depth"], np.nan),
                     "duration": box_bins / n_bins * period,
                     "transit_time": ((start_bin + box_bins / 2) / n_bins % 1) * period}


def _period_grids(scan, signals, peaks, empty=None):
    """Per curve, the linspace description of the grid ``_pdm_periods`` gives it from ``scan``'s parameters: ``start,
    step, stop, p_offsets``, checked for a peak table when ``peaks``.  ``empty``: the limits of a curve without samples
    (None: it has none, ``_pdm_limits`` raises)."""
    limits = [_pdm_limits(s, scan.p_min, scan.p_max, scan.n_periods, scan.oversample) if empty is None or s.size else empty
              for s in signals]
    start = np.array([lim[0] for lim in limits], dtype=np.float64)
    stop = np.array([lim[1] for lim in limits], dtype=np.float64)
    count = np.array([lim[2] for lim in limits], dtype=np.int64)
    if (count < 0).any():
        b = int(np.argmax(count < 0))
        raise ValueError(f"curve {b}: number of samples, {count[b]}, must be non-negative")
    step = _linspace_steps(start, stop, count)
    if peaks:
        _check_fseries_order(start, step, stop, count)
    return start, step, stop, _batch_offsets(count)


def _with_peaks(res, table, by_prominence):
    """``res`` with the binding's peak table, if there is one, as its ``peaks``."""
    from .spectral import PeakTable
    if table is not None:
        res.peaks = PeakTable(None, table, by_prominence, frequency_at=res._frequency_at)
    return res


def _bls_batch(scan, signals, errs, peaks, by_prominence, want_power):
    """The batch of :class:`BLS` (``pdc_bls_scan_ragged``): every curve on exactly the grid its own single call would
    scan (``_pdm_limits``), with that call's weights (``errs``, as ``GLS.batch`` takes them)."""
    len_min, len_max = scan.box_lengths()
    signals = [s if isinstance(s, TSeries) else _coerce(s) for s in signals]   # (an empty TSeries has no baseline to probe)
    if not signals:
        raise ValueError("BLS.batch needs at least one signal")
    peaks = _batch_request(peaks)   # (want_power=False alone is a request: ``best`` is always produced)
    values = [np.asarray(s.values, dtype=float) for s in signals]
    sizes = [v.size for v in values]
    dy = _batch_errs(errs, sizes)
    # (a curve without samples has no grid of its own: its row is empty and its best entries are -1 / NaN)
    start, step, stop, p_offsets = _period_grids(scan, signals, peaks, empty=(0.0, 0.0, 0))
    t = np.concatenate([np.asarray(s.time, dtype=float) for s in signals])
    rows, best, table = _cabi.bls_scan_ragged(t, np.concatenate(values), dy, _batch_offsets(sizes), start, step, stop,
                                              p_offsets, int(scan.n_bins), len_min, len_max, int(scan.min_points),
                                              scan.dips_only, k=peaks, by_prominence=by_prominence, want_power=want_power,
                                              device=scan.device, devices=_batch_slots(scan.devices))
    return _with_peaks(BLSBatch(start, step, stop, p_offsets, scan.n_bins, rows, best, None), table, by_prominence)


def _string_batch(scan, signals, peaks, by_prominence, want_power):
    """The batch of :class:`StringLength` (``pdc_stringlength_scan_ragged``): every curve scaled as the single call
    scales it (``_quarter_scaled``) and scanned on exactly the grid ``_string_periods`` gives it."""
    peaks = _batch_request(peaks, want_power)
    coerced = []
    for b, s in enumerate(signals):
        try:
            coerced.append(_coerce(s))
        except IndexError:   # (an empty series has no baseline)
            raise ValueError(f"curve {b} has no samples: StringLength cannot scale an empty curve") from None
    signals = coerced
    if not signals:
        raise ValueError("StringLength.batch needs at least one signal")
    count = operator.index(scan.n_periods)
    if count < 0:
        raise ValueError(f"Number of samples, {count}, must be non-negative.")
    values = [np.asarray(s.values, dtype=float) for s in signals]
    sizes = np.array([v.size for v in values], dtype=np.int64)
    if (sizes == 0).any():
        b = int(np.argmax(sizes == 0))
        raise ValueError(f"curve {b} has no samples: StringLength cannot scale an empty curve")
    offsets = _batch_offsets(sizes)
    x = np.concatenate(values)
    # _quarter_scaled for every curve at once: np.nanmax / np.nanmin are np.fmax / np.fmin reductions
    top = np.repeat(np.fmax.reduceat(x, offsets[:-1]), sizes)
    bottom = np.repeat(np.fmin.reduceat(x, offsets[:-1]), sizes)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = (x - top) / (2 * (top - bottom)) + 0.25
    t = np.concatenate([np.asarray(s.time, dtype=float) for s in signals])
    baselines = np.array([s.baseline for s in signals], dtype=np.float64)
    start, step, stop = _string_grid(baselines, scan.dphi, count)
    if peaks:
        ok = (count <= 1) | (np.isfinite(stop) & (stop > 0))
        if not ok.all():
            b = int(np.flatnonzero(~ok)[0])
            raise ValueError(f"curve {b}: a peak table needs a frequency step dphi / baseline that is finite and "
                             f"positive (got {stop[b]!r})")
    p_offsets = np.arange(len(signals) + 1, dtype=np.int64) * count
    out, table = _cabi.stringlength_scan_ragged(t, m, offsets, start, step, stop, p_offsets, k=peaks,
                                                by_prominence=by_prominence, want_power=want_power,
                                                device=scan.device, devices=_batch_slots(scan.devices))
    return _with_peaks(StringLengthBatch(start, step, stop, p_offsets, out, None), table, by_prominence)


_KINDS = {"pdm": 0, "aov": 1, "ce": 2}
_CELL_SAMPLES = 65280   # conditional entropy: a workgroup bins a whole curve in 16-bit cells


def _phase_batch(scan, kind, signals, nb, nc, peaks, by_prominence, want_power, subharmonic=False):
    """The batch of :class:`PDM` / :class:`AOV` / :class:`ConditionalEntropy` (``pdc_phase_scan_ragged``): every
    curve on exactly the grid its own single call would scan, with that call's host-side inputs (``sigma``, the
    magnitude bins, the sub-harmonic threshold) computed the same way, per curve, and uploaded."""
    code = _KINDS[kind]
    peaks = _batch_request(peaks, want_power)
    signals = [_coerce(s) for s in signals]
    if not signals:
        raise ValueError(f"{type(scan).__name__}.batch needs at least one signal")
    values = [np.asarray(s.values, dtype=float) for s in signals]
    sizes = np.array([v.size for v in values], dtype=np.int64)
    if code == 2 and sizes.max() > _CELL_SAMPLES:
        b = int(np.argmax(sizes > _CELL_SAMPLES))
        raise ValueError(f"curve {b} has {sizes[b]} samples: ConditionalEntropy.batch bins a whole curve in one "
                         f"workgroup of 16-bit cells, at most {_CELL_SAMPLES} samples")
    start, step, stop, p_offsets = _period_grids(scan, signals, peaks)
    significant = None
    if subharmonic:
        count = np.diff(p_offsets)
        if (count < 2).any():
            b = int(np.argmax(count < 2))
            raise ValueError(f"curve {b}: sub-harmonic averaging needs at least two trial periods (got {count[b]})")
        significant = np.array([1.0 - 11.0 / s.size ** 0.8 for s in signals], dtype=np.float64)
    offsets = _batch_offsets(sizes)
    t = np.concatenate([np.asarray(s.time, dtype=float) for s in signals])
    x = np.concatenate(values)
    sigma = None
    if code == 0:
        sigma = np.array([np.var(s.values, ddof=1) for s in signals], dtype=np.float64)
    elif code == 2:
        # ConditionalEntropy.__call__'s magnitude bins, for all curves at once (nanmin / nanmax are fmin / fmax)
        low = np.repeat(np.fmin.reduceat(x, offsets[:-1]), sizes)
        high = np.repeat(np.fmax.reduceat(x, offsets[:-1]), sizes)
        with np.errstate(invalid="ignore", divide="ignore"):
            unit = (x - low) / (high - low)
            x = np.minimum(np.floor(unit * nc), nc - 1).astype(float)
            ok = (x >= 0) & (x < nc)
        if not ok.all():
            b = int(np.searchsorted(offsets, np.argmin(ok), side="right") - 1)
            raise ValueError(f"curve {b}: magnitude bins must lie in 0 .. n_mag-1 (a constant curve, or NaN values)")
    out, table = _cabi.phase_scan_ragged(code, t, x, offsets, start, step, stop, p_offsets, nb, nc, sigma=sigma,
                                         significant=significant, k=peaks, by_prominence=by_prominence,
                                         want_power=want_power, device=scan.device, devices=_batch_slots(scan.devices))
    return _with_peaks(PhaseBatch(start, step, stop, p_offsets, out, None), table, by_prominence)


_BATCH_DOC = """Periodograms of many light curves, each on the grid its own data give (``{grid}`` per curve), in
        one set of launches (``{entry}_scan_ragged`` / ``{entry}_ragged_peaks``): what a loop of ``{cls}(...)(s)``
        followed by ``{find}()`` gives, without a launch per curve.  Returns a :class:`{result}`.

        peaks: int, keyword-only
            ``k > 0`` (<= 1024): also the ``k`` {what} of every periodogram, found on the device
            (``PhaseBatch.peaks``; ``height`` holds the statistic itself).
        by_prominence: bool, keyword-only
            Rank them by prominence instead.
        want_power: bool, keyword-only
            ``False``: the periodograms stay on the device (``periodograms`` is None); needs ``peaks > 0``.

        With ``devices=(...)`` the curves are dealt to those device slots in contiguous groups balanced by
        ``sum n_b P_b``.  The object's own attributes (``periods``, ``periodogram`` ...) are left as they were."""
_PHASE_DOC = dict(grid="_pdm_periods", entry="pdc_phase", result="PhaseBatch")
_DIPS, _PEAKS = "deepest (``find_dips``) minima", "highest (``find_peaks``) maxima"


def _average_with_double_period(thetas, periods, n_samples, shortest, longest):
    """Sub-harmonic averaging (``phase.py:166,181,188-193``): wherever theta is significant
    (below ``1 - 11 / N**0.8``) and the doubled period is still on the grid, replace theta by the
    mean of itself and the value at twice the period.  All reads use the pre-update values."""
    significant = 1.0 - 11.0 / n_samples ** 0.8
    spacing = periods[1] - periods[0]
    (here,) = np.where((thetas < significant) & (periods <= longest / 2))
    doubled = np.round(2 * here + shortest / spacing).astype(int)
    thetas[here] = (thetas[here] + thetas[doubled]) / 2
    return thetas


class StringLength(object):
    """String Length period search (Dworetsky 1983, MNRAS 203, 917).

    dphi: float
        Frequency step in units of ``1 / baseline`` (0.1 by default).
    n_periods: int
        How many trial periods (1000 by default).
    cores: int, optional
        Ignored on the GPU; clamped to the host's core count exactly like upstream
        (``phase.py:41-43``) so that code reading ``.cores`` keeps working.
    device: int, keyword-only
        GPU ordinal.
    devices: sequence of int, keyword-only
        Several GPUs of this node: the period grid is cut into one contiguous slab per entry —
        the GPU counterpart of upstream's ``Pool(cores)`` fan-out (``phase.py:69-70``).
    """

    def __init__(self, dphi=0.1, n_periods=1000, cores=None, *, device=None, devices=None):
        self.dphi = dphi
        self.n_periods = n_periods
        self.cores = MAX_CORES if cores is None or cores > MAX_CORES else cores
        self.device = device
        self.devices = None if devices is None else tuple(devices)

    def _stringlength(self, period):
        """Length of the closed (phase, magnitude) polygon at one trial period — the seam of
        ``phase.py:45-51`` — evaluated by the same kernel as the full scan."""
        lengths = _cabi.stringlength_scan(self.m.time, self.m.values, [period], device=self.device)
        return float(lengths[0])

    def __call__(self, signal):
        """Scan ``n_periods`` trial periods (``phase.py:53-72``).

        The upstream call cannot run at HEAD (it hands a list to ``FSeries`` and subtracts
        misaligned one-element series — SURVEY.md fact 4); this does what its comments say:
        scale the signal to [-0.25, +0.25], fold at each period, sort by phase, sum the closed
        polygon.  Returned on ascending frequency like every ``FSeries``.
        """
        signal = _coerce(signal)
        self.signal = signal
        times = np.asarray(signal.time, dtype=float)
        self.m = TSeries(times, _quarter_scaled(np.asarray(signal.values, dtype=float)),
                         assume_sorted=True)
        periods = _string_periods(signal.baseline, self.dphi, self.n_periods)
        lengths = _cabi.stringlength_scan(times, self.m.values, periods, device=self.device,
                                          devices=self.devices)
        self.periodogram = FSeries(1 / periods, lengths)
        return self.periodogram

    def batch(self, signals, *, peaks=0, by_prominence=False, want_power=True):
        return _string_batch(self, signals, peaks, by_prominence, want_power)

    batch.__doc__ = _BATCH_DOC.format(cls="StringLength", find="find_dips", what=_DIPS, grid="_string_periods",
                                      entry="pdc_stringlength", result="StringLengthBatch")


class PDM(object):
    """Phase Dispersion Minimization (Stellingwerf 1978, ApJ 224, 953; Stellingwerf 2011).

    nb, nc: int
        Bins per cover and number of covers (5 and 2 by default): every sample falls in ``nc``
        overlapping bins of width ``1 / nb``.
    p_min, p_max: float, optional
        Shortest / longest trial period; by default twice the median sampling step and
        ``oversample`` times the baseline.
    n_periods: int or None
        Number of trial periods (1000 by default; ``None`` derives it from the frequency range).
    oversample: scalar
        See ``p_max``.
    do_subharmonic: bool
        Average theta at each significant period with theta at twice that period: a real
        variation shows at both, noise does not.
    cores: int, optional
        Stored but unused on the GPU.
    device: int, keyword-only
        GPU ordinal.
    devices: sequence of int, keyword-only
        Several GPUs of this node, one contiguous slab of the period grid each (upstream's
        ``Pool(cores)``, ``phase.py:182-186``).
    """

    def __init__(self, nb=5, nc=2, p_min=None, p_max=None, n_periods=1000, oversample=1,
                 do_subharmonic=False, cores=None, *, device=None, devices=None):
        self.nb, self.nc = nb, nc
        self.p_min, self.p_max = p_min, p_max
        self.n_periods = n_periods
        self.oversample = oversample
        self.do_subharmonic = do_subharmonic
        self.cores = cores
        self.device = device
        self.devices = None if devices is None else tuple(devices)

    def _scan(self, periods):
        return _cabi.pdm_scan(self.t, self.x, periods, self.nb, self.nc, self.sigma,
                              device=self.device, devices=self.devices)

    def _pdm(self, period):
        """Stellingwerf's theta at one trial period — the seam of ``phase.py:128-149``."""
        return float(self._scan([period])[0])

    def __call__(self, signal):
        """theta (Eq. 3 of the 1978 paper) on the trial-period grid (``phase.py:151-195``)."""
        signal = _coerce(signal)
        self.signal = signal
        self.t = np.asarray(signal.time, dtype=float)
        self.x = np.asarray(signal.values, dtype=float)
        self.sigma = np.var(signal.values, ddof=1)
        self.periods, shortest, longest = _pdm_periods(signal, self.p_min, self.p_max,
                                                       self.n_periods, self.oversample)
        thetas = self._scan(self.periods)
        if self.do_subharmonic:
            thetas = _average_with_double_period(thetas, self.periods, signal.size, shortest, longest)
        self.periodogram = FSeries(1 / self.periods, thetas)
        return self.periodogram

    def batch(self, signals, *, peaks=0, by_prominence=False, want_power=True):
        return _phase_batch(self, "pdm", signals, self.nb, self.nc, peaks, by_prominence, want_power,
                            subharmonic=self.do_subharmonic)

    batch.__doc__ = _BATCH_DOC.format(cls="PDM", find="find_dips", what=_DIPS, **_PHASE_DOC)


class AOV(object):
    """Analysis of Variance period search (Schwarzenberg-Czerny 1989) - one of the scans the
    reference lists as TODO (``phase.py:11``), shaped like :class:`PDM` and computed by the same
    binning kernel (``csrc/pdm.hip``): the statistic is large where the folded curve is coherent.

    Parameters
    ----------
    n_bins: int, optional
        Number of phase bins r (the default is 10).
    p_min, p_max, n_periods, oversample, cores:
        The trial-period grid, exactly as for :class:`PDM` (``phase.py:167-180``).
    device: int, keyword-only
        GPU ordinal.
    devices: sequence of int, keyword-only
        Several GPUs of this node, one contiguous slab of the period grid each.
    """

    def __init__(self, n_bins=10, p_min=None, p_max=None, n_periods=1000, oversample=1, cores=None,
                 *, device=None, devices=None):
        self.n_bins = n_bins
        self.p_min, self.p_max = p_min, p_max
        self.n_periods = n_periods
        self.oversample = oversample
        self.cores = cores
        self.device = device
        self.devices = None if devices is None else tuple(devices)

    def __call__(self, signal):
        signal = _coerce(signal)
        self.signal = signal
        self.t = np.asarray(signal.time, dtype=float)
        self.x = np.asarray(signal.values, dtype=float)
        self.periods, _, _ = _pdm_periods(signal, self.p_min, self.p_max, self.n_periods,
                                          self.oversample)
        theta = _cabi.aov_scan(self.t, self.x, self.periods, self.n_bins, device=self.device,
                               devices=self.devices)
        self.periodogram = FSeries(1 / self.periods, theta)
        return self.periodogram

    def batch(self, signals, *, peaks=0, by_prominence=False, want_power=True):
        return _phase_batch(self, "aov", signals, self.n_bins, 1, peaks, by_prominence, want_power)

    batch.__doc__ = _BATCH_DOC.format(cls="AOV", find="find_peaks", what=_PEAKS, **_PHASE_DOC)


class SuperSmoother(object):
    """Supersmoother period search - the reference only names it (``spectral.py:8``: "TODO: check out
    Supersmoother (Reimann 1994)"); shaped like :class:`PDM`.  Per trial period the curve is folded and sorted by
    phase, Friedman's variable span smoother (Friedman 1984: three running-lines smooths with spans 0.05 / 0.2 /
    0.5 of the curve, periodic in phase, the span chosen per point by leave-one-out residuals) is fitted to it,
    and the periodogram is the mean absolute residual about that fit (Reimann 1994): minimal at the period.

    Parameters
    ----------
    alpha: float, optional
        Friedman's bass control in [0, 10]: larger values pull the chosen spans towards the widest one
        (smoother fits); 0 (the default) switches it off.
    p_min, p_max, n_periods, oversample, cores:
        The trial-period grid, exactly as for :class:`PDM` (``phase.py:167-180``).
    device / devices: keyword-only
        GPU ordinal / several GPUs of this node, one contiguous slab of the period grid each.
    """

    def __init__(self, alpha=0.0, p_min=None, p_max=None, n_periods=1000, oversample=1, cores=None,
                 *, device=None, devices=None):
        self.alpha = alpha
        self.p_min, self.p_max = p_min, p_max
        self.n_periods = n_periods
        self.oversample = oversample
        self.cores = cores
        self.device = device
        self.devices = None if devices is None else tuple(devices)

    def __call__(self, signal):
        signal = _coerce(signal)
        self.signal = signal
        self.t = np.asarray(signal.time, dtype=float)
        self.x = np.asarray(signal.values, dtype=float)
        self.periods, _, _ = _pdm_periods(signal, self.p_min, self.p_max, self.n_periods,
                                          self.oversample)
        stat = _cabi.supersmoother_scan(self.t, self.x, self.periods, self.alpha, device=self.device,
                                        devices=self.devices)
        self.periodogram = FSeries(1 / self.periods, stat)
        return self.periodogram


class ConditionalEntropy(object):
    """Conditional-entropy period search (Graham et al. 2013) - TODO upstream (``phase.py:15``),
    shaped like :class:`PDM`: the entropy of the magnitudes given the phase, over an
    ``n_phase x n_mag`` partition of the folded, unit-normalised light curve; minimal at the period.

    Parameters
    ----------
    n_phase, n_mag: int, optional
        Phase and magnitude bins (defaults 10 and 5).
    p_min, p_max, n_periods, oversample, cores:
        The trial-period grid, exactly as for :class:`PDM`.
    device: int, keyword-only
        GPU ordinal.
    devices: sequence of int, keyword-only
        Several GPUs of this node, one contiguous slab of the period grid each.
    """

    def __init__(self, n_phase=10, n_mag=5, p_min=None, p_max=None, n_periods=1000, oversample=1,
                 cores=None, *, device=None, devices=None):
        self.n_phase, self.n_mag = n_phase, n_mag
        self.p_min, self.p_max = p_min, p_max
        self.n_periods = n_periods
        self.oversample = oversample
        self.cores = cores
        self.device = device
        self.devices = None if devices is None else tuple(devices)

    def __call__(self, signal):
        signal = _coerce(signal)
        self.signal = signal
        self.t = np.asarray(signal.time, dtype=float)
        values = np.asarray(signal.values, dtype=float)
        low, high = np.nanmin(values), np.nanmax(values)
        unit = (values - low) / (high - low)
        self.mag_bin = np.minimum(np.floor(unit * self.n_mag), self.n_mag - 1).astype(float)
        self.periods, _, _ = _pdm_periods(signal, self.p_min, self.p_max, self.n_periods,
                                          self.oversample)
        entropy = _cabi.cond_entropy_scan(self.t, self.mag_bin, self.periods, self.n_phase, self.n_mag,
                                          device=self.device, devices=self.devices)
        self.periodogram = FSeries(1 / self.periods, entropy)
        return self.periodogram

    def batch(self, signals, *, peaks=0, by_prominence=False, want_power=True):
        return _phase_batch(self, "ce", signals, self.n_phase, self.n_mag, peaks, by_prominence, want_power)

    batch.__doc__ = _BATCH_DOC.format(cls="ConditionalEntropy", find="find_dips", what=_DIPS, **_PHASE_DOC)


class GregoryLoredo(object):
    """Gregory-Loredo period search (Gregory & Loredo 1992, ApJ 398, 146) - the third scan the reference
    lists as TODO (``phase.py:13``), shaped like :class:`PDM`.  It works on ARRIVAL TIMES: the time stamps of
    ``signal`` are the events, its values are not used.  Model ``M_m`` is a periodic rate that is constant
    in each of ``m`` phase bins; per trial frequency the data enter through the multiplicity of the bin
    counts, ``W_m = N! / (n_1! ... n_m!)``, marginalised over the unknown offset of the bins (their eq.
    5.13-5.14).  The periodogram returned is the log of the per-frequency odds in favour of a periodic
    signal, ``ln sum_{m=2}^{m_max} O_m1(w) / (m_max - 1)`` with
    ``O_m1(w) = N! (m-1)! / (N+m-1)! * <m^N / W_m(w, phi)>_phi`` (the integrand of eq. 5.28; equal prior
    odds for every ``m``); it peaks at the period.  ``.log_s[m]`` keeps ``ln <m^N / W_m>`` per ``m``.

    Parameters
    ----------
    m_max: int, optional
        Largest number of phase bins (the default is 12, as in the paper); ``m`` runs over 2 .. m_max.
    n_offsets: int, optional
        Shifts of the bin boundaries the offset integral is averaged over (the default is 8);
        ``m_max * n_offsets`` must not exceed 190.
    p_min, p_max, n_periods, oversample, cores:
        The trial-period grid, exactly as for :class:`PDM` (``phase.py:167-180``).
    device / devices: keyword-only
        GPU ordinal / several GPUs of this node, one contiguous slab of the period grid each.
    """

    def __init__(self, m_max=12, n_offsets=8, p_min=None, p_max=None, n_periods=1000, oversample=1, cores=None,
                 *, device=None, devices=None):
        self.m_max, self.n_offsets = m_max, n_offsets
        self.p_min, self.p_max = p_min, p_max
        self.n_periods = n_periods
        self.oversample = oversample
        self.cores = cores
        self.device = device
        self.devices = None if devices is None else tuple(devices)

    def __call__(self, signal):
        from scipy.special import gammaln, logsumexp
        signal = _coerce(signal)
        self.signal = signal
        self.t = np.asarray(signal.time, dtype=float)
        self.periods, _, _ = _pdm_periods(signal, self.p_min, self.p_max, self.n_periods, self.oversample)
        n = int(np.sum(np.isfinite(self.t)))
        self.log_s, terms = {}, []
        for m in range(2, self.m_max + 1):
            self.log_s[m] = _cabi.gl_scan(self.t, self.periods, m, self.n_offsets, device=self.device,
                                          devices=self.devices)
            # ln [N! (m-1)! / (N+m-1)!]: the prior volume of the m bin heights
            terms.append(self.log_s[m] + gammaln(n + 1) + gammaln(m) - gammaln(n + m))
        log_odds = logsumexp(np.array(terms), axis=0) - np.log(self.m_max - 1)
        self.periodogram = FSeries(1 / self.periods, log_odds)
        return self.periodogram


class BLS(object):
    """Box least squares transit search (Kovacs, Zucker & Mazeh 2002, A&A 391, 369), shaped like :class:`AOV`: the
    scan for a box-shaped dip - a planetary transit, a detached eclipse - that is flat for most of the phase and low
    for the rest.  The reference has no such class - **parity unpinned by the reference**.

    Weights and centring are those of ``GLS``: ``w = err**-2 / sum(err**-2)``, ``y' = y - sum(w y)``,
    ``YY = sum(w y'**2)``.  Per trial period the samples are folded (``(t / P) % 1``, no time origin) into ``n_bins``
    phase bins; a box is a start bin and a length of ``len_min .. len_max`` bins, wrapping past phase 1, with
    ``r = sum w``, ``s = sum w y'`` and ``c`` samples inside.  Over the boxes with at least ``min_points`` samples
    inside and outside (``dips_only``: and ``s < 0``),

        ``power(P) = max s**2 / (r (1 - r)) / YY``,

    the share of the weighted variance the best two-level model removes (in [0, 1], like the normalised GLS power),
    and ``depth = -s / (r (1 - r))`` is the out-of-box level minus the in-box level of that box.  Evaluated by
    ``csrc/bls.hip`` in 64-bit fixed point (bit-identical from call to call); nothing here computes a periodogram on
    the CPU.

    Parameters
    ----------
    n_bins: int, optional
        Phase bins, 2 .. 2048 (the default is 200).
    q_min, q_max: float, optional
        Shortest and longest box as a fraction of the period, ``0 < q_min <= q_max < 1`` (defaults 0.01 and 0.1):
        ``len_min = max(1, floor(q_min n_bins))``, ``len_max = min(n_bins - 1, max(len_min, ceil(q_max n_bins)))``.
    p_min, p_max, n_periods, oversample, cores:
        The trial-period grid, exactly as for :class:`PDM` (``phase.py:167-180``).
    min_points: int, optional
        Samples a box must have inside and leave outside (the default is 5).
    dips_only: bool, optional
        Only boxes below the out-of-box level.
    device: int, keyword-only
        GPU ordinal.

    After a call: ``.signal .t .x .err .periods .periodogram`` and, aligned with ``.periods``, ``.power .depth
    .duration .transit_time`` (mid-box time modulo the period) ``.start_bin .box_bins`` - NaN where a period has no
    admissible box - and ``.best``, the ``period, power, depth, duration, transit_time`` at the highest power.
    """

    MAX_BINS = 2048

    def __init__(self, n_bins=200, q_min=0.01, q_max=0.1, p_min=None, p_max=None, n_periods=1000, oversample=1,
                 min_points=5, dips_only=False, cores=None, *, device=None):
        self.n_bins = n_bins
        self.q_min, self.q_max = q_min, q_max
        self.p_min, self.p_max = p_min, p_max
        self.n_periods = n_periods
        self.oversample = oversample
        self.min_points = min_points
        self.dips_only = bool(dips_only)
        self.cores = cores
        self.device = device
        self.devices = None   # device slots of batch(): an attribute, set after construction (a GPU may repeat)
        self.box_lengths()

    def box_lengths(self):
        """``(len_min, len_max)`` in bins; raises ``ValueError`` for parameters the scan does not take."""
        for name in ("n_bins", "min_points"):
            v = getattr(self, name)
            if isinstance(v, bool) or v != int(v):
                raise ValueError(f"{name} must be an integer")
        if not 2 <= int(self.n_bins) <= self.MAX_BINS:
            raise ValueError(f"n_bins must be 2 .. {self.MAX_BINS}")
        if int(self.min_points) < 1:
            raise ValueError("min_points must be at least 1")
        if not 0 < self.q_min <= self.q_max < 1:
            raise ValueError("box fractions need 0 < q_min <= q_max < 1")
        n_bins = int(self.n_bins)
        len_min = max(1, int(np.floor(self.q_min * n_bins)))
        len_max = min(n_bins - 1, max(len_min, int(np.ceil(self.q_max * n_bins))))
        if not 1 <= len_min <= len_max <= n_bins - 1:
            raise ValueError("box lengths need 1 <= len_min <= len_max <= n_bins - 1")
        return len_min, len_max

    def __call__(self, signal, err=None):
        len_min, len_max = self.box_lengths()
        signal = _coerce(signal)
        t = np.asarray(signal.time, dtype=float)
        x = np.asarray(signal.values, dtype=float)
        have_err = err is not None
        err = np.asarray(err, dtype=float) if have_err else np.ones_like(x)
        if err.shape != x.shape:
            raise ValueError("Input arrays have incompatible lengths.")
        periods, _, _ = _pdm_periods(signal, self.p_min, self.p_max, self.n_periods, self.oversample)
        n_bins = int(self.n_bins)
        power, depth, start, box = _cabi.bls_scan(t, x, err if have_err else None, periods, n_bins, len_min, len_max,
                                                  int(self.min_points), self.dips_only, device=self.device)
        self.signal, self.t, self.x, self.err, self.periods = signal, t, x, err, periods
        found = start >= 0
        self.power, self.depth = power, depth
        self.start_bin = np.where(found, start, np.nan)
        self.box_bins = np.where(found, box, np.nan)
        self.duration = self.box_bins / n_bins * periods
        self.transit_time = ((self.start_bin + self.box_bins / 2) / n_bins % 1) * periods
        j = int(np.nanargmax(power)) if np.any(~np.isnan(power)) else None
        self.best = {name: (float("nan") if j is None else float(values[j])) for name, values in
                     (("period", periods), ("power", power), ("depth", depth), ("duration", self.duration),
                      ("transit_time", self.transit_time))}
        self.periodogram = FSeries(1 / periods, power)
        return self.periodogram

    def batch(self, signals, errs=None, *, peaks=0, by_prominence=False, want_power=True):
        """Box searches of many light curves, each on the grid its own data give (``_pdm_periods`` per curve), in one
        set of launches (``pdc_bls_scan_ragged`` / ``pdc_bls_ragged_peaks``): what a loop of ``BLS(...)(s, e)`` gives,
        bit for bit, without a launch per curve.  Returns a :class:`BLSBatch`; its ``best`` (one line per curve:
        period, power, depth, duration, transit time of the highest power) is found on the device.

        errs: None, or a sequence (one entry per signal) of arrays or Nones (ones)
        peaks: int, keyword-only
            ``k > 0`` (<= 1024): also the ``k`` highest (``find_peaks``) maxima of every power row, found on the
            device (``BLSBatch.peaks``).
        by_prominence: bool, keyword-only
            Rank them by prominence instead.
        want_power: bool, keyword-only
            ``False``: the four per-period rows stay on the device (``periodograms``, ``power`` ... are None); ``best``
            and the peak table are still returned.

        ``n_bins``, the box lengths, ``min_points`` and ``dips_only`` are the object's, shared by all curves.  With the
        attribute ``devices`` set (``scan.devices = (0, 1)``; the constructor's parameter list is unchanged) the curves
        are dealt to those device slots in contiguous groups balanced by ``sum n_b P_b``; else they run on ``device``.
        A curve without samples has no grid of its own: its rows are empty and its ``best`` entries are -1 / NaN.
        The object's own attributes (``periods``, ``periodogram`` ...) are left as they were."""
        return _bls_batch(self, signals, errs, peaks, by_prominence, want_power)
