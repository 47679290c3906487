"""Time-frequency analysis of sampled curves, computed on MI355X.

``WPS`` is the reference's Morlet wavelet power spectrum of an EVENLY sampled curve: PyWavelets' published ``cwt``
algorithm restated as an exact gather-sum (``csrc/wps.hip``), the plane kept on the device where only its marginals are
read - **parity unpinned by the reference** (PyWavelets is not a dependency; two assumptions).

``WWZ`` is Foster's weighted wavelet Z-transform (Foster 1996, AJ 112, 1709): at every time shift ``tau`` and trial
frequency ``f`` the weighted least-squares fit of a constant plus a sinusoid under the Gaussian window
``exp(-c (2 pi f)^2 (t - tau)^2)``, whose width scales with the period - for curves whose period moves during the
observation (migrating spots, semiregular and Mira variables, mode switching, drifting QPOs).  WWZ is not in the
reference at all - **parity unpinned by the reference**.  The definitions are in ``include/periodicity_hip.h``; the
statistic is evaluated by ``csrc/wwz.hip``.  Nothing in this module computes either statistic on the CPU; ``HHT`` and
``CompositeSpectrum`` are not ported.
"""
import collections as _collections
import copy as _copy
import warnings as _warnings

import numpy as np

from . import _cabi
from .core import FSeries, TFSeries, TSeries
from .spectral import GLS, _as_tseries

__all__ = ["WWZ", "WWZMap", "BestWWZ", "WPS", "cmor_table"]

BestWWZ = _collections.namedtuple("BestWWZ", ["tau", "frequency", "wwz", "amplitude"])


class WWZMap(object):
    """What ``WWZ.__call__`` returns: the transform over time shift x frequency, reduced on the device.

    ``.frequency`` ``[nf]``, ``.tau`` ``[ntau]``; ``.wwz``, ``.amplitude`` (WWA) and ``.neff`` ``[ntau][nf]``, None
    without ``want_planes``; per time shift the cell of the largest WWZ among those with ``neff >= min_neff``, as
    ``np.nanargmax(np.where(neff >= min_neff, wwz, nan), axis=1)`` picks it: ``.ridge_bin`` (-1 where no cell is
    eligible), ``.ridge_frequency``, ``.ridge_period`` (NaN there), ``.ridge_wwz``, ``.ridge_amplitude``; ``.best``,
    the largest ridge cell as a ``BestWWZ(tau, frequency, wwz, amplitude)`` - NaN where no row has one; ``.visited``,
    the samples inside the support cut summed over all (tile, tau).
    """

    def __init__(self, frequency, tau, out):
        self.frequency = frequency
        self.tau = tau
        self.wwz = out["wwz"]
        self.amplitude = out["amp"]
        self.neff = out["neff"]
        self.ridge_bin = out["ridge_bin"]
        found = self.ridge_bin >= 0
        self.ridge_frequency = np.where(found, frequency[np.maximum(self.ridge_bin, 0)], np.nan)
        with np.errstate(divide="ignore"):
            self.ridge_period = 1.0 / self.ridge_frequency
        self.ridge_wwz = out["ridge_wwz"]
        self.ridge_amplitude = out["ridge_amp"]
        value, row, j = out["best"]
        if row >= 0:
            self.best = BestWWZ(float(tau[row]), float(frequency[j]), value, float(self.ridge_amplitude[row]))
        else:
            self.best = BestWWZ(np.nan, np.nan, value, np.nan)
        self.visited = out["visited"]


class WWZ(object):
    """Weighted wavelet Z-transform of a discrete, unevenly sampled signal.

    Parameters
    ----------
    fmin, fmax, n: as ``GLS`` - the frequency grid follows its rule.
    decay: float, keyword-only, optional
        The window's decay constant ``c`` (default Foster's ``1 / (8 pi^2)``); larger: shorter windows, better time
        resolution, worse frequency resolution.
    min_neff: float, keyword-only, optional
        Cells with fewer effective samples than this (default 6) are not eligible for the ridge and the best cell.
        The planes hold every cell.
    device: int, keyword-only, optional
    """

    def __init__(self, fmin=None, fmax=None, n=5, *, decay=1 / (8 * np.pi ** 2), min_neff=6.0, device=None):
        decay, min_neff = float(decay), float(min_neff)
        if not (np.isfinite(decay) and decay > 0):
            raise ValueError("decay must be finite and positive.")
        if not np.isfinite(min_neff):
            raise ValueError("min_neff must be finite.")
        self.fmin = fmin
        self.fmax = fmax
        self.n = n
        self.decay = decay
        self.min_neff = min_neff
        self.device = device

    def _grid(self, signal):
        """The grid of ``GLS._grid``."""
        return GLS(self.fmin, self.fmax, self.n)._grid(signal)

    def __call__(self, signal, err=None, taus=64, want_planes=True):
        """The transform of ``signal`` (times in ascending order) as a ``WWZMap``.

        err: array-like, optional
            Measurement uncertainties for each sample.
        taus: int or array-like
            The time shifts: an array of finite values, or their number on ``np.linspace(t[0], t[-1], taus)``.
        want_planes: False leaves the three planes on the device: ridge and best cell only.
        """
        signal = _as_tseries(signal)
        t = np.asarray(signal.time, dtype=float)
        y = np.asarray(signal.values, dtype=float)
        if t.ndim != 1 or t.size < 4:
            raise ValueError("At least four samples are needed.")
        if np.any(np.diff(t) < 0) or not np.all(np.isfinite(t)):
            raise ValueError("The times must be finite and in ascending order.")
        dy = None
        if err is not None:
            dy = np.asarray(err, dtype=float)
            if dy.ndim != 1 or dy.size != t.size:
                raise ValueError("Input arrays have incompatible lengths.")
        if isinstance(taus, (int, np.integer)) and not isinstance(taus, bool):
            if taus < 1:
                raise ValueError("taus must be at least 1.")
            tau = np.linspace(t[0], t[-1], int(taus))
        else:
            tau = np.array(taus, dtype=float)
            if tau.ndim != 1 or tau.size < 1:
                raise ValueError("taus must be an integer or a one-dimensional array with at least one entry.")
            if not np.all(np.isfinite(tau)):
                raise ValueError("taus must be finite.")
        self.frequency = self._grid(signal)
        f0, delta, nf = _cabi.grid_params(self.frequency)
        if nf < 2:   # a grid of one bin has no step of its own; any positive step rebuilds it
            delta = 1.0
        out = _cabi.wwz_scan(t, y, dy, f0, delta, nf, tau, self.decay, self.min_neff, want_planes=bool(want_planes),
                             device=_cabi.pick_device(self.device, None))
        self.signal = signal
        self.err = err
        self.map = WWZMap(self.frequency, tau, out)
        return self.map

    def copy(self):
        return _copy.deepcopy(self)


# ---- WPS ---------------------------------------------------------------------------------------------------------------
WPS_POINTS = 1024            # the wavelet is tabulated on 2 ** precision points, precision = 10 (ASSUMED)
WPS_SUPPORT = (-8.0, 8.0)    # ... over this support (ASSUMED)
WPS_BANDWIDTH, WPS_CENTER = 2.0, 1.0   # "cmor2.0-1.0"
WPS_CENTRAL_FREQUENCY = 1.0  # scale2frequency("cmor2.0-1.0", 1) (ASSUMED)


def cmor_table():
    """``(table, step, span)``: the integrated complex Morlet wavelet "cmor2.0-1.0" as the continuous transform reads
    it - ``conj(cumsum(psi) * step)`` on ``np.linspace(-8, 8, 1024)`` - with the grid's step and width, all float64.
    The device takes these bits as they are; nothing else of the transform is computed on the host."""
    xg = np.linspace(WPS_SUPPORT[0], WPS_SUPPORT[1], WPS_POINTS)
    step = xg[1] - xg[0]
    psi = (np.pi * WPS_BANDWIDTH) ** -0.5 * np.exp(2j * np.pi * WPS_CENTER * xg) * np.exp(-xg ** 2 / WPS_BANDWIDTH)
    return np.conj(np.cumsum(psi) * step), float(step), float(xg[-1] - xg[0])


class WPS(object):
    """Wavelet power spectrum with Morlet wavelets of an evenly sampled signal (the reference's ``timefrequency.WPS``),
    evaluated by ``csrc/wps.hip``.

    The reference calls ``pywt.cwt(values - mean, scales, "cmor2.0-1.0", dt)`` with
    ``scales = scale2frequency(family, 1) * periods / median_dt``, squares and divides by the scale.  PyWavelets is not a
    dependency: its published algorithm is restated (``include/periodicity_hip.h``), with
    ``scale2frequency("cmor2.0-1.0", 1) == 1.0`` and a table of 1024 points over [-8, 8] assumed - **parity unpinned by
    the reference**.

    Parameters
    ----------
    periods: array-like
        Periods to consider, in the time units of the signal; used in the order given.
    device: int, keyword-only, optional

    After a call: ``.signal``, ``.time``, ``.scales``, ``.frequency``, ``.spectrum`` (``|coef|^2 / scale``, a
    ``TFSeries``, None without ``want_planes``), ``.masked_spectrum`` (NaN outside the cone of influence), ``.coefs``
    (complex ndarray, None without ``want_coefs``), ``.power`` (``spectrum * scales``, derived on the host each time it
    is read), ``.mask_coi``, and the marginals ``gwps()``, ``sav()``, ``masked_gwps()``, ``masked_sav()``, which
    without a range are reduced on the device and need no plane.
    """

    def __init__(self, periods, *, device=None):
        self.periods = np.array(periods, dtype=float)
        if self.periods.ndim != 1 or self.periods.size < 1:
            raise ValueError("periods must be a one-dimensional array with at least one entry.")
        if not np.all(np.isfinite(self.periods)) or np.any(self.periods <= 0):
            raise ValueError("periods must be finite and positive.")
        self.frequency = 1.0 / self.periods
        self.device = device
        self.spectrum = self.masked_spectrum = self.coefs = None

    def __call__(self, signal, want_planes=True, want_coefs=False):
        """The spectrum of ``signal`` (evenly sampled, finite) at the given periods: a ``TFSeries``
        ``[len(periods)][len(signal)]``, or None with ``want_planes=False``, which leaves the plane on the device and
        brings back the marginals only.  ``want_coefs`` also returns the complex coefficients."""
        signal = _as_tseries(signal)
        t = np.asarray(signal.time, dtype=float)
        y = np.asarray(signal.values, dtype=float)
        if t.ndim != 1 or t.size < 2:
            raise ValueError("At least two samples are needed.")
        if not (np.all(np.isfinite(y)) and np.all(np.isfinite(t))):
            raise ValueError("The signal must be finite: fill its gaps first.")
        dt = np.median(np.diff(t))
        if not dt > 0:
            raise ValueError("The times must ascend.")
        scales = WPS_CENTRAL_FREQUENCY * self.periods / dt
        table, step, span = cmor_table()
        for s in scales:
            if _cabi.wps_taps(s, step, span)[3] < 2:
                raise ValueError("Selected scale is too small: a period needs at least 1/16 of a sampling step.")
        out = _cabi.wps_scan(y - np.mean(y), t, self.periods, scales, table, step, span, np.exp2(0.5),
                             want_planes=bool(want_planes), want_coefs=bool(want_coefs),
                             device=_cabi.pick_device(self.device, None))
        self.signal = signal
        self.time = t
        self.scales = scales
        self.coefs = out["coefs"]
        self._marginals = out
        self.gwps_count, self.sav_count = out["gwps_count"], out["sav_count"]   # cells inside the cone, per period / time
        self.spectrum = self.masked_spectrum = None
        if want_planes:
            self.spectrum = TFSeries(time=t, frequency=self.frequency, values=out["spectrum"])
            self.masked_spectrum = TFSeries(time=t, frequency=self.frequency,
                                            values=np.where(self.mask_coi, out["spectrum"], np.nan))
        return self.spectrum

    @property
    def power(self):
        """``|coef|^2`` as a ``TFSeries``: ``spectrum * scales``, multiplied on the host at every read."""
        if self.spectrum is None:
            raise ValueError("power needs the plane: call with want_planes=True.")
        return TFSeries(time=self.time, frequency=self.frequency, values=self.spectrum.values * self.scales[:, None])

    @property
    def mask_coi(self):
        """True inside the cone of influence: ``sqrt(2) period < min(t - t_min, t_max - t)``."""
        corr = np.exp2(0.5)
        t_max, t_min = np.max(self.time), np.min(self.time)
        t_mesh, p_mesh = np.meshgrid(self.time, self.periods)
        return corr * p_mesh < np.minimum(t_mesh - t_min, t_max - t_mesh)

    def coi(self, coi_samples=100):
        """The cone's border as a ``TSeries`` of periods over time, ``coi_samples`` log-spaced periods a side."""
        corr = np.exp2(0.5)
        t_max, t_min = np.max(self.time), np.min(self.time)
        p = np.logspace(np.log10(np.min(self.periods)), np.log10(np.max(self.periods)), coi_samples)
        p = p[corr * p < (t_max - t_min) / 2]
        return TSeries(np.hstack((t_min + corr * p, t_max - corr * p)), np.hstack((p, p)))

    def _plane(self, masked, what):
        plane = self.masked_spectrum if masked else self.spectrum
        if plane is None:
            raise ValueError(f"{what} over a range needs the plane: call with want_planes=True.")
        return plane

    def _over_periods(self, masked, pmin, pmax, what):
        if pmin is None and pmax is None:
            return TSeries(self.time, self._marginals["masked_sav" if masked else "sav"].copy())
        keep = np.ones(self.periods.size, bool)
        if pmin is not None:
            keep &= self.periods >= pmin
        if pmax is not None:
            keep &= self.periods <= pmax
        with _warnings.catch_warnings():
            _warnings.simplefilter("ignore", category=RuntimeWarning)
            return self._plane(masked, what)[keep].mean("frequency")

    def _over_time(self, masked, tmin, tmax, what):
        if tmin is None and tmax is None:
            return FSeries(self.frequency, self._marginals["masked_gwps" if masked else "gwps"].copy())
        keep = np.ones(self.time.size, bool)
        if tmin is not None:
            keep &= self.time >= tmin
        if tmax is not None:
            keep &= self.time <= tmax
        with _warnings.catch_warnings():
            _warnings.simplefilter("ignore", category=RuntimeWarning)
            return self._plane(masked, what)[:, keep].mean("time")

    def sav(self, pmin=None, pmax=None):
        """Scale-averaged variance: the mean over the periods (in ``[pmin, pmax]``) as a ``TSeries``."""
        return self._over_periods(False, pmin, pmax, "sav")

    def masked_sav(self, pmin=None, pmax=None):
        """``sav`` over the cells inside the cone of influence; NaN where a time has none."""
        return self._over_periods(True, pmin, pmax, "masked_sav")

    def gwps(self, tmin=None, tmax=None):
        """Global wavelet power spectrum: the mean over time (in ``[tmin, tmax]``) as an ``FSeries``."""
        return self._over_time(False, tmin, tmax, "gwps")

    def masked_gwps(self, tmin=None, tmax=None):
        """``gwps`` over the cells inside the cone of influence; NaN where a period has none."""
        return self._over_time(True, tmin, tmax, "masked_gwps")
