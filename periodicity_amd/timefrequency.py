"""Time-frequency analysis of unevenly sampled curves, computed on MI355X.

``WWZ`` is Foster's weighted wavelet Z-transform (Foster 1996, AJ 112, 1709): at every time shift ``tau`` and trial
frequency ``f`` the weighted least-squares fit of a constant plus a sinusoid under the Gaussian window
``exp(-c (2 pi f)^2 (t - tau)^2)``, whose width scales with the period - for curves whose period moves during the
observation (migrating spots, semiregular and Mira variables, mode switching, drifting QPOs).  The reference's
``timefrequency.WPS`` needs an evenly sampled series and is not ported; WWZ is not in the reference at all -
**parity unpinned by the reference**.  The definitions are in ``include/periodicity_hip.h``; the statistic is
evaluated by ``csrc/wwz.hip``.  Nothing in this module computes it on the CPU.
"""
import collections as _collections
import copy as _copy

import numpy as np

from . import _cabi
from .spectral import GLS, _as_tseries

__all__ = ["WWZ", "WWZMap", "BestWWZ"]

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
