"""Auto- and cross-correlation of unevenly sampled curves, computed on MI355X.

``DCF`` is the discrete correlation function of Edelson & Krolik (1988, ApJ 333, 646): every pair of samples is binned
by its time lag and nothing is interpolated - the standard estimator of the autocorrelation of a curve with gaps, and
of the delay between two curves (reverberation mapping, lensed quasars, optical against X-ray).  The reference's
``TSeries.acf`` (``core.py:578-608``) is an inverse FFT of the power spectrum on ``median_dt`` and is only right for
evenly sampled curves; it has no cross-correlation - **parity unpinned by the reference**.  On an evenly sampled curve
``DCF(include_self=True)`` is the reference's mask-corrected ACF.  The statistic is defined in
``include/periodicity_hip.h``; the pairs are binned and summed by ``csrc/dcf.hip``.  Nothing in this module does that
on the CPU: numpy centres the curves and turns the per-bin sums into the normalised values.
"""
import copy as _copy

import numpy as np

from . import _cabi
from .core import TSeries
from .spectral import _as_tseries

__all__ = ["DCF"]

SUMS = ("Sa", "Sb", "Saa", "Sbb", "Sab", "Sabab")


def _curve(signal, err):
    signal = _as_tseries(signal)
    t = np.asarray(signal.time, dtype=float)
    y = np.asarray(signal.values, dtype=float)
    if t.ndim != 1 or t.size < 2:
        raise ValueError("At least two samples are needed.")
    if np.any(np.diff(t) < 0) or not np.all(np.isfinite(t)):
        raise ValueError("The times must be finite and in ascending order.")
    if err is not None:
        err = np.asarray(err, dtype=float)
        if err.ndim != 1 or err.size != t.size:
            raise ValueError("Input arrays have incompatible lengths.")
    return signal, t, y, err


class DCF(object):
    """Discrete correlation function of one curve with itself, or of two curves.

    Parameters
    ----------
    max_lag: float, optional
        Centre of the last lag bin at most this; default half the baseline (of the shorter curve).
    dlag: float, optional
        Width of a lag bin; default ``median_dt`` (the larger of the two curves').
    min_lag: float, optional
        Centre of the first lag bin; default 0 for one curve and ``-max_lag`` for two.
    normalization: {"global", "local"}
        ``"global"`` (Edelson & Krolik): ``Sab / (n norm)`` with ``norm = sqrt((var_a - mean(err_a^2)) (var_b -
        mean(err_b^2)))`` of the whole curves (population variances), ``sigma = sqrt(max(Sabab / norm^2 - n dcf^2, 0))
        / (n - 1)``.  ``"local"`` (Lehar et al. 1992; White & Peterson 1994): Pearson's r of the bin's own pairs,
        ``sigma = (1 - r^2) / sqrt(n - 1)``; uncertainties are not used.
    min_pairs: int
        Bins with fewer pairs (at least 2) are NaN.
    include_self: bool
        One curve: also count the pairs of a sample with itself (lag 0).
    device: int, keyword-only, optional

    A call sets ``.signal``, ``.other``, ``.lags`` (bin centres ``min_lag + dlag arange(nlag)``), ``.edges``
    (``(min_lag - dlag / 2) + dlag arange(nlag + 1)``; bin k holds ``edges[k] <= lag < edges[k+1]``), ``.pairs``, ``.sums``
    (a dict of the six per-bin sums Sa, Sb, Saa, Sbb, Sab, Sabab of the centred curves), ``.dcf``, ``.sigma`` and
    ``.correlogram``, the returned ``TSeries(lags, dcf)``.  The lag of a pair is ``t_other - t_signal``: a peak at a
    positive lag means ``other`` follows ``signal``.
    """

    def __init__(self, max_lag=None, dlag=None, min_lag=None, normalization="global", min_pairs=2, include_self=False, *,
                 device=None):
        if normalization not in ("global", "local"):
            raise ValueError('normalization must be "global" or "local".')
        if int(min_pairs) != min_pairs or min_pairs < 2:
            raise ValueError("min_pairs must be an integer of at least 2.")
        for name, value in (("max_lag", max_lag), ("dlag", dlag), ("min_lag", min_lag)):
            if value is not None and not np.isfinite(value):
                raise ValueError(f"{name} must be finite.")
        if dlag is not None and not dlag > 0:
            raise ValueError("dlag must be positive.")
        self.max_lag = max_lag
        self.dlag = dlag
        self.min_lag = min_lag
        self.normalization = normalization
        self.min_pairs = int(min_pairs)
        self.include_self = bool(include_self)
        self.device = device

    def _grid(self, signal, other):
        """``(lags, edges)`` for the curves of a call (``other`` None: one curve)."""
        curves = [signal] if other is None else [signal, other]
        dlag = self.dlag
        if dlag is None:
            dlag = max(float(c.median_dt) for c in curves)
        max_lag = self.max_lag
        if max_lag is None:
            max_lag = 0.5 * min(float(c.baseline) for c in curves)
        min_lag = self.min_lag
        if min_lag is None:
            min_lag = 0.0 if other is None else -max_lag
        if not (np.isfinite(dlag) and dlag > 0):
            raise ValueError("dlag must be finite and positive (the default is median_dt).")
        if not (np.isfinite(max_lag) and np.isfinite(min_lag) and max_lag >= min_lag):
            raise ValueError("max_lag must be finite and not below min_lag.")
        nlag = int(np.floor((max_lag - min_lag) / dlag)) + 1
        lags = min_lag + dlag * np.arange(nlag)
        edges = (min_lag - 0.5 * dlag) + dlag * np.arange(nlag + 1)
        return lags, edges

    def __call__(self, signal, other=None, err=None, other_err=None):
        """The correlation of ``signal`` with itself (``other`` None) or with ``other``, as a ``TSeries`` over the lags.

        err, other_err: array-like, optional
            Measurement uncertainties of ``signal`` and of ``other``: their mean squares are taken off the variances
            of the global normalisation.  With one curve ``err`` serves both factors.
        """
        signal, ta, ya, ea = _curve(signal, err)
        auto = other is None
        if auto:
            if other_err is not None:
                raise ValueError("other_err needs other.")
            tb, yb, eb = ta, ya, ea
        else:
            other, tb, yb, eb = _curve(other, other_err)
        lags, edges = self._grid(signal, None if auto else other)
        norm = None
        if self.normalization == "global":
            factors = [np.var(y) - (0.0 if e is None else np.mean(e ** 2)) for y, e in ((ya, ea), (yb, eb))]
            if not all(f > 0 for f in factors):
                raise ValueError("The variance of a curve does not exceed the mean square of its uncertainties: "
                                 "the global normalisation is undefined.")
            norm = np.sqrt(factors[0] * factors[1])
        a = ya - np.mean(ya)
        b = a if auto else yb - np.mean(yb)
        pairs, sums = _cabi.dcf_scan(ta, a, tb, b, edges, skip_same_index=auto and not self.include_self,
                                     device=_cabi.pick_device(self.device, None))   # (one curve: the same arrays twice)
        self.signal = signal
        self.other = None if auto else other
        self.lags = lags
        self.edges = edges
        self.pairs = pairs
        self.sums = dict(zip(SUMS, sums))
        self.dcf, self.sigma = self.normalise(pairs, self.sums, norm, self.min_pairs)
        self.correlogram = TSeries(lags, self.dcf, assume_sorted=True)
        return self.correlogram

    @staticmethod
    def normalise(pairs, sums, norm, min_pairs=2):
        """``(dcf, sigma)`` of per-bin counts and sums: globally normalised by ``norm``, locally when it is None."""
        n = pairs.astype(float)
        with np.errstate(divide="ignore", invalid="ignore"):
            if norm is not None:
                dcf = sums["Sab"] / (n * norm)
                sigma = np.sqrt(np.maximum(sums["Sabab"] / norm ** 2 - n * dcf ** 2, 0)) / (n - 1)
            else:
                ma, mb = sums["Sa"] / n, sums["Sb"] / n
                dcf = (sums["Sab"] / n - ma * mb) / np.sqrt((sums["Saa"] / n - ma ** 2) * (sums["Sbb"] / n - mb ** 2))
                sigma = (1 - dcf ** 2) / np.sqrt(n - 1)
        few = pairs < min_pairs
        return np.where(few, np.nan, dcf), np.where(few, np.nan, sigma)

    @property
    def peak_lag(self):
        """The lag of the largest finite value (of equal ones the smaller ``|lag|``); None when no bin has a value."""
        finite = np.flatnonzero(np.isfinite(self.dcf))
        if finite.size == 0:
            return None
        at = finite[self.dcf[finite] == self.dcf[finite].max()]
        return float(self.lags[at[np.argmin(np.abs(self.lags[at]))]])

    @property
    def period(self):
        """One curve only: the lag of the most prominent peak among the bins with a value and a positive lag (the rule of
        the reference's ``acf_period_quality``, ``core.py:835-836``; of equal prominences the smaller lag); None when
        there is no peak."""
        if self.other is not None:
            raise ValueError("period is defined for the correlation of a curve with itself.")
        keep = np.isfinite(self.dcf) & (self.lags > 0)
        peaks = TSeries(self.lags[keep], self.dcf[keep], assume_sorted=True).find_peaks()
        if peaks.size == 0:
            return None
        return float(peaks.time[np.argmax(peaks.attrs["prominences"])])

    def copy(self):
        return _copy.deepcopy(self)
