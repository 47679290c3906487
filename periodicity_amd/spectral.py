"""Generalized Lomb-Scargle periodogram with the reference's callable API, computed on MI355X.

Drop-in for ``periodicity.spectral`` (``/root/reference/src/periodicity/spectral.py``):
``GLS(fmin, fmax, n, psd)(signal, err, fit_mean) -> FSeries`` with the same positional order,
defaults and attribute side effects (``.frequency .err .signal .periodogram``,
``spectral.py:97,101,133-134``), plus ``bootstrap / fap / fal / window / model / copy``
(``spectral.py:137-204``).  ``LombScargle`` is an alias of ``GLS``.

What differs, deliberately: the three ``_trig_sum`` calls (``spectral.py:109-112``) are an
FFT/extirpolation *approximation* upstream; here they are the exact direct sums that function's
docstring defines (``spectral.py:13-15``), evaluated by the HIP kernel in
``csrc/gls.hip``.  The frequency grid, weights and epilogue follow the reference line by line.
Nothing in this module computes a periodogram on the CPU.
"""
import collections as _collections
import copy as _copy

import numpy as np

from . import _cabi
from .core import FSeries, TSeries, _batch_errs, _batch_offsets, _batch_request, _batch_slots

__all__ = ["GLS", "LombScargle", "BGLST", "MultiHarmonicGLS", "KeplerianGLS", "BestOrbit", "MultibandGLS", "HTest", "ZTest", "SpinSearch", "GLSBatch", "PeakTable"]


def _as_tseries(signal):
    """``spectral.py:86-87``: anything that is not a time series is wrapped as values on
    ``arange`` times.  Real ``periodicity.core.TSeries`` objects pass through (duck typing)."""
    if isinstance(signal, TSeries) or (hasattr(signal, "time") and hasattr(signal, "values")
                                       and hasattr(signal, "baseline")):
        return signal
    return TSeries(values=signal)


class GLS(object):
    """Generalized Lomb-Scargle periodogram (Zechmeister & Kurster 2009) of a discrete signal.

    Parameters (``spectral.py:53-72``)
    ----------
    fmin, fmax: float, optional
        Grid limits; default half a cycle per baseline and the pseudo-Nyquist ``0.5/median_dt``.
    n: float, optional
        Samples per peak (default 5): grid spacing is ``1 / baseline / n``.
    psd: bool, optional
        Leave the periodogram un-normalised.
    method: {"direct", "fft"}, keyword-only, optional
        ``"direct"`` (default): exact direct summation of the trig sums (``spectral.py:13-15``).
        ``"fft"``: the reference's own Press-Rybicki extirpolation + FFT (``spectral.py:18-39``)
        on the device — reproduces upstream's values including their approximation error.
    device: int, keyword-only, optional
        GPU ordinal (default ``$PERIODICITY_AMD_DEVICE`` or 0).
    devices: sequence of int, keyword-only, optional
        Shard the frequency grid over these GPUs of one node (RCCL all-gather of the power array).
    """

    def __init__(self, fmin=None, fmax=None, n=5, psd=False, *, method="direct", device=None,
                 devices=None):
        if method not in ("direct", "fft"):
            raise ValueError("method must be 'direct' or 'fft'")
        self.fmin = fmin
        self.fmax = fmax
        self.n = n
        self.psd = psd
        self.method = method
        self.device = device
        self.devices = None if devices is None else tuple(devices)

    def _grid_scalars(self, signal):
        """``df``, ``fmin``, ``fmax`` of ``spectral.py:88-96``."""
        df = 1.0 / signal.baseline / self.n
        fmin = 0.5 * df if self.fmin is None else self.fmin
        fmax = 0.5 / signal.median_dt if self.fmax is None else self.fmax
        return df, fmin, fmax

    def _grid(self, signal):
        """Uniform frequency grid of ``spectral.py:88-98`` — built by ``np.arange`` itself so its
        length and values carry numpy's rounding; the kernel reproduces ``start + j*step``."""
        df, fmin, fmax = self._grid_scalars(signal)
        return np.arange(fmin, fmax + df, df)

    def __call__(self, signal, err=None, fit_mean=True):
        """Periodogram of ``signal`` on the default (or configured) uniform grid.

        Parameters (``spectral.py:74-85``)
        ----------
        err: array-like, optional
            Measurement uncertainties for each sample (may be heteroscedastic).
        fit_mean: bool, optional
            Let the mean float with the fit (the "generalized" part).
        """
        signal = _as_tseries(signal)
        self.frequency = self._grid(signal)
        f0, delta, nf = _cabi.grid_params(self.frequency)
        have_err = err is not None
        if not have_err:
            err = np.ones_like(signal.values)
        self.err = err
        dy = np.asarray(err, dtype=float) if have_err else None
        t = np.asarray(signal.time, dtype=float)
        y = np.asarray(signal.values, dtype=float)
        if self.method == "fft":
            # the reference's own extirpolation + FFT evaluation of the trig sums, on the device
            df, fmin, _ = self._grid_scalars(signal)
            dev = _cabi.pick_device(self.device, self.devices)
            power = _cabi.gls_scan_fft(t, y, dy, fmin, df, nf, fit_mean, self.psd, device=dev)
        elif self.devices is not None and len(self.devices) > 1:
            power = _cabi.gls_scan_multi(t, y, dy, f0, delta, nf, fit_mean, self.psd,
                                         self.devices)
        else:
            dev = _cabi.pick_device(self.device, self.devices)
            power = _cabi.gls_scan(t, y, dy, f0, delta, nf, fit_mean, self.psd, device=dev)
        self.signal = signal
        self.periodogram = FSeries(self.frequency, power)
        return self.periodogram

    def copy(self):
        return _copy.deepcopy(self)

    def _ragged_grids(self, signals):
        """Every curve's grid, exactly ``self._grid(signal)``, and the ``(f0, delta, f_offsets)`` the ragged
        kernel rebuilds it from (``start + j*step`` per curve).  A grid of fewer than two bins has no step of its
        own; any positive step rebuilds it, and 1 is used."""
        grids = [self._grid(s) for s in signals]
        f_offsets = _batch_offsets([g.size for g in grids])
        f0 = np.array([g[0] if g.size else 0.0 for g in grids], dtype=np.float64)
        delta = np.array([g[1] - g[0] if g.size > 1 else 1.0 for g in grids], dtype=np.float64)
        return grids, f0, delta, f_offsets

    def batch(self, signals, errs=None, fit_mean=True, *, peaks=0, by_prominence=False, want_power=True):
        """Periodograms of many light curves, each on the grid its own data give (``self._grid``, the rule of
        ``spectral.py:88-98`` applied per curve), in one set of launches (``pdc_gls_scan_ragged`` /
        ``pdc_gls_ragged_peaks``): what a loop of ``GLS(...)(s, e, fit_mean)`` followed by
        ``period_at_highest_peak`` etc. gives, without a launch per curve.

        Parameters
        ----------
        signals: sequence of TSeries (or anything ``GLS.__call__`` accepts)
        errs: None, or a sequence (one entry per signal) of arrays or Nones
        fit_mean: bool
        peaks: int, keyword-only
            ``k > 0``: also the ``k`` (<= 1024) highest - or, ``by_prominence``, most prominent - ``find_peaks``
            maxima of every spectrum, found on the device (``GLSBatch.peaks``).
        want_power: bool, keyword-only
            ``False``: the spectra stay on the device (``periodograms`` is None); needs ``peaks > 0``.

        With ``devices=(...)`` the curves are dealt to those device slots in contiguous groups balanced by
        ``sum n_b nf_b``.  The ``GLS`` object's own attributes (``frequency``, ``periodogram`` ...) are left as
        they were.
        """
        if self.method == "fft":
            raise NotImplementedError("GLS.batch runs the direct sums only: method='fft' needs one FFT size per curve")
        signals = [_as_tseries(s) for s in signals]
        if not signals:
            raise ValueError("GLS.batch needs at least one signal")
        peaks = _batch_request(peaks, want_power)
        sizes = [len(s) for s in signals]
        dy = _batch_errs(errs, sizes)
        grids, f0, delta, f_offsets = self._ragged_grids(signals)
        t = np.concatenate([np.asarray(s.time, dtype=float) for s in signals])
        y = np.concatenate([np.asarray(s.values, dtype=float) for s in signals])
        offsets = _batch_offsets(sizes)
        devices = _batch_slots(self.devices)
        if peaks:
            out = _cabi.gls_ragged_peaks(t, y, dy, offsets, f0, delta, f_offsets, k=peaks, by_prominence=by_prominence,
                                         fit_mean=fit_mean, psd=self.psd, want_power=want_power, device=self.device,
                                         devices=devices)
            power = out["power"]
            table = PeakTable(grids, out, by_prominence)
        else:
            power = _cabi.gls_scan_ragged(t, y, dy, offsets, f0, delta, f_offsets, fit_mean, self.psd,
                                          device=self.device, devices=devices)[0]
            table = None
        periodograms = None
        if want_power:
            periodograms = [FSeries(g, power[f_offsets[b]:f_offsets[b + 1]]) for b, g in enumerate(grids)]
        return GLSBatch(grids, periodograms, table)

    def bootstrap(self, n_bootstraps, random_seed=None):
        """Maxima of ``n_bootstraps`` periodograms of ``(values, err)`` resampled with replacement
        on the unchanged time axis (``spectral.py:140-152``).  The draws come from
        ``default_rng(seed).integers(0, n, n)`` once per replicate, in order, exactly as
        upstream; the replicates then run as ONE batched launch that shares the time axis and
        returns only the NaN-aware maximum of each spectrum (with ``devices=(...)``: one contiguous
        group of replicates per GPU, no exchange).  Only the curve and the 4-byte indices go to the device
        (``pdc_gls_bootstrap``)."""
        rng = np.random.default_rng(random_seed)
        ndata = len(self.signal)
        values = np.asarray(self.signal.values, dtype=float)
        err = np.asarray(self.err, dtype=float)
        t = np.asarray(self.signal.time, dtype=float)
        # the draws, exactly as upstream makes them (one ``integers(0, n, n)`` call per replicate, in order) -
        # kept as 4-byte indices: the resampled (values, err) arrays are never built on the host, the device
        # prologue gathers ``values[picks]``, ``err[picks]`` while it lays out the weight table
        picks = np.empty((n_bootstraps, ndata), dtype=np.int32)
        for i in range(n_bootstraps):
            picks[i] = rng.integers(0, ndata, ndata)
        bs_replicates = np.empty(n_bootstraps)
        # err=None upstream means all-ones errors (``spectral.py:99-100``): resampling leaves them
        # all ones, and the equal-weights kernels share the weight-only sums between replicates
        dy = None if np.all(err == 1.0) else err
        if n_bootstraps and self.method == "fft":
            # all replicates through the reference's own algorithm in one batched set of launches
            df, fmin, _ = self._grid_scalars(self.signal)
            nf = self._grid(self.signal).size
            bs_replicates[:] = _cabi.gls_bootstrap(t, values, dy, picks, fmin, df, nf, True, self.psd, method="fft",
                                                   device=_cabi.pick_device(self.device, self.devices))[0]
        elif n_bootstraps:
            f0, delta, nf = _cabi.grid_params(self._grid(self.signal))
            bs_replicates[:] = _cabi.gls_bootstrap(t, values, dy, picks, f0, delta, nf, True, self.psd,
                                                   device=self.device, devices=self.devices)[0]
        self.bs_replicates = bs_replicates
        return self.bs_replicates

    def fap(self, power):
        """Fraction of bootstrap maxima above ``power`` (``spectral.py:154-160``)."""
        return np.mean(power < self.bs_replicates)

    def fal(self, fap):
        """Power level at false-alarm probability ``fap`` (``spectral.py:162-163``)."""
        return np.quantile(self.bs_replicates, 1 - fap)

    def window(self):
        """Spectral window: periodogram of an all-ones signal, no floating mean
        (``spectral.py:165-167``)."""
        gls = self.copy()
        return gls(0.0 * self.signal + 1.0, fit_mean=False)

    def model(self, tf, f0):
        """Weighted least-squares sinusoid-plus-offset at frequency ``f0`` evaluated at times
        ``tf`` (``spectral.py:169-204``).  O(N) host arithmetic, not part of the scan."""
        t = np.asarray(self.signal.time, dtype=float)
        sigma = np.asarray(self.err, dtype=float)
        w = sigma ** -2.0
        y = np.asarray(self.signal.values, dtype=float)
        y_mean = np.dot(y, w) / w.sum()

        def basis(times):
            arg = 2 * np.pi * f0 * np.asarray(times, dtype=float)
            return np.vstack([np.ones_like(arg), np.sin(arg), np.cos(arg)])

        A = basis(t) / sigma
        theta = np.linalg.solve(A @ A.T, A @ ((y - y_mean) / sigma))
        return TSeries(tf, y_mean + basis(tf).T @ theta)


LombScargle = GLS


class PeakTable(object):
    """The ``k`` best peaks of every spectrum of a ``GLS.batch`` call, ``[B][k]`` arrays ranked descending (by
    height, or by prominence), padded with NaN (``index``: -1) past a curve's ``count`` of ``find_peaks`` maxima.
    (``PDM.batch`` and ``ConditionalEntropy.batch`` fill it with the ``find_dips`` minima, deepest first.)

    ``period_lo[b, r]``, ``period_hi[b, r]`` are the pair ``periods_at_half_max(r + 1, use_prominence=by_prominence)``
    returns for curve ``b`` (``core.py:963-978``); each is NaN where that method finds no crossing on its side.
    """

    def __init__(self, grids, out, by_prominence, frequency_at=None):
        self.by_prominence = bool(by_prominence)
        self.count = out["count"]
        self.index = out["indices"]
        self.height = out["heights"]
        self.prominence = out["prominences"]
        B, k = self.index.shape
        self.frequency = np.full((B, k), np.nan)
        self.period_lo = np.full((B, k), np.nan)
        self.period_hi = np.full((B, k), np.nan)
        columns = (("frequency", self.index), ("period_lo", out["half_lo"]), ("period_hi", out["half_hi"]))
        if frequency_at is None:
            for b, g in enumerate(grids):
                for name, idx in columns:
                    ok = idx[b] >= 0
                    getattr(self, name)[b, ok] = g[idx[b][ok]]
        else:   # frequency_at(rows, bins): the grids without building them (the phase scans' batches)
            rows = np.broadcast_to(np.arange(B)[:, None], (B, k))
            for name, idx in columns:
                ok = idx >= 0
                getattr(self, name)[ok] = frequency_at(rows[ok], idx[ok])
        with np.errstate(divide="ignore"):
            self.period = 1.0 / self.frequency
            self.period_lo = 1.0 / self.period_lo
            self.period_hi = 1.0 / self.period_hi


class GLSBatch(object):
    """What ``GLS.batch`` returns: ``frequency`` (one grid per curve), ``periodograms`` (one ``FSeries`` per curve,
    or None) and ``peaks`` (a :class:`PeakTable`, or None)."""

    def __init__(self, frequency, periodograms, peaks):
        self.frequency = frequency
        self.periodograms = periodograms
        self.peaks = peaks

    def __len__(self):
        return len(self.frequency)


class BGLST(GLS):
    """Bayesian generalised Lomb-Scargle periodogram with linear trend.

    The reference exports this name (``spectral.py:7``) for an empty class (``spectral.py:207-208``; its README lists
    the method as "soon"): there is no upstream behaviour to reproduce - **parity unpinned by the reference**.  This
    class computes the published statistic (Olspert, Pelt, Käpylä & Lehtinen 2018, A&A 615, A111) on the grid rule of
    ``GLS`` (``spectral.py:88-98``): for every trial frequency the log marginal likelihood of

        ``y_i = A cos(2 pi f t_i) + B sin(2 pi f t_i) + alpha tau_i + beta + eps_i``,  ``eps_i ~ N(0, err_i**2)``,

    ``tau = (t - t_ref) / baseline``, with independent zero-mean Gaussian priors ``A, B ~ N(0, sigma_A**2)``,
    ``alpha ~ N(0, sigma_alpha**2)`` (trend over the whole baseline), ``beta ~ N(0, sigma_beta**2)`` (level at
    ``t_ref``) integrated out analytically.  Unlike ``GLS`` the values are NOT centred or detrended first - the
    trend is part of the model and competes with long periods on equal terms, which is the point of the method.

    Parameters
    ----------
    fmin, fmax, n: as ``GLS``.
    sigma_A, sigma_alpha, sigma_beta: float, keyword-only, optional
        Prior standard deviations.  Defaults (this build's; the reference has none): ``std(values)`` for the
        amplitudes and for the trend over the baseline, ``sqrt(var(values) + mean(values)**2)`` for the level.
    t_ref: float, keyword-only, optional
        Time at which ``beta`` is the level (default: the middle of the series).
    device: int, keyword-only, optional
    """

    def __init__(self, fmin=None, fmax=None, n=5, *, sigma_A=None, sigma_alpha=None, sigma_beta=None, t_ref=None,
                 device=None):
        super().__init__(fmin, fmax, n, False, device=device)
        self.sigma_A, self.sigma_alpha, self.sigma_beta, self.t_ref = sigma_A, sigma_alpha, sigma_beta, t_ref

    def priors(self, signal):
        """``(sigma_A, sigma_alpha, sigma_beta, t_ref)`` with the defaults filled in for ``signal``."""
        signal = _as_tseries(signal)
        y = np.asarray(signal.values, dtype=float)
        t = np.asarray(signal.time, dtype=float)
        spread = float(np.std(y))
        spread = spread if spread > 0 else 1.0
        return (float(self.sigma_A) if self.sigma_A is not None else spread,
                float(self.sigma_alpha) if self.sigma_alpha is not None else spread,
                float(self.sigma_beta) if self.sigma_beta is not None else float(np.sqrt(np.var(y) + np.mean(y) ** 2)) or 1.0,
                float(self.t_ref) if self.t_ref is not None else 0.5 * (t[0] + t[-1]))

    @staticmethod
    def _scalars(t, y, err, sigma_A, sigma_alpha, sigma_beta, t_ref):
        """The twelve frequency-independent inputs of ``pdc_bglst_scan`` (include/periodicity_hip.h)."""
        span = float(t[-1] - t[0]) or 1.0
        w = err ** -2.0
        W = float(w.sum())
        w = w / W
        tau = (t - t_ref) / span
        return np.array([W, np.dot(w, y * y), np.dot(w, y), np.dot(w, tau * y), np.dot(w, tau * tau), np.dot(w, tau),
                         (t[0] - t_ref) / span, 1.0 / span, sigma_A ** -2.0, sigma_alpha ** -2.0, sigma_beta ** -2.0,
                         float(np.sum(np.log(2 * np.pi * err ** 2))) + 4 * np.log(sigma_A) + 2 * np.log(sigma_alpha)
                         + 2 * np.log(sigma_beta)])

    def __call__(self, signal, err=None):
        """``FSeries(frequency, log marginal likelihood)``; ``period_at_highest_peak`` etc. as for ``GLS``."""
        signal = _as_tseries(signal)
        if len(signal) < 4:
            raise ValueError("BGLST marginalises four parameters: at least four samples")
        self.frequency = self._grid(signal)
        f0, delta, nf = _cabi.grid_params(self.frequency)
        t = np.asarray(signal.time, dtype=float)
        y = np.asarray(signal.values, dtype=float)
        have_err = err is not None
        err = np.ones_like(y) if not have_err else np.asarray(err, dtype=float)
        if err.size != y.size:
            raise ValueError("Input arrays have incompatible lengths.")
        self.err = err
        sA, sa, sb, t_ref = self.priors(signal)
        scalars = self._scalars(t, y, err, sA, sa, sb, t_ref)
        dev = _cabi.pick_device(self.device, None)
        ll = _cabi.bglst_scan(t, y, err if have_err else None, f0, delta, nf, scalars, device=dev)
        self.signal = signal
        self.periodogram = FSeries(self.frequency, ll)
        return self.periodogram

    def posterior_mean(self, frequency):
        """Posterior means ``(A, B, alpha, beta)`` of the model's parameters at one frequency (``alpha`` per unit
        time, ``beta`` at ``t_ref``) for the last signal: a 4 x 4 solve on the host."""
        t = np.asarray(self.signal.time, dtype=float)
        y = np.asarray(self.signal.values, dtype=float)
        sA, sa, sb, t_ref = self.priors(self.signal)
        span = float(t[-1] - t[0]) or 1.0
        phi = np.stack([np.cos(2 * np.pi * frequency * t), np.sin(2 * np.pi * frequency * t), (t - t_ref) / span,
                        np.ones_like(t)], axis=1)
        w = np.asarray(self.err, dtype=float) ** -2.0
        m = phi.T @ (phi * w[:, None]) + np.diag([sA ** -2.0, sA ** -2.0, sa ** -2.0, sb ** -2.0])
        a, b, alpha, beta = np.linalg.solve(m, phi.T @ (w * y))
        return a, b, alpha / span, beta

    # the GLS-only methods make no sense for a likelihood
    def bootstrap(self, *args, **kwargs):
        raise NotImplementedError("BGLST has no bootstrap: the log-likelihood itself carries the significance")

    fap = fal = window = model = bootstrap

    def batch(self, *args, **kwargs):
        raise NotImplementedError("BGLST.batch is not implemented: the ragged-grid batch computes GLS power only")


class MultiHarmonicGLS(GLS):
    """Multi-harmonic generalised Lomb-Scargle periodogram: at every trial frequency the weighted least-squares fit
    of a truncated Fourier series (Schwarzenberg-Czerny 1996, ApJ 460, L107; Palmer 2009, ApJ 695, 496 - what other
    packages expose as ``nterms``), for variables that are periodic but not sinusoidal (eclipses, RR Lyrae, spots).

    The reference has no such class - **parity unpinned by the reference**.  Grid, weights, centring and the two
    normalisations are those of ``GLS`` (``spectral.py:88-108,129-132``): with ``theta = 2 pi f (t - t[0])``, design
    columns ``cos(h theta), sin(h theta)`` for ``h = 1 .. nterms`` plus a constant when ``fit_mean``,
    ``M = Phi^T diag(w) Phi``, ``b = Phi^T diag(w) y`` and ``YY = sum w y**2``,

        ``power(f) = b^T M^-1 b / YY``   (``psd``: ``b^T M^-1 b * 0.5 * sum err**-2``),

    which for ``nterms=1`` is the GLS power.  At the lowest few frequencies the harmonics are nearly constant over
    the baseline and ``M`` is close to singular: such a bin is badly conditioned, and NaN where a Cholesky pivot
    is not positive.  Evaluated by ``csrc/mhgls.hip``; nothing here computes a periodogram on the CPU.

    Parameters
    ----------
    fmin, fmax, n, psd: as ``GLS``.
    nterms: int, keyword-only, optional
        Harmonics of the model, 1 .. 4 (default 2).
    device: int, keyword-only, optional
    """

    MAX_TERMS = 4

    def __init__(self, fmin=None, fmax=None, n=5, psd=False, *, nterms=2, device=None):
        if isinstance(nterms, bool) or nterms != int(nterms) or not 1 <= int(nterms) <= self.MAX_TERMS:
            raise ValueError(f"nterms must be an integer 1 .. {self.MAX_TERMS}")
        super().__init__(fmin, fmax, n, psd, device=device)
        self.nterms = int(nterms)

    def __call__(self, signal, err=None, fit_mean=True):
        """``FSeries(frequency, power)`` on the grid of ``GLS``; ``period_at_highest_peak`` etc. as for ``GLS``."""
        signal = _as_tseries(signal)
        self.frequency = self._grid(signal)
        f0, delta, nf = _cabi.grid_params(self.frequency)
        if nf < 2:   # a grid of one bin has no step of its own; any positive step rebuilds it
            delta = 1.0
        have_err = err is not None
        if not have_err:
            err = np.ones_like(signal.values)
        dy = np.asarray(err, dtype=float) if have_err else None
        t = np.asarray(signal.time, dtype=float)
        y = np.asarray(signal.values, dtype=float)
        dev = _cabi.pick_device(self.device, None)
        power = _cabi.mhgls_scan(t, y, dy, f0, delta, nf, self.nterms, fit_mean, self.psd, device=dev)
        self.err = err
        self.fit_mean = bool(fit_mean)
        self.signal = signal
        self.periodogram = FSeries(self.frequency, power)
        return self.periodogram

    def _design(self, times, f0):
        """Design columns of the last call's model at frequency ``f0``, one row per time."""
        arg = 2 * np.pi * f0 * (np.asarray(times, dtype=float) - float(self.signal.time[0]))
        cols = [np.ones_like(arg)] if self.fit_mean else []
        for h in range(1, self.nterms + 1):
            cols += [np.cos(h * arg), np.sin(h * arg)]
        return np.stack(cols, axis=1)

    def model(self, tf, f0):
        """The fitted Fourier series of the last call (its ``err`` and ``fit_mean``) at frequency ``f0``, evaluated
        at times ``tf``.  O(N) host arithmetic, not part of the scan."""
        sigma = np.asarray(self.err, dtype=float)
        y = np.asarray(self.signal.values, dtype=float)
        y_mean = np.dot(y, sigma ** -2.0) / np.sum(sigma ** -2.0) if self.fit_mean else 0.0
        A = self._design(self.signal.time, f0) / sigma[:, None]
        theta = np.linalg.solve(A.T @ A, A.T @ ((y - y_mean) / sigma))
        return TSeries(tf, y_mean + self._design(tf, f0) @ theta)

    def bootstrap(self, *args, **kwargs):
        raise NotImplementedError("MultiHarmonicGLS has no bootstrap yet: the batched replicate kernels compute GLS power only")

    fap = fal = bootstrap

    def batch(self, *args, **kwargs):
        raise NotImplementedError("MultiHarmonicGLS.batch is not implemented: the ragged-grid batch computes GLS power only")


BestOrbit = _collections.namedtuple("BestOrbit", "frequency e m0 power")


def _frac_product(a, b):
    """``frac(a * b)`` in [-1/2, 1/2] with the product carried exactly (Veltkamp split, Dekker product), as the kernels
    reduce their cycles."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    hi = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    a1, b1 = ca - (ca - a), cb - (cb - b)
    a2, b2 = a - a1, b - b1
    lo = ((a1 * b1 - hi) + a1 * b2 + a2 * b1) + a2 * b2
    return (hi - np.rint(hi)) + lo


def _true_anomaly(cycles, e):
    """``(cos nu, sin nu)`` at mean anomaly ``cycles`` by a bracketed Newton iteration in fp64.  O(N) host arithmetic
    for ``orbit`` and ``model``, not part of the scan."""
    cycles = np.asarray(cycles, dtype=float)
    m = cycles - np.rint(cycles)
    M = 2 * np.pi * np.abs(m)
    lo, hi = np.zeros_like(M), np.full_like(M, np.pi)
    E = M + e * np.sin(M)
    for _ in range(64):
        g = E - e * np.sin(E) - M
        lo, hi = np.where(g < 0, E, lo), np.where(g > 0, E, hi)
        step = E - g / (1 - e * np.cos(E))
        E = np.where((step > lo) & (step < hi), step, 0.5 * (lo + hi))
    inv = 1 / (1 - e * np.cos(E))
    return (np.cos(E) - e) * inv, np.sign(m) * np.sqrt((1 - e) * (1 + e)) * np.sin(E) * inv


class KeplerianGLS(GLS):
    """Keplerian periodogram (Zechmeister & Kurster 2009, A&A 496, 577, section 4): at every trial frequency the best
    weighted least-squares fit of a Keplerian orbit, scanned over a grid of eccentricities and times of periastron -
    the statistic for radial-velocity curves of eccentric orbits, where a sinusoid loses most of the power.

    The reference has no such class - **parity unpinned by the reference**.  Grid, weights, centring and the two
    normalisations are those of ``GLS``.  With ``phi = frac(f (t - t[0]))``, ``M = 2 pi (phi - m0)``, ``E`` the solution
    of ``E - e sin E = M`` and ``nu`` the true anomaly, the design columns are ``cos nu, sin nu`` plus a constant when
    ``fit_mean``, and a cell ``(f, e, m0)`` holds ``b^T M^-1 b / YY`` as ``MultiHarmonicGLS`` defines it; the
    periodogram is the largest cell of each frequency.  At ``e = 0`` a cell is the GLS power.  Evaluated by
    ``csrc/kepler.hip``; nothing here computes a periodogram on the CPU.

    Parameters
    ----------
    fmin, fmax, n, psd: as ``GLS``.
    ecc: int or array, keyword-only, optional
        Eccentricities, each in [0, 0.95]; an int gives ``np.linspace(0, 0.9, ecc)`` (default 10).
    n_phase: int or array, keyword-only, optional
        Mean anomalies at the first sample in cycles, each in [0, 1); an int gives ``np.arange(n_phase) / n_phase``
        (default 32).  The time of periastron of a cell is ``t[0] + m0 / f``.
    device: int, keyword-only, optional

    After a call: ``.cell`` (per bin the index ``k * len(m0) + l`` of its best cell, -1 where every cell is NaN),
    ``.eccentricity`` and ``.periastron_phase`` (per bin, NaN there), ``.cube`` (``[nf][ne][nm]``, None unless
    ``want_cube``) and ``.best``, the ``BestOrbit(frequency, e, m0, power)`` of the highest bin.
    """

    MAX_ECC = 0.95
    MAX_CELLS = 65535

    def __init__(self, fmin=None, fmax=None, n=5, psd=False, *, ecc=10, n_phase=32, device=None):
        self.ecc = self._list(ecc, "ecc", lambda k: np.linspace(0.0, 0.9, k), lambda a: (a >= 0) & (a <= self.MAX_ECC),
                              f"in [0, {self.MAX_ECC}]")
        self.m0 = self._list(n_phase, "n_phase", lambda k: np.arange(k) / k, lambda a: (a >= 0) & (a < 1), "in [0, 1)")
        if self.ecc.size * self.m0.size > self.MAX_CELLS:
            raise ValueError(f"at most {self.MAX_CELLS} cells (eccentricities times phases) per frequency")
        super().__init__(fmin, fmax, n, psd, device=device)

    @staticmethod
    def _list(value, name, from_count, in_range, range_text):
        if isinstance(value, bool):
            raise ValueError(f"{name} must be a count or an array")
        if isinstance(value, (int, np.integer)):
            if value < 1:
                raise ValueError(f"{name} must be at least 1")
            return from_count(int(value))
        a = np.array(value, dtype=float)
        if a.ndim != 1 or a.size < 1:
            raise ValueError(f"{name} must be a count or a one-dimensional array that is not empty")
        if not np.all(in_range(a)):   # (NaN fails every comparison)
            raise ValueError(f"every entry of {name} must be finite and {range_text}")
        return a

    def __call__(self, signal, err=None, fit_mean=True, want_cube=False):
        """``FSeries(frequency, power)`` on the grid of ``GLS``, the power of a bin that of its best cell;
        ``period_at_highest_peak`` etc. as for ``GLS``."""
        signal = _as_tseries(signal)
        self.frequency = self._grid(signal)
        f0, delta, nf = _cabi.grid_params(self.frequency)
        if nf < 2:   # a grid of one bin has no step of its own; any positive step rebuilds it
            delta = 1.0
        have_err = err is not None
        if not have_err:
            err = np.ones_like(signal.values)
        dy = np.asarray(err, dtype=float) if have_err else None
        t = np.asarray(signal.time, dtype=float)
        y = np.asarray(signal.values, dtype=float)
        dev = _cabi.pick_device(self.device, None)
        out = _cabi.kepler_scan(t, y, dy, f0, delta, nf, self.ecc, self.m0, fit_mean, self.psd, want_cube=want_cube,
                                device=dev)
        self.err = err
        self.fit_mean = bool(fit_mean)
        self.signal = signal
        self.cell = out["cell"]
        self.cube = out["cube"]
        found = self.cell >= 0
        at = np.where(found, self.cell, 0)
        self.eccentricity = np.where(found, self.ecc[at // self.m0.size], np.nan)
        self.periastron_phase = np.where(found, self.m0[at % self.m0.size], np.nan)
        value, bin_, cell = out["best"]
        self.best_bin = bin_
        self.best = (BestOrbit(np.nan, np.nan, np.nan, np.nan) if bin_ < 0 else
                     BestOrbit(float(self.frequency[bin_]), float(self.ecc[cell // self.m0.size]),
                               float(self.m0[cell % self.m0.size]), value))
        self.periodogram = FSeries(self.frequency, out["power"])
        return self.periodogram

    def _bin(self, f0):
        """The bin nearest ``f0`` (None: the best bin) of the last call, which must have a cell."""
        j = self.best_bin if f0 is None else int(np.argmin(np.abs(self.frequency - f0)))
        if j < 0 or self.cell[j] < 0:
            raise ValueError("no cell of that bin has a value")
        return j

    def _fit(self, j):
        """Host refit at bin ``j`` and its cell: ``(f, e, m0, ybar, theta)`` with theta the coefficients of
        ``cos nu, sin nu`` and, with ``fit_mean``, the constant.  O(N) host arithmetic, not part of the scan."""
        f, e, m0 = float(self.frequency[j]), float(self.eccentricity[j]), float(self.periastron_phase[j])
        sigma = np.asarray(self.err, dtype=float)
        t = np.asarray(self.signal.time, dtype=float)
        y = np.asarray(self.signal.values, dtype=float)
        ybar = np.dot(y, sigma ** -2.0) / np.sum(sigma ** -2.0) if self.fit_mean else 0.0
        A = self._design(t, f, e, m0) / sigma[:, None]
        theta = np.linalg.solve(A.T @ A, A.T @ ((y - ybar) / sigma))
        return f, e, m0, ybar, theta

    def _design(self, times, f, e, m0):
        c, s = _true_anomaly(_frac_product(f, np.asarray(times, dtype=float) - float(self.signal.time[0])) - m0, e)
        return np.stack([c, s] + ([np.ones_like(c)] if self.fit_mean else []), axis=1)

    def orbit(self, f0=None):
        """The orbit fitted at the bin nearest ``f0`` (None: the best bin) and that bin's cell, as a dict
        ``period, K, e, omega, gamma, t_peri`` of ``y = K (cos(nu + omega) + e cos omega) + gamma``: with the fitted
        coefficients ``A cos nu + B sin nu + const``, ``A = K cos omega``, ``B = -K sin omega``,
        ``gamma = const - K e cos omega + ybar`` and ``t_peri = t[0] + m0 / f``."""
        f, e, m0, ybar, theta = self._fit(self._bin(f0))
        A, B = float(theta[0]), float(theta[1])
        const = float(theta[2]) if self.fit_mean else 0.0
        return {"period": 1.0 / f, "K": float(np.hypot(A, B)), "e": e, "omega": float(np.arctan2(-B, A) % (2 * np.pi)),
                "gamma": const - A * e + ybar, "t_peri": float(self.signal.time[0]) + m0 / f}

    def model(self, tf, f0=None):
        """The orbit of ``orbit(f0)`` evaluated at times ``tf``."""
        f, e, m0, ybar, theta = self._fit(self._bin(f0))
        return TSeries(tf, ybar + self._design(tf, f, e, m0) @ theta)

    def bootstrap(self, *args, **kwargs):
        raise NotImplementedError("KeplerianGLS has no bootstrap yet: the batched replicate kernels compute GLS power only")

    fap = fal = bootstrap

    def batch(self, *args, **kwargs):
        raise NotImplementedError("KeplerianGLS.batch is not implemented: the ragged-grid batch computes GLS power only")


class MultibandGLS(GLS):
    """Shared-phase multiband generalised Lomb-Scargle periodogram (VanderPlas & Ivezic 2015, ApJ 812, 18, the
    ``Nbase = nterms, Nband = 0`` model; ``LombScargleMultiband`` elsewhere): ONE period from a light curve whose samples
    come from several filters or instruments, each with its own mean.  At every trial frequency one truncated Fourier
    series common to all bands plus one floating offset per band is fitted by weighted least squares.

    The reference has no such class - **parity unpinned by the reference**.  Grid, weights (``err**-2`` normalised over
    ALL samples) and the two normalisations are those of ``GLS`` on the merged curve.  With ``fit_mean`` every band is
    centred on its own weighted mean (for conditioning; the offsets still float), the design has one indicator column
    per band and ``cos(h theta), sin(h theta)`` for ``h = 1 .. nterms``, and

        ``power(f) = b^T M^-1 b / YY``   (``psd``: ``b^T M^-1 b * 0.5 * sum err**-2``);

    with one band that is ``MultiHarmonicGLS(nterms)``.  Without ``fit_mean`` there are no offsets and the bands do not
    enter: ``MultiHarmonicGLS(nterms)(..., fit_mean=False)`` on the merged curve.  A bin whose Cholesky pivot is not
    positive is NaN.  Evaluated by ``csrc/mbgls.hip``; nothing here computes a periodogram on the CPU.

    Parameters
    ----------
    fmin, fmax, n, psd: as ``GLS``.
    nterms: int, keyword-only, optional
        Harmonics of the shared series, 1 .. 3 (default 1).
    device: int, keyword-only, optional
    """

    MAX_TERMS = 3
    MAX_BANDS = 32

    def __init__(self, fmin=None, fmax=None, n=5, psd=False, *, nterms=1, device=None):
        if isinstance(nterms, bool) or nterms != int(nterms) or not 1 <= int(nterms) <= self.MAX_TERMS:
            raise ValueError(f"nterms must be an integer 1 .. {self.MAX_TERMS}")
        super().__init__(fmin, fmax, n, psd, device=device)
        self.nterms = int(nterms)

    def __call__(self, signal, bands, err=None, fit_mean=True):
        """``FSeries(frequency, power)`` on the grid of ``GLS``.  ``bands``: one label per sample (strings or integers),
        aligned with the time-sorted samples of the ``TSeries`` as ``err`` is."""
        signal = _as_tseries(signal)
        labels, index = np.unique(np.asarray(bands), return_inverse=True)
        index = np.ascontiguousarray(index.reshape(-1), dtype=np.int32)
        if np.asarray(bands).ndim != 1 or index.size != len(signal):
            raise ValueError("Input arrays have incompatible lengths.")
        if labels.size > self.MAX_BANDS:
            raise ValueError(f"at most {self.MAX_BANDS} bands (got {labels.size})")
        self.frequency = self._grid(signal)
        f0, delta, nf = _cabi.grid_params(self.frequency)
        if nf < 2:   # a grid of one bin has no step of its own; any positive step rebuilds it
            delta = 1.0
        have_err = err is not None
        if not have_err:
            err = np.ones_like(signal.values)
        dy = np.asarray(err, dtype=float) if have_err else None
        t = np.asarray(signal.time, dtype=float)
        y = np.asarray(signal.values, dtype=float)
        dev = _cabi.pick_device(self.device, None)
        power = _cabi.mbgls_scan(t, y, dy, index, labels.size, f0, delta, nf, self.nterms, fit_mean, self.psd, device=dev)
        self.err = err
        self.fit_mean = bool(fit_mean)
        self.signal = signal
        self.bands = labels
        self.band_index = index
        self.periodogram = FSeries(self.frequency, power)
        return self.periodogram

    def _harmonics(self, times, f0):
        arg = 2 * np.pi * f0 * (np.asarray(times, dtype=float) - float(self.signal.time[0]))
        return np.stack([f(h * arg) for h in range(1, self.nterms + 1) for f in (np.cos, np.sin)], axis=1)

    def _fit(self, f0):
        """``(offsets [n_bands], harmonic coefficients [2 nterms])`` of the last call's model at frequency ``f0``: a host
        weighted least-squares fit, O(N)."""
        sigma = np.asarray(self.err, dtype=float)
        y = np.asarray(self.signal.values, dtype=float)
        nb = self.bands.size if self.fit_mean else 0
        onehot = (self.band_index[:, None] == np.arange(nb)[None, :]).astype(float)
        A = np.hstack([onehot, self._harmonics(self.signal.time, f0)])
        theta = np.linalg.lstsq(A / sigma[:, None], y / sigma, rcond=None)[0]
        return (theta[:nb] if self.fit_mean else np.zeros(self.bands.size)), theta[nb:]

    def model(self, tf, band, f0):
        """The fitted series of the last call plus the offset of ``band`` (one of the labels) at frequency ``f0``,
        evaluated at times ``tf``.  O(N) host arithmetic, not part of the scan."""
        where = np.flatnonzero(self.bands == band)
        if where.size != 1:
            raise ValueError(f"{band!r} is not one of the bands {list(self.bands)}")
        offsets, coef = self._fit(f0)
        return TSeries(tf, offsets[where[0]] + self._harmonics(tf, f0) @ coef)

    def band_offsets(self, f0):
        """``{label: fitted offset}`` of the last call's model at frequency ``f0`` (zeros without ``fit_mean``)."""
        offsets, _ = self._fit(f0)
        return {label: float(o) for label, o in zip(self.bands.tolist(), offsets)}

    def window(self):
        raise NotImplementedError("MultibandGLS has no window: GLS.window calls the periodogram without band labels")

    def bootstrap(self, *args, **kwargs):
        raise NotImplementedError("MultibandGLS has no bootstrap: the batched replicate kernels compute GLS power only")

    fap = fal = bootstrap

    def batch(self, *args, **kwargs):
        raise NotImplementedError("MultibandGLS.batch is not implemented: the ragged-grid batch computes GLS power only")


BestCell = _collections.namedtuple("BestCell", "frequency fdot value harmonics index fdot_index")


class SpinSearch(object):
    """What ``HTest.search`` / ``ZTest.search`` return: the statistic over frequency x spin-down, reduced on the device.

    ``.frequency`` ``[nf]``, ``.fdot`` ``[nfd]``, ``.epoch``; ``.plane`` ``[nfd][nf]`` and ``.harmonics`` (the plane of
    m, ``HTest`` only), both None without ``want_plane``; ``.ridge`` (``FSeries``: per frequency the largest value over
    the rows, as ``np.nanargmax(plane, axis=0)`` picks it), ``.ridge_fdot`` (its fdot; NaN where no row is finite),
    ``.ridge_index`` (its row, -1 there), ``.ridge_harmonics`` (``HTest`` only); ``.best``, the largest cell as a
    ``BestCell(frequency, fdot, value, harmonics, index, fdot_index)`` - NaN and -1 where nothing is finite.
    """

    def __init__(self, frequency, fdot, epoch, out, nharm):
        self.frequency = frequency
        self.fdot = fdot
        self.epoch = epoch
        self.plane = out["plane"]
        self.harmonics = out["m_plane"]
        self.ridge = FSeries(frequency, out["ridge"])
        self.ridge_index = out["ridge_row"]
        self.ridge_fdot = np.where(self.ridge_index >= 0, fdot[np.maximum(self.ridge_index, 0)], np.nan)
        self.ridge_harmonics = out["ridge_m"]
        value, j, row, m = out["best"]
        found = j >= 0
        self.best = BestCell(float(frequency[j]) if found else np.nan, float(fdot[row]) if found else np.nan, value,
                             (m if nharm is None else nharm) if found else -1, j, row)


class _EventScan(object):
    """What ``HTest`` and ``ZTest`` share: the event list, its grid (the rule of ``GLS``) and the library calls."""

    MAX_HARMONICS = 20

    def __init__(self, fmin, fmax, n, harmonics, name, device):
        if isinstance(harmonics, bool) or harmonics != int(harmonics) or not 1 <= int(harmonics) <= self.MAX_HARMONICS:
            raise ValueError(f"{name} must be an integer 1 .. {self.MAX_HARMONICS}")
        self.fmin = fmin
        self.fmax = fmax
        self.n = n
        self.device = device
        self._nharm = int(harmonics)

    def _scan(self, signal, weights, want):
        """Sorts the events (weights follow), builds the grid, calls the library; ``(h, m, z2)`` as ``want`` asks."""
        t, w, events, (f0, delta, nf) = self._prepare(signal, weights)
        out = _cabi.htest_scan(t, w, f0, delta, nf, nharm=self._nharm, want=want,
                               device=_cabi.pick_device(self.device, None))
        self.signal = events
        self.weights = w
        return out

    def _prepare(self, signal, weights):
        """The sorted events and their weights as arrays, the events as a ``TSeries``, ``(f0, delta, nf)`` of the grid
        (``self.frequency``)."""
        if isinstance(signal, TSeries) or (hasattr(signal, "time") and hasattr(signal, "values")):
            t = np.asarray(signal.time, dtype=float)
        else:
            t = np.asarray(signal, dtype=float)
        if t.ndim != 1:
            raise ValueError("Only one-dimensional event lists are supported.")
        if t.size < 2:
            raise ValueError("At least two events are needed to build the frequency grid.")
        w = None
        if weights is not None:
            w = np.asarray(weights, dtype=float)
            if w.ndim != 1 or w.size != t.size:
                raise ValueError("Input arrays have incompatible lengths.")
        order = np.argsort(t, kind="stable")
        t = t[order]
        w = None if w is None else w[order]
        events = TSeries(t, assume_sorted=True)
        self.frequency = self._grid(events)
        f0, delta, nf = _cabi.grid_params(self.frequency)
        if nf < 2:   # a grid of one bin has no step of its own; any positive step rebuilds it
            delta = 1.0
        return t, w, events, (f0, delta, nf)

    def search(self, signal, weights=None, *, fdot, epoch=None, want_plane=True):
        """The statistic over the plane of trial frequencies (the grid of a plain call) and spin-down rates ``fdot``,
        with the phase ``f tau + fdot tau**2 / 2`` cycles, ``tau = t - epoch``: for a source whose frequency drifts
        during the observation.  The plane is reduced on the device; a ``SpinSearch`` comes back.

        fdot: one-dimensional array of finite values, any order (a row each).
        epoch: where ``f`` is the frequency; None: the earliest event.
        want_plane: False leaves the plane (and its harmonics) on the device: ridge and best cell only.
        """
        fdot = np.array(fdot, dtype=float)
        if fdot.ndim != 1 or fdot.size < 1:
            raise ValueError("fdot must be a one-dimensional array with at least one entry.")
        if not np.all(np.isfinite(fdot)):
            raise ValueError("fdot must be finite.")
        t, w, events, (f0, delta, nf) = self._prepare(signal, weights)
        epoch = float(t[0]) if epoch is None else float(epoch)
        if not np.isfinite(epoch):
            raise ValueError("epoch must be finite.")
        with_m = self._stat == "h"
        want = ["ridge", "ridge_row", "best"] + (["ridge_m"] if with_m else [])
        if want_plane:
            want += ["plane"] + (["m_plane"] if with_m else [])
        out = _cabi.htest_fdot_scan(t, w, f0, delta, nf, fdot, epoch, nharm=self._nharm, stat=self._stat, want=want,
                                    device=_cabi.pick_device(self.device, None))
        self.signal = events
        self.weights = w
        return SpinSearch(self.frequency, fdot, epoch, out, None if with_m else self._nharm)

    def _grid(self, events):
        """The grid of ``GLS._grid`` with the events as time stamps."""
        df = 1.0 / events.baseline / self.n
        fmin = 0.5 * df if self.fmin is None else self.fmin
        fmax = 0.5 / events.median_dt if self.fmax is None else self.fmax
        return np.arange(fmin, fmax + df, df)

    def copy(self):
        return _copy.deepcopy(self)


class HTest(_EventScan):
    """H-test periodogram of an event list (de Jager, Raubenheimer & Swanepoel 1989, A&A 221, 180): the search for
    pulsations in photon arrival times when the pulse shape is not known.  The reference has no such class -
    **parity unpinned by the reference**.

    With ``theta_i = 2 pi f (t_i - t_0)``, ``t_0`` the earliest event, and photon weights ``w_i`` (1 without;
    Kerr 2011, ApJ 732, 38), ``C_k = sum w_i cos(k theta_i)``, ``S_k = sum w_i sin(k theta_i)``,

        ``Z2_m(f) = (2 / sum w_i**2) sum_{k <= m} (C_k**2 + S_k**2)``   (Buccheri et al. 1983, A&A 128, 245),
        ``H(f) = max_{1 <= m <= max_harmonics} (Z2_m - 4 m + 4)``,

    and ``harmonics(f)`` is the lowest ``m`` that reaches the maximum.  The grid is that of ``GLS`` with the events
    as time stamps.  Its default ``fmin``, half a cycle per baseline, sits where the finite window leaks into every
    ``Z2_m`` - events spread evenly over the baseline give ``H`` of about ``8 N / pi**2`` in the first bin - so a
    search should set ``fmin`` to a few cycles per baseline.  Evaluated by ``csrc/htest.hip``; nothing here
    computes a periodogram on the CPU.

    ``signal``: a ``TSeries`` contributes its time stamps (its values are not used, as in ``GregoryLoredo``); a raw
    one-dimensional array IS the list of arrival times.  Events are sorted before the grid is built and
    ``weights`` follow their events.

    Parameters
    ----------
    fmin, fmax, n: as ``GLS``.
    max_harmonics: int, keyword-only, optional
        Largest number of harmonics tried, 1 .. 20 (default 20, as in the paper).
    device: int, keyword-only, optional

    After a call: ``.frequency``, ``.periodogram`` (H), ``.harmonics`` (int array), ``.z2`` (``FSeries`` of Z2 at
    ``max_harmonics``), ``.signal`` (the sorted events) and ``.weights``.  ``.search(signal, weights, fdot=...)`` covers
    the frequency - spin-down plane (``csrc/htest_fdot.hip``) and returns a ``SpinSearch``.
    """

    def __init__(self, fmin=None, fmax=None, n=5, *, max_harmonics=20, device=None):
        super().__init__(fmin, fmax, n, max_harmonics, "max_harmonics", device)
        self._stat = "h"
        self.max_harmonics = self._nharm

    def __call__(self, signal, weights=None):
        h, m, z2 = self._scan(signal, weights, ("h", "m", "z2"))
        self.harmonics = m
        self.z2 = FSeries(self.frequency, z2)
        self.periodogram = FSeries(self.frequency, h)
        return self.periodogram

    @staticmethod
    def fap(h):
        """Single-trial tail probability of H, ``min(1, exp(-0.4 H))`` (de Jager & Busching 2010, A&A 517, L9)."""
        return np.minimum(1.0, np.exp(-0.4 * np.asarray(h, dtype=float)))


class ZTest(_EventScan):
    """Z2_n periodogram of an event list (Buccheri et al. 1983, A&A 128, 245) with a fixed number of harmonics;
    ``nharm=1`` is the Rayleigh test.  The reference has no such class - **parity unpinned by the reference**.
    Definitions, grid, inputs and the advice on ``fmin`` as for ``HTest``; evaluated by ``csrc/htest.hip``.

    Parameters
    ----------
    fmin, fmax, n: as ``GLS``.
    nharm: int, keyword-only, optional
        Harmonics summed, 1 .. 20 (default 2).
    device: int, keyword-only, optional

    After a call: ``.frequency``, ``.periodogram``, ``.signal`` (the sorted events) and ``.weights``.  ``.search`` as for
    ``HTest``, with Z2 as the value of a cell.
    """

    def __init__(self, fmin=None, fmax=None, n=5, *, nharm=2, device=None):
        super().__init__(fmin, fmax, n, nharm, "nharm", device)
        self._stat = "z2"
        self.nharm = self._nharm

    def __call__(self, signal, weights=None):
        _, _, z2 = self._scan(signal, weights, ("z2",))
        self.periodogram = FSeries(self.frequency, z2)
        return self.periodogram

    def fap(self, z):
        """Single-trial tail probability of Z2: chi-squared with ``2 nharm`` degrees of freedom."""
        from scipy.stats import chi2
        return chi2.sf(z, 2 * self.nharm)
