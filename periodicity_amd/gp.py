"""Gaussian-process likelihood scans, computed on MI355X.

The reference's ``gp.py`` (``CeleriteModeler``, ``HarmonicGP``, ``BrownianGP``) evaluates one celerite likelihood per
hyper-parameter vector - ``gp.compute(...)`` then ``gp.log_likelihood(y)`` - from L-BFGS and from ``emcee``.  Here the
same likelihood is evaluated for many vectors in one call (``csrc/gp.hip``: a lane per vector, the O(N J^2) celerite
recursion of Foreman-Mackey et al. 2017, AJ 154, 220): ``CeleriteLikelihood`` for an arbitrary list of kernels - an
MCMC ensemble, a nested sampler's live points - and ``HarmonicGP.scan`` / ``BrownianGP.scan`` for a grid of trial
periods times a grid of nuisance parameters, folded per period into a profile and a marginal log-likelihood: what one
looks at before starting a sampler, and where the multimodality in period shows that an optimiser hides.

Nothing in this module evaluates a likelihood on the CPU: numpy sorts the curve, builds the celerite coefficients of
every candidate (``sho_terms``, ``rotation_terms``, ``brownian_terms``: the standard SHO algebra, written out below) and
labels what comes back.  Samplers, gradients, prediction and the PSD are out of scope.
"""
import itertools

import numpy as np

from . import _cabi
from .core import FSeries, TSeries
from .spectral import _as_tseries

__all__ = ["sho_terms", "rotation_terms", "brownian_terms", "device_coefficients", "CeleriteLikelihood", "GPResult",
           "GPScan", "HarmonicGP", "BrownianGP"]

MAX_CELLS = 65535


# ---- term builders: celerite coefficients (a, b, c, d) of k(D) = sum e^{-c|D|} (a cos dD + b sin d|D|) ---------------
def _broadcast(*values):
    arrays = np.broadcast_arrays(*[np.asarray(v, dtype=float) for v in values])
    if arrays[0].ndim > 1:
        raise ValueError("The parameters of a term must be scalars or one-dimensional.")
    return [np.atleast_1d(a).astype(float) for a in arrays]


def sho_terms(S0=None, w0=None, Q=None, *, sigma=None, tau=None, rho=None):
    """A stochastically driven damped harmonic oscillator, by ``(S0, w0, Q)`` or by ``(sigma, tau, rho)`` with
    ``w0 = 2 pi / rho``, ``Q = pi tau / rho``, ``S0 = sigma^2 / (w0 Q)``.  Vectorised; returns ``[M][J][4]``:

    * ``Q > 1/2`` - one complex term: ``f = sqrt(4 Q^2 - 1)``, ``a = S0 w0 Q``, ``b = a / f``, ``c = w0 / 2Q``, ``d = c f``;
    * ``Q < 1/2`` - two real terms: ``f = sqrt(1 - 4 Q^2)``, ``a+- = S0 w0 Q (1 +- 1/f) / 2``, ``c+- = (w0 / 2Q)(1 -+ f)``.

    Every ``Q`` of one call lies on the same side of 1/2 (``J`` is one number); ``Q = 1/2`` is refused."""
    by_sigma = sigma is not None or tau is not None or rho is not None
    if by_sigma:
        if S0 is not None or w0 is not None or Q is not None or sigma is None or tau is None or rho is None:
            raise ValueError("Give (S0, w0, Q) or (sigma, tau, rho).")
        sigma, tau, rho = _broadcast(sigma, tau, rho)
        w0 = 2 * np.pi / rho
        Q = np.pi * tau / rho
        S0 = sigma ** 2 / (w0 * Q)
    else:
        if S0 is None or w0 is None or Q is None:
            raise ValueError("Give (S0, w0, Q) or (sigma, tau, rho).")
        S0, w0, Q = _broadcast(S0, w0, Q)
    if not (np.all(np.isfinite(S0)) and np.all(np.isfinite(w0)) and np.all(np.isfinite(Q)) and np.all(w0 > 0)
            and np.all(Q > 0)):
        raise ValueError("S0, w0 and Q must be finite, w0 and Q positive.")
    if np.any(Q == 0.5):
        raise ValueError("Q = 1/2 (critical damping) has no celerite form.")
    under = Q > 0.5
    if not (np.all(under) or not np.any(under)):
        raise ValueError("Every Q of one call must lie on the same side of 1/2.")
    amp = S0 * w0 * Q
    rate = w0 / (2 * Q)
    zero = np.zeros_like(amp)
    if np.all(under):
        f = np.sqrt(4 * Q ** 2 - 1)
        return np.stack([amp, amp / f, rate, rate * f], axis=-1)[:, None, :]
    f = np.sqrt(1 - 4 * Q ** 2)
    plus = np.stack([0.5 * amp * (1 + 1 / f), zero, rate * (1 - f), zero], axis=-1)
    minus = np.stack([0.5 * amp * (1 - 1 / f), zero, rate * (1 + f), zero], axis=-1)
    return np.stack([plus, minus], axis=1)


def rotation_terms(sigma, period, Q0, dQ, f):
    """Two underdamped oscillators at ``period`` and ``period / 2`` (celerite2's ``RotationTerm``, the reference's
    ``HarmonicGP`` kernel): ``amp = sigma^2 / (1 + f)``; ``Q1 = 1/2 + Q0 + dQ``, ``w1 = 4 pi Q1 / (period sqrt(4 Q1^2 -
    1))``, ``S1 = amp / (w1 Q1)``; ``Q2 = 1/2 + Q0``, ``w2 = 8 pi Q2 / (period sqrt(4 Q2^2 - 1))``, ``S2 = f amp / (w2
    Q2)``.  Always ``J = 2``, and ``k(0) = sigma^2``.  Returns ``[M][2][4]``."""
    sigma, period, Q0, dQ, f = _broadcast(sigma, period, Q0, dQ, f)
    if not (np.all(period > 0) and np.all(Q0 > 0) and np.all(dQ >= 0) and np.all(f >= 0)):
        raise ValueError("period and Q0 must be positive, dQ and f not negative.")
    amp = sigma ** 2 / (1 + f)
    Q1 = 0.5 + Q0 + dQ
    w1 = 4 * np.pi * Q1 / (period * np.sqrt(4 * Q1 ** 2 - 1))
    Q2 = 0.5 + Q0
    w2 = 8 * np.pi * Q2 / (period * np.sqrt(4 * Q2 ** 2 - 1))
    return np.concatenate([sho_terms(amp / (w1 * Q1), w1, Q1), sho_terms(f * amp / (w2 * Q2), w2, Q2)], axis=1)


BROWNIAN_Q = 0.01


def brownian_terms(sigma, tau, period, mix):
    """The reference's ``BrownianTerm`` (``gp.py:487-497``): an oscillator ``sho_terms(sigma=sigma sqrt(mix), tau=tau,
    rho=period)`` plus an overdamped one of ``Q = 0.01`` whose slow mode decays on ``tau`` and carries ``(1 - mix)
    sigma^2``: ``f = sqrt(1 - 4 Q^2)``, ``w0 = 2 Q / (tau (1 - f))``, ``S0 = (1 - mix) sigma^2 / (w0 Q (1 + 1/f) / 2)``.
    The oscillator must be underdamped (``pi tau / period > 1/2``: the reference's prior has ``tau >= period``), so
    ``J = 3``.  ``k(0) = sigma^2 (1 - (1 - mix)(1 - f) / (1 + f))``: ``sigma^2`` to 1e-4.  Returns ``[M][3][4]``."""
    sigma, tau, period, mix = _broadcast(sigma, tau, period, mix)
    if not (np.all(tau > 0) and np.all(period > 0) and np.all(mix >= 0) and np.all(mix <= 1)):
        raise ValueError("tau and period must be positive, mix in [0, 1].")
    if not np.all(np.pi * tau / period > 0.5):
        raise ValueError("The periodic part must be underdamped: pi tau / period > 1/2.")
    f = np.sqrt(1 - 4 * BROWNIAN_Q ** 2)
    w0 = 2 * BROWNIAN_Q / (tau * (1 - f))
    S0 = (1 - mix) * sigma ** 2 / (0.5 * w0 * BROWNIAN_Q * (1 + 1 / f))
    return np.concatenate([sho_terms(sigma=sigma * np.sqrt(mix), tau=tau, rho=period),
                           sho_terms(S0, w0, np.full_like(w0, BROWNIAN_Q))], axis=1)


def _check_terms(terms):
    terms = np.asarray(terms, dtype=float)
    if terms.ndim == 2:
        terms = terms[None]
    if terms.ndim != 3 or terms.shape[2] != 4 or terms.shape[0] < 1 or terms.shape[1] < 1:
        raise ValueError("terms must have the shape [M][J][4] of celerite coefficients (a, b, c, d).")
    return terms


def device_coefficients(terms):
    """``[M][J][4]`` of ``(a, b, c, d)`` as the library takes them: ``(a, b, c, nu = d / 2 pi)``, so that the kernel
    reduces a phase in cycles before it meets 2 pi."""
    coeff = np.array(_check_terms(terms), dtype=np.float64, order="C")
    coeff[:, :, 3] = coeff[:, :, 3] / (2 * np.pi)
    return coeff


# ---- the curve ----------------------------------------------------------------------------------------------------
class GPResult(object):
    """``log_likelihood``, ``mean`` and ``status`` (0, or the 1-based sample at which a candidate's matrix stopped being
    positive definite: its likelihood is -inf), each ``[M]``."""

    def __init__(self, log_likelihood, mean, status):
        self.log_likelihood = log_likelihood
        self.mean = mean
        self.status = status


class CeleriteLikelihood(object):
    """The log-likelihood of one curve under many celerite kernels.

    Parameters
    ----------
    signal: TSeries, array-like or a pair ``(t, y)`` of arrays
        A pair is sorted by time as ``TSeries`` sorts (stably), ``err`` with it; ``.tau = t - t[0]`` is what the device
        sees.  A ``TSeries`` is sorted already and ``err`` is taken in its order.
    err: array-like, optional
        Measurement uncertainties (their squares are the diagonal); default none.
    device: int, keyword-only, optional
    """

    def __init__(self, signal, err=None, *, device=None):
        pair = isinstance(signal, (tuple, list)) and len(signal) == 2 and np.ndim(signal[0]) == 1
        if pair:   # raw (t, y): sorted here, stably as TSeries does, and the uncertainties with them
            t, y = np.asarray(signal[0], dtype=float), np.asarray(signal[1], dtype=float)
            if y.shape != t.shape:
                raise ValueError("Input arrays have incompatible lengths.")
        else:      # a TSeries has sorted its arrays already: err is in that order
            signal = _as_tseries(signal)
            t, y = np.asarray(signal.time, dtype=float), np.asarray(signal.values, dtype=float)
        if t.ndim != 1 or t.size < 1:
            raise ValueError("At least one sample is needed.")
        err = np.zeros(t.size) if err is None else np.asarray(err, dtype=float)
        if err.ndim != 1 or err.size != t.size:
            raise ValueError("Input arrays have incompatible lengths.")
        if pair:
            order = np.argsort(t, kind="stable")
            t, y, err = t[order], y[order], err[order]
            signal = TSeries(t, y, assume_sorted=True)
        if not (np.all(np.isfinite(t)) and np.all(np.isfinite(y)) and np.all(np.isfinite(err))):
            raise ValueError("Times, values and uncertainties must be finite.")
        self.signal = signal
        self.t = t
        self.y = y
        self.err = err
        self.tau = t - t[0]
        self.var = err ** 2
        self.device = device

    def _device(self):
        return _cabi.pick_device(self.device, None)

    def __call__(self, terms, jitter=0.0, mean=None):
        """``terms``: ``[M][J][4]`` celerite coefficients ``(a, b, c, d)`` (or ``[J][4]`` for one kernel); ``jitter``: a
        variance added to every ``err ** 2``, a scalar or ``[M]``; ``mean``: a scalar or ``[M]``, or None to profile it out
        per candidate (``.mean`` is then the maximum-likelihood mean).  Returns a ``GPResult``."""
        coeff = device_coefficients(terms)
        if mean is None:   # the curve is centred first: the profiled mean is then small beside the scatter
            centre = float(np.mean(self.y))
            ll, mu, status = _cabi.gp_loglike(self.tau, self.y - centre, self.var, coeff, jitter, None, fit_mean=True,
                                              device=self._device())
            return GPResult(ll, mu + centre, status)
        mean = np.asarray(mean, dtype=float)
        if mean.ndim == 0:
            ll, _, status = _cabi.gp_loglike(self.tau, self.y - float(mean), self.var, coeff, jitter, None,
                                             device=self._device())
            return GPResult(ll, np.full(coeff.shape[0], float(mean)), status)
        if mean.shape != (coeff.shape[0],):
            raise ValueError("mean must be a scalar or one value per candidate.")
        ll, mu, status = _cabi.gp_loglike(self.tau, self.y, self.var, coeff, jitter, mean, device=self._device())
        return GPResult(ll, mu, status)


# ---- period scans -------------------------------------------------------------------------------------------------
class GPScan(object):
    """What a period scan returns: ``period`` ``[np]``, ``log_likelihood`` (the profile: per period the largest
    likelihood over the nuisance cells; NaN where no cell is positive definite), ``marginal`` (ln of the cells' mean
    likelihood), ``cell`` (int32, -1), ``mean`` (of the best cell), ``cube`` ``[np][nq]`` or None, ``best`` (a dict),
    ``periodogram`` (an ``FSeries`` of the profile over ``1 / period``), and ``params(i)``."""

    def __init__(self, period, names, cells, out, fixed):
        self.period = period
        self.names = names
        self.cells = cells                      # [nq][len(names)]
        self.log_likelihood = out["profile"]
        self.marginal = out["marginal"]
        self.cell = out["cell"]
        self.mean = out["mean"]
        self.cube = out["cube"]
        self.fixed = fixed
        value, at, cell = out["best"]
        self.best = None
        if at >= 0:
            self.best = dict(period=float(period[at]), log_likelihood=value, index=at, cell=cell, mean=float(self.mean[at]),
                             **self.params(at), **fixed)
        self.periodogram = FSeries(1.0 / period, self.log_likelihood)

    def params(self, i):
        """The nuisance values of period ``i``'s best cell (a dict; NaN where the period has none)."""
        cell = int(self.cell[i])
        values = self.cells[cell] if cell >= 0 else np.full(len(self.names), np.nan)
        return {name: float(v) for name, v in zip(self.names, values)}


class _PeriodScanGP(CeleriteLikelihood):
    """A curve and the reference's defaults for the amplitude and the jitter (``gp.py``: ``sigma = np.std(y)``,
    ``jitter = min(err) ** 2``)."""

    names = ()

    def __init__(self, signal, err, *, device=None):
        super().__init__(signal, err, device=device)
        self.sigma = float(np.std(self.y))
        self.jitter = float(np.min(self.err) ** 2)
        self.mean = float(np.mean(self.y))

    def _scan(self, periods, lists, sigma, jitter, fit_mean, want_cube, terms):
        """``terms(sigma, period, cells)``: the ``[M][J][4]`` coefficients of the grid's candidates, ``period`` ``[M]`` and
        ``cells`` ``[M][len(lists)]`` row by row."""
        periods = np.asarray(periods, dtype=float)
        if periods.ndim != 1 or periods.size < 1 or not np.all(np.isfinite(periods)) or not np.all(periods > 0):
            raise ValueError("periods must be a one-dimensional list of positive numbers.")
        lists = [np.atleast_1d(np.asarray(v, dtype=float)) for v in lists]
        if any(v.ndim != 1 or v.size < 1 or not np.all(np.isfinite(v)) for v in lists):
            raise ValueError("Every nuisance list must be a non-empty one-dimensional list of finite numbers.")
        nq = int(np.prod([v.size for v in lists]))
        if nq > MAX_CELLS:
            raise ValueError(f"The nuisance lists span {nq} cells, at most {MAX_CELLS} fit.")
        sigma = self.sigma if sigma is None else float(sigma)
        jitter = self.jitter if jitter is None else float(jitter)
        if not (sigma > 0 and np.isfinite(sigma) and jitter >= 0 and np.isfinite(jitter)):
            raise ValueError("sigma must be positive and jitter not negative.")
        cells = np.array(list(itertools.product(*lists)), dtype=float)   # [nq][k], the last list fastest
        period = np.repeat(periods, nq)
        coeff = device_coefficients(terms(sigma, period, np.tile(cells, (periods.size, 1))))
        centre = self.mean
        out = _cabi.gp_scan(self.tau, self.y - centre, self.var, coeff, periods.size, jitter, None, fit_mean=fit_mean,
                            want_cube=want_cube, device=self._device())
        out["mean"] = out["mean"] + centre
        return GPScan(periods, self.names, cells, out, dict(sigma=sigma, jitter=jitter))


class HarmonicGP(_PeriodScanGP):
    """The reference's ``HarmonicGP`` (a ``RotationTerm`` kernel; parameters ``sigma, period, Q0, dQ, f, jitter, mean``)
    as a scan over trial periods."""

    names = ("Q0", "dQ", "f")

    def scan(self, periods, Q0, dQ, f, sigma=None, jitter=None, fit_mean=True, want_cube=False):
        """The likelihood of every ``(period, Q0, dQ, f)`` of ``periods`` times the Cartesian product of the three lists
        (at most 65535 cells), folded per period.  ``fit_mean``: profile the mean out per cell, else it is the curve's
        mean.  Returns a ``GPScan``."""
        return self._scan(periods, [Q0, dQ, f], sigma, jitter, fit_mean, want_cube,
                          lambda sigma, period, cells: rotation_terms(sigma, period, cells[:, 0], cells[:, 1], cells[:, 2]))


class BrownianGP(_PeriodScanGP):
    """The reference's ``BrownianGP`` (its ``BrownianTerm``; parameters ``sigma, tau, period, mix, jitter, mean``) as a
    scan over trial periods."""

    names = ("tau", "mix")

    def scan(self, periods, tau, mix, sigma=None, jitter=None, fit_mean=True, want_cube=False, tau_in_periods=False):
        """As ``HarmonicGP.scan`` over ``(period, tau, mix)``; with ``tau_in_periods`` the list is ``tau / period`` (the
        reference's prior draws ``tau = period 10^u``) and ``params(i)["tau"]`` is that ratio."""
        def terms(sigma, period, cells):
            return brownian_terms(sigma, cells[:, 0] * period if tau_in_periods else cells[:, 0], period, cells[:, 1])

        return self._scan(periods, [tau, mix], sigma, jitter, fit_mean, want_cube, terms)
