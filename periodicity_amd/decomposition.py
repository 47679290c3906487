"""Empirical mode decompositions on the device: ``EMD`` and ``CEEMDAN`` of the reference's ``decomposition.py``, and
``envelopes`` (its ``TSeries.get_envelope``).

One workgroup sifts one row from the signal down to its residue inside a single kernel (``csrc/emd.hip``, DESIGN.md
4.1s); ``EMD.batch`` decomposes many rows of one length in one launch, and ``CEEMDAN`` keeps its ensemble of noise modes on
the device and runs each stage - noisy rows, their first modes, the ensemble mean - there.  The reference's ``TSeries``
needs xarray, so parity with it is unpinned: the definition is restated from its calls to scipy and numpy and checked
against those (``tests/emd_oracle.py``).

Out of scope: ``LMD``, ``VMD``, ``timefrequency.HHT`` and ``CompositeSpectrum``, rows of different lengths in one batch,
and ``devices=``.
"""
import warnings

import numpy as np

from . import _cabi
from .core import TSeries

__all__ = ["EMD", "CEEMDAN", "envelopes"]


def _series(signal):
    return signal if isinstance(signal, TSeries) else TSeries(values=signal)


def _cap(max_modes):
    """(modes asked of the device, whether the caller set no bound): None and infinity mean the device's 64."""
    if max_modes is None or max_modes == np.inf:
        return _cabi.EMD_MAX_MODES, True
    max_modes = int(max_modes)
    if max_modes > _cabi.EMD_MAX_MODES:
        raise ValueError(f"at most {_cabi.EMD_MAX_MODES} modes are kept on the device (got {max_modes})")
    return max_modes, False


def envelopes(signal, pad_width=0):
    """``(upper, lower)``: the not-a-knot cubic splines through the maxima and through the minima of ``signal``, with
    ``pad_width`` extrema reflected about either end.  Raises ValueError where the reference's ``get_envelope`` does."""
    signal = _series(signal)
    out = _cabi.emd_sift(signal.time, signal.values, pad_width=pad_width)
    if out["monotonic"]:
        if min(out["maxima"].size, out["minima"].size) < pad_width:
            raise ValueError("Signal doesn't have enough extrema for padding.")
        raise ValueError("Signal doesn't have enough extrema for envelope interpolation.")
    return TSeries(signal.time, out["upper"], assume_sorted=True), TSeries(signal.time, out["lower"], assume_sorted=True)


class EMD(object):
    """Empirical Mode Decomposition (Rilling, Flandrin & Goncalves 2003), the reference's stopping rule.

    Parameters
    ----------
    max_iter: int, optional
        Maximum number of sifting iterations per mode (the default is 2000; at most 10^6).
    pad_width: int, optional
        Number of extrema to repeat on either side of the signal while interpolating envelopes (the default is 2).
    theta_1, theta_2, alpha: float, optional
        ``sigma = |mean / amplitude|`` of the envelopes must stay under ``theta_1`` on all but a fraction ``alpha`` of
        the samples and under ``theta_2`` everywhere.
    device: int, optional
        The GPU (default: the process default).
    """

    def __init__(self, max_iter=2000, pad_width=2, theta_1=0.05, theta_2=0.50, alpha=0.05, *, device=None):
        self.max_iter = max_iter
        self.pad_width = pad_width
        self.theta_1 = theta_1
        self.theta_2 = theta_2
        self.alpha = alpha
        self.device = device

    def _params(self):
        return dict(max_iter=self.max_iter, pad_width=self.pad_width, theta_1=self.theta_1, theta_2=self.theta_2,
                    alpha=self.alpha)

    def _run(self, time, rows, max_modes):
        cap, unbounded = _cap(max_modes)
        B, n = rows.shape
        if n < 4 or cap <= 0:   # (the reference: no sift below four samples)
            return [[] for _ in range(B)], rows.copy(), np.zeros((B, 0), dtype=np.int64), np.zeros(B, dtype=np.int64)
        out = _cabi.emd_batch(time, rows, max_modes=cap, device=self.device, **self._params())
        if unbounded and np.any(out["flags"] & 2):
            warnings.warn(f"EMD stopped at the device's {cap} modes with a residue that is not monotonic",
                          RuntimeWarning, stacklevel=3)
        modes = [[out["modes"][b, k].copy() for k in range(int(out["n_modes"][b]))] for b in range(B)]
        return modes, out["residue"], out["sifts"], out["flags"]

    def __call__(self, signal, max_modes=None):
        """The list of modes of ``signal`` (``TSeries``); also sets ``signal``, ``modes``, ``residue``, ``n_modes`` as the
        reference does, and ``sifts`` (updates applied to each mode) and ``flags``.

        max_modes: int, optional
            If given, stops the decomposition after this number of modes; without it the device's 64 (a warning says so
            if they are reached).
        """
        signal = _series(signal)
        time = np.asarray(signal.time, dtype=np.float64)
        modes, residue, sifts, flags = self._run(time, np.asarray(signal.values, dtype=np.float64)[None, :], max_modes)
        self.signal = signal
        self.modes = [TSeries(signal.time, m, assume_sorted=True) for m in modes[0]]
        self.residue = TSeries(signal.time, residue[0], assume_sorted=True)
        self.n_modes = len(self.modes)
        self.sifts = [int(s) for s in sifts[0, :self.n_modes]]
        self.flags = int(flags[0])
        return self.modes

    def batch(self, signals, max_modes=None):
        """Decomposes many curves of one length on one time axis in a single launch: ``signals`` is a 2-D array (time
        ``arange(N)``) or a list of ``TSeries`` that share their times.  Returns the per-row lists of modes and sets
        ``batch_modes``, ``batch_residues`` (list of ``TSeries``), ``batch_sifts`` and ``batch_flags``."""
        if isinstance(signals, np.ndarray):
            rows = np.asarray(signals, dtype=np.float64)
            if rows.ndim != 2:
                raise ValueError("a batch is a 2-D array: one row per curve")
            time = np.arange(rows.shape[1])
        else:
            signals = [_series(s) for s in signals]
            if not signals:
                raise ValueError("an empty batch")
            time = signals[0].time
            for s in signals[1:]:
                if s.size != signals[0].size or not np.array_equal(s.time, time):
                    raise ValueError("the curves of a batch must share one time axis (rows of different lengths are "
                                     "out of scope)")
            rows = np.stack([np.asarray(s.values, dtype=np.float64) for s in signals])
        modes, residue, sifts, flags = self._run(np.asarray(time, dtype=np.float64), rows, max_modes)
        self.batch_modes = [[TSeries(time, m, assume_sorted=True) for m in row] for row in modes]
        self.batch_residues = [TSeries(time, r, assume_sorted=True) for r in residue]
        self.batch_sifts = [[int(s) for s in sifts[b, :len(row)]] for b, row in enumerate(modes)]
        self.batch_flags = flags
        return self.batch_modes


class CEEMDAN(object):
    """Complete Ensemble Empirical Mode Decomposition with Adaptive Noise (Torres et al. 2011; Colominas et al. 2014),
    the reference's control flow line for line.

    Parameters
    ----------
    epsilon: float, optional
        Normalized standard deviation of the added Gaussian noise (the default is 0.2).
    ensemble_size: int, optional
        Number of realizations averaged for each IMF (the default is 50).
    min_energy: float, optional
        Stopping criterium for the energy contribution of the residue.
    random_seed: int, optional
        Seed of ``np.random.default_rng``; the noise is the reference's bit for bit for the same seed.
    cores: accepted and unused (the ensemble runs on the device).
    device: int, optional
        The GPU (default: the process default).
    Further keywords go to ``EMD``.
    """

    def __init__(self, epsilon=0.2, ensemble_size=50, min_energy=0.0, random_seed=None, cores=None, *, device=None,
                 **kwargs):
        self.epsilon = epsilon
        self.ensemble_size = ensemble_size
        self.min_energy = min_energy
        self.cores = cores
        self.device = device
        self.emd = EMD(device=device, **kwargs)
        self.rng = np.random.default_rng(random_seed)

    def __call__(self, signal, max_modes=None, progress=False):
        """The list of IMFs of ``signal``; sets ``signal``, ``modes``, ``residue``, ``n_modes`` as the reference does,
        and ``trajectories``: per stage the ``(n_modes[E], sifts[E])`` of the realisations' first-mode decompositions
        (``noise_trajectories``: the same of the noise decomposition).  ``progress`` is accepted and unused."""
        signal = _series(signal)
        if max_modes is None:
            max_modes = np.inf
        time = np.asarray(signal.time, dtype=np.float64)
        x = np.asarray(signal.values, dtype=np.float64)
        E = self.ensemble_size
        sigma_x = np.std(x)

        # Creates the noise realizations, one draw of N per realisation, in order; their modes stay on the device
        noise = np.stack([self.rng.standard_normal(x.size) for _ in range(E)])
        plan = _cabi.CeemdanPlan(time, noise, device=self.device, **self.emd._params())
        try:
            if np.any(plan.flags & 2):
                warnings.warn("a noise realisation has more modes than the device keeps", RuntimeWarning, stacklevel=2)
            self.noise_trajectories = (plan.n_modes.copy(), plan.sifts.copy())
            first = plan.noise_mode(0)
            self.trajectories = []
            imfs = []
            residue = x / sigma_x
            while len(imfs) < max_modes:
                k = len(imfs)
                # Averages the ensemble of trials for the next mode
                beta = np.zeros(E)
                for i in np.flatnonzero(plan.n_modes > k):
                    b = self.epsilon * np.std(residue)
                    if k == 0:
                        b /= np.std(first[i])
                    beta[i] = b
                mu, n_first, sifts, _ = plan.stage(residue, k, beta)
                self.trajectories.append((n_first, sifts))
                imfs.append(residue - mu)
                residue = mu.copy()

                # Checks stopping criteria (if the residue is an IMF or too small)
                if np.var(residue) < self.min_energy:
                    break
                residue_imfs = self.emd(TSeries(signal.time, residue, assume_sorted=True))
                if len(residue_imfs) <= 1:
                    if len(imfs) < max_modes and len(residue_imfs) == 1:
                        imfs.append(residue)
                    break
        finally:
            plan.close()

        # Undoes the initial normalization
        for i in range(len(imfs)):
            imfs[i] = imfs[i] * sigma_x
        self.signal = signal
        self.modes = [TSeries(signal.time, m, assume_sorted=True) for m in imfs]
        self.residue = signal - sum(self.modes)
        self.n_modes = len(imfs)
        return self.modes

    def postprocessing(self):
        """Sets ``c_modes`` and ``c_residue``: each mode sifted once more together with what the previous one left."""
        ck = self.emd(self.modes[0], max_modes=1)[0]
        c_imfs = [ck]
        qk = self.modes[0] - ck
        for k in range(1, self.n_modes):
            Dk = qk + self.modes[k]
            modes = self.emd(Dk, max_modes=1)
            if len(modes) > 0:
                ck = modes[0]
            else:
                c_imfs.append(self.modes[k])
                break
            qk = Dk - ck
            c_imfs.append(ck)
        self.c_residue = sum(self.modes) + self.residue - sum(c_imfs)
        self.c_modes = c_imfs

    @staticmethod
    def _orthogonality(modes):
        orth = np.eye(len(modes))   # (each pair once: symmetric with a unit diagonal to the last bit)
        for i in range(len(modes)):
            for j in range(i + 1, len(modes)):
                orth[i, j] = orth[j, i] = np.corrcoef(modes[i].values, modes[j].values)[0, 1]
        return orth

    @property
    def orthogonality_matrix(self):
        """Pearson correlation of every pair of modes (the reference reads a ``self.imfs`` it never sets)."""
        return self._orthogonality(self.modes)

    @property
    def c_orthogonality_matrix(self):
        return self._orthogonality(self.c_modes)
