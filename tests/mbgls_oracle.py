"""Test-local oracle of the shared-phase multiband generalised Lomb-Scargle periodogram (plain numpy; imports nothing
from ``periodicity_amd``).  The reference has no such class - PARITY UNPINNED BY THE REFERENCE: what is restated here is
the published statistic (VanderPlas & Ivezic 2015, the ``Nbase = H, Nband = 0`` model) on the weights and normalisations
of ``GLS``.

The FULL ``(B + 2H)`` design is built - one indicator column per band, then ``cos(k theta)``, ``sin(k theta)`` evaluated
directly per (sample, frequency) pair - and solved by Cholesky: no Schur step, no recurrence, no product-to-sum rule, so
the oracle shares no shortcut with the kernel it checks."""
import numpy as np

import mhgls_oracle as mo

CHUNK = 256   # frequencies per block of the dense evaluation, unless the caller names another
COND_LIMIT = 1e6   # bins compared in value: cond(M) <= COND_LIMIT (M is nearly singular at the lowest few frequencies)
SEEDS = {12: 2, 31: 3, 64: 4, 65: 5, 200: 6, 1000: 7}   # 64 / 65 straddle the 64-sample chunk of the rotation tables


def with_labels(t, y, err, n_bands, seed):
    """Random labels (every band holds at least one sample) and an offset of 0.5 per band: ``(t, y, err, band)``."""
    n = t.size
    rng = np.random.default_rng(seed + 100)
    band = rng.integers(0, n_bands, n)
    band[:n_bands] = np.arange(n_bands)
    rng.shuffle(band)
    return t, y + 0.5 * band, err, band


def curve(n, n_bands, seed=None):
    """The test curve of size ``n`` in ``n_bands`` bands: ``mhgls_oracle.curve`` plus the labels and offsets of
    ``with_labels``.  ``seed``: for a size outside ``SEEDS``."""
    seed = SEEDS[n] if seed is None else seed
    return with_labels(*mo.curve(n, seed), n_bands, seed)


def long_curve(n_bands=3, seed=31):
    """``mhgls_oracle.long_curve`` (3000 days at a Julian-date offset, period 0.0031 days) in ``n_bands`` bands."""
    return with_labels(*mo.long_curve(seed=seed), n_bands, seed)


def sparse_fixture():
    """72 samples, 6 bands x 12 epochs over 400 days, period 0.6137: ``(t, y, err, band)``; grid ``GLS(0.5, 3.0)``."""
    rng = np.random.default_rng(21)
    B, per = 6, 12
    t = np.sort(rng.uniform(0, 400, B * per))
    band = np.tile(np.arange(B), per)
    rng.shuffle(band)
    err = rng.uniform(0.08, 0.15, B * per)
    y = (15 + 0.4 * band + 0.25 * np.sin(2 * np.pi * t / 0.6137) + 0.1 * np.sin(4 * np.pi * t / 0.6137 + 1)
         + err * rng.standard_normal(B * per))
    return t, y, err, band


SPARSE_PERIOD = 0.6137


def _weights(y, err, band, n_bands, fit_mean, dtype):
    """Weights normalised over all samples, the values (centred per band with ``fit_mean``) and sum err**-2."""
    y = np.asarray(y, dtype=dtype)
    w = np.ones_like(y) if err is None else np.asarray(err, dtype=dtype) ** -2
    W = w.sum()
    w = w / W
    if fit_mean:
        y = y.copy()
        for b in range(n_bands):
            sel = band == b
            y[sel] -= np.dot(w[sel], y[sel]) / w[sel].sum()
    return w, y, W


def normal_equations(t, y, err, band, n_bands, freq, nterms, fit_mean, dtype=np.float64, chunk=CHUNK):
    """``M [F, D, D]``, ``b [F, D]``, ``YY`` and ``sum err**-2`` for the design ``1[band = 0], ..., 1[band = B - 1],
    cos th, sin th, ..., cos H th, sin H th`` (no indicators without ``fit_mean``), ``th = 2 pi f (t - min t)``.  The
    design of a smaller ``nterms`` is a leading block of the same columns.  ``chunk`` frequencies at a time (the block
    ``[chunk][D][N]`` is what the evaluation holds in memory)."""
    band = np.asarray(band)
    w, yc, W = _weights(y, err, band, n_bands, fit_mean, dtype)
    t = np.asarray(t, dtype=dtype)
    freq = np.asarray(freq, dtype=dtype)
    tp = t - t.min()
    two_pi = 2 * np.arccos(dtype(-1))
    D = 2 * nterms + (n_bands if fit_mean else 0)
    M = np.empty((freq.size, D, D), dtype=dtype)
    b = np.empty((freq.size, D), dtype=dtype)
    for lo in range(0, freq.size, chunk):
        theta = two_pi * freq[lo:lo + chunk, None] * tp[None, :]
        cols = [np.broadcast_to((band == k).astype(dtype), theta.shape) for k in range(n_bands)] if fit_mean else []
        for k in range(1, nterms + 1):
            cols += [np.cos(k * theta), np.sin(k * theta)]
        phi = np.stack(cols, axis=1)                       # [f, D, N]
        M[lo:lo + chunk] = np.matmul(phi * w, np.swapaxes(phi, 1, 2))
        b[lo:lo + chunk] = np.matmul(phi, w * yc)
    return M, b, np.dot(w, yc * yc), W


def columns(n_bands, nterms, fit_mean):
    """Columns of the model with ``nterms`` harmonics inside a larger one's normal equations."""
    return 2 * nterms + (n_bands if fit_mean else 0)


power_from = mo.power_from   # b^T M^-1 b by Cholesky in the arrays' dtype, NaN where a pivot is not positive
cond_from = mo.cond_from     # 2-norm condition number of the full float64 M


def power(t, y, err, band, n_bands, freq, nterms, fit_mean=True, psd=False, dtype=np.longdouble, chunk=CHUNK):
    return power_from(*normal_equations(t, y, err, band, n_bands, freq, nterms, fit_mean, dtype, chunk), psd=psd)


def cond(t, y, err, band, n_bands, freq, nterms, fit_mean=True, chunk=CHUNK):
    return cond_from(normal_equations(t, y, err, band, n_bands, freq, nterms, fit_mean, np.float64, chunk)[0])
