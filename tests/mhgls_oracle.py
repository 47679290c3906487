"""Test-local oracle of the multi-harmonic generalised Lomb-Scargle periodogram (plain numpy; imports nothing from
``periodicity_amd``).  The reference has no such class - PARITY UNPINNED BY THE REFERENCE: what is restated here is the
published statistic (Schwarzenberg-Czerny 1996; Palmer 2009) on the weights, centring and normalisations of ``GLS``.

Every ``cos(k theta)``, ``sin(k theta)`` is evaluated directly per (sample, frequency) pair - no recurrence, no
product-to-sum rule - so the oracle shares no shortcut with the kernel it checks."""
import numpy as np

CHUNK = 256   # frequencies per block of the dense evaluation, unless the caller names another
LONG_PERIOD = 0.0031   # days: the signal of ``long_curve``


def curve(n, seed):
    """The test curve of size ``n``: draws in the order t, err, noise."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 3.0 * n, n))
    err = rng.uniform(0.1, 0.3, n)
    y = 1 + 0.7 * np.sin(2 * np.pi * t / 6.3) + 0.3 * np.sin(4 * np.pi * t / 6.3 + 1) + err * rng.standard_normal(n)
    return t, y, err


def _weights(y, err, fit_mean, dtype):
    """Normalised weights, the (centred) values and sum err**-2."""
    y = np.asarray(y, dtype=dtype)
    w = np.ones_like(y) if err is None else np.asarray(err, dtype=dtype) ** -2
    W = w.sum()
    w = w / W
    if fit_mean:
        y = y - np.dot(w, y)
    return w, y, W


def long_curve(n=300, seed=31, span=3000.0, offset=2454900.5, period=LONG_PERIOD):
    """A long-baseline curve: ``n`` samples over ``span`` days at a Julian-date ``offset``, a two-harmonic signal of
    ``period`` days - about 1e6 cycles over the baseline.  Draws in the order t, err, noise."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, span, n)) + offset
    err = rng.uniform(0.1, 0.3, n)
    y = (1 + 0.7 * np.sin(2 * np.pi * (t - t[0]) / period) + 0.3 * np.sin(4 * np.pi * (t - t[0]) / period + 1)
         + err * rng.standard_normal(n))
    return t, y, err


def normal_equations(t, y, err, freq, nterms, fit_mean, dtype=np.float64, chunk=CHUNK):
    """``M [F, D, D]``, ``b [F, D]``, ``YY`` and ``sum err**-2`` for the design ``1, cos th, sin th, ..., cos H th,
    sin H th`` (no constant without ``fit_mean``), ``th = 2 pi f (t - t[0])``; ``chunk`` frequencies at a time (the
    block ``[chunk][D][N]`` is what the evaluation holds in memory)."""
    w, yc, W = _weights(y, err, fit_mean, dtype)
    t = np.asarray(t, dtype=dtype)
    freq = np.asarray(freq, dtype=dtype)
    tp = t - t[0]
    two_pi = 2 * np.arccos(dtype(-1))
    D = 2 * nterms + (1 if fit_mean else 0)
    M = np.empty((freq.size, D, D), dtype=dtype)
    b = np.empty((freq.size, D), dtype=dtype)
    for lo in range(0, freq.size, chunk):
        theta = two_pi * freq[lo:lo + chunk, None] * tp[None, :]
        cols = [np.ones_like(theta)] if fit_mean else []
        for k in range(1, nterms + 1):
            cols += [np.cos(k * theta), np.sin(k * theta)]
        phi = np.stack(cols, axis=1)                       # [f, D, N]
        M[lo:lo + chunk] = np.matmul(phi * w, np.swapaxes(phi, 1, 2))
        b[lo:lo + chunk] = np.matmul(phi, w * yc)
    return M, b, np.dot(w, yc * yc), W


def _quadratic(M, b):
    """``b^T M^-1 b`` per bin by Cholesky in the arrays' own dtype; NaN where a pivot is not positive."""
    F, D, _ = M.shape
    L = np.zeros_like(M)
    z = np.zeros_like(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(D):
            d = M[:, j, j] - np.sum(L[:, j, :j] ** 2, axis=1)
            d = np.where(d > 0, d, np.nan)
            L[:, j, j] = np.sqrt(d)
            z[:, j] = (b[:, j] - np.sum(L[:, j, :j] * z[:, :j], axis=1)) / L[:, j, j]
            for i in range(j + 1, D):
                L[:, i, j] = (M[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
    return np.sum(z * z, axis=1)


def power_from(M, b, YY, W, psd=False):
    """The power from the normal equations: ``b^T M^-1 b / YY`` (``psd``: ``b^T M^-1 b * 0.5 * sum err**-2``)."""
    quad = _quadratic(M, b)
    return quad * M.dtype.type(0.5) * W if psd else quad / YY


def cond_from(M):
    """2-norm condition number of ``M`` per bin (inf where it cannot be computed)."""
    M = np.asarray(M, dtype=np.float64)
    out = np.full(M.shape[0], np.inf)
    ok = np.all(np.isfinite(M), axis=(1, 2))
    out[ok] = np.linalg.cond(M[ok], 2)
    return out


def power(t, y, err, freq, nterms, fit_mean=True, psd=False, dtype=np.longdouble, chunk=CHUNK):
    """Multi-harmonic GLS power on ``freq``, solved by Cholesky in ``dtype``."""
    return power_from(*normal_equations(t, y, err, freq, nterms, fit_mean, dtype, chunk), psd=psd)


def cond(t, y, err, freq, nterms, fit_mean=True, chunk=CHUNK):
    return cond_from(normal_equations(t, y, err, freq, nterms, fit_mean, np.float64, chunk)[0])


COND_LIMIT = 1e6   # bins compared in value: cond <= COND_LIMIT (M is nearly singular at the lowest few frequencies)
