"""Test-local oracle of box least squares (Kovacs, Zucker & Mazeh 2002) in plain numpy: the definition, literally.
Nothing here comes from periodicity_amd.  The reference has no such class - PARITY UNPINNED BY THE REFERENCE.

Weights ``w = err**-2 / sum(err**-2)`` (ones when absent), ``y' = y - sum(w y)``, ``YY = sum(w y'**2)``.  Per trial
period ``phi = (t / P) % 1`` in float64, bins ``[k / n_bins, (k + 1) / n_bins)`` by ``np.searchsorted`` on the doubles
``k / n_bins`` (``phi == 1.0`` joins the last bin), per bin ``r = sum w``, ``s = sum w y'``, ``c = count`` with
``np.add.at`` in the chosen dtype.  A box is a start bin ``i`` and a length ``L`` in ``len_min .. len_max``, wrapping past
phase 1; it is admissible when ``c >= min_points``, ``N_b - c >= min_points`` and ``0 < r < 1`` (``dips_only``:
``s < 0``).  ``SR = s**2 / (r (1 - r))``, ``power = max SR / YY``, ``depth = -s / (r (1 - r))``.  EVERY ``(L, i)`` is
evaluated."""
import numpy as np


def curve(n, seed, period=7.3, depth=1.0, q=0.05):
    """Sorted uniform times on [0, 3 n], err uniform in 0.5 - 1.5 x 0.1, level 10, a box of ``depth`` over the first
    ``q`` of the phase at ``period``, Gaussian noise."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 3.0 * n, n))
    err = rng.uniform(0.5, 1.5, n) * 0.1
    y = 10.0 - depth * ((t / period) % 1.0 < q) + err * rng.standard_normal(n)
    return t, y, err


def centred(t, y, err, dtype=np.longdouble):
    """``(w, y', YY)`` in ``dtype``, or None for input that has no periodogram (a non-finite value, ``err == 0``,
    ``YY == 0``): every output is NaN then."""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    err = np.ones_like(y) if err is None else np.asarray(err, dtype=np.float64)
    if not (np.all(np.isfinite(t)) and np.all(np.isfinite(y)) and np.all(np.isfinite(err)) and np.all(err != 0)) or y.size == 0:
        return None
    iv = err.astype(dtype) ** -2
    w = iv / np.sum(iv)
    yc = y.astype(dtype) - np.sum(w * y.astype(dtype))
    yy = np.sum(w * yc * yc)
    if not (np.isfinite(yy) and yy > 0):
        return None
    return w, yc, yy


def bin_index(t, period, n_bins):
    """numpy's bin of every sample at one trial period, or None when a phase is NaN."""
    with np.errstate(all="ignore"):
        phi = (np.asarray(t, dtype=np.float64) / np.float64(period)) % 1
    if np.any(np.isnan(phi)):
        return None
    k = np.searchsorted(np.arange(n_bins + 1) / n_bins, phi, side="right") - 1
    return np.where(k == n_bins, n_bins - 1, k)


class Scan(object):
    """What one call of :func:`scan` evaluated: ``sr[p, L - len_min, i]`` = ``SR / YY`` of box ``(i, L)`` at period
    ``p`` and ``depths[p, L - len_min, i]`` its depth (float64 copies of the ``dtype`` results), NaN where the box lacks
    ``min_points`` samples inside or outside or ``0 < r < 1`` fails - or everywhere, for a period with a NaN phase and
    for input without a periodogram."""

    def __init__(self, sr, depths, len_min):
        self.sr, self.depths, self.len_min = sr, depths, len_min

    def table(self, dips_only=False):
        """``SR / YY`` over ``(p, L, i)`` of the admissible boxes, NaN elsewhere (``s < 0`` is ``depth > 0``)."""
        return np.where(self.depths > 0, self.sr, np.nan) if dips_only else self.sr

    def power(self, dips_only=False):
        tab = self.table(dips_only).reshape(self.sr.shape[0], -1)
        out = np.full(tab.shape[0], np.nan)
        some = np.any(~np.isnan(tab), axis=1)
        out[some] = np.nanmax(tab[some], axis=1)
        return out

    def box(self, p, start_bin, box_bins, dips_only=False):
        """``(SR / YY, depth)`` of box ``(start_bin, box_bins)`` at period ``p``."""
        return self.table(dips_only)[p, box_bins - self.len_min, start_bin], self.depths[p, box_bins - self.len_min, start_bin]


def scan(t, y, err, periods, n_bins, len_min, len_max, min_points=5, dtype=np.longdouble):
    periods = np.atleast_1d(np.asarray(periods, dtype=np.float64))
    n_len = len_max - len_min + 1
    sr = np.full((periods.size, n_len, n_bins), np.nan)
    depths = np.full((periods.size, n_len, n_bins), np.nan)
    prep = centred(t, y, err, dtype)
    if prep is None:
        return Scan(sr, depths, len_min)
    w, yc, yy = prep
    lengths = np.arange(len_min, len_max + 1)[:, None]
    starts = np.arange(n_bins)[None, :]
    for p, period in enumerate(periods):
        k = bin_index(t, period, n_bins)
        if k is None:
            continue
        r, s, c = np.zeros(n_bins, dtype=dtype), np.zeros(n_bins, dtype=dtype), np.zeros(n_bins, dtype=np.int64)
        np.add.at(r, k, w)
        np.add.at(s, k, w * yc)
        np.add.at(c, k, 1)
        # window sums from the prefix of the histogram extended by the wrap-around bins
        pre = [np.concatenate([np.zeros(1, dtype=a.dtype), np.cumsum(np.concatenate([a, a[:len_max]]))]) for a in (r, s, c)]
        R, S, C = (a[starts + lengths] - a[starts] for a in pre)
        ok = (C >= min_points) & (c.sum() - C >= min_points) & (R > 0) & (R < 1)
        with np.errstate(all="ignore"):
            den = R * (1 - R)
            sr[p] = np.where(ok, S * S / den / yy, np.nan).astype(np.float64)
            depths[p] = np.where(ok, -S / den, np.nan).astype(np.float64)
    return Scan(sr, depths, len_min)


def naive(t, y, err, period, n_bins, len_min, len_max, min_points=5, dips_only=False):
    """The same search as a triple loop over (L, i, samples), float64: ``(power, {(i, L): SR / YY})``."""
    prep = centred(t, y, err, np.float64)
    k = bin_index(t, period, n_bins)
    table = {}
    if prep is None or k is None:
        return float("nan"), table
    w, yc, yy = prep
    for L in range(len_min, len_max + 1):
        for i in range(n_bins):
            r = s = 0.0
            c = 0
            for j in range(len(k)):
                if (k[j] - i) % n_bins < L:
                    r += w[j]
                    s += w[j] * yc[j]
                    c += 1
            if c >= min_points and len(k) - c >= min_points and 0 < r < 1 and (s < 0 or not dips_only):
                table[(i, L)] = s * s / (r * (1 - r)) / yy
    return (max(table.values()) if table else float("nan")), table
