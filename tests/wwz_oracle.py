"""Test-local oracle of the weighted wavelet Z-transform (Foster 1996, AJ 112, 1709; plain numpy, imports nothing from
``periodicity_amd``).  The reference has no such statistic - PARITY UNPINNED BY THE REFERENCE: what is restated here are
the definitions of ``include/periodicity_hip.h``.

``exp``, ``cos`` and ``sin`` are evaluated directly per (sample, frequency, tau): no recurrence, no support cut, no
centring of ``y``, so the oracle shares no shortcut with the kernel it checks.  The 3 x 3 Cholesky is written out by
hand in the working precision (float64 or ``np.longdouble``)."""
import numpy as np

FOSTER = 1.0 / (8.0 * np.pi ** 2)
MIN_NEFF = 6.0        # cells compared in value: oracle Neff >= MIN_NEFF
LEFT_OUT_CAP = 0.05   # at most this share of a grid may be left out
RTOL, ATOL = 1e-6, 1e-9   # Tier E


def chirp_curve(offset=0.0):
    """The parity input: 300 uniform times on [0, 100) with (40, 55) removed (253 samples), a chirp from 0.2 to 0.4
    cycles per unit time with a growing amplitude, noise, a mean of 5; ``err`` uniform in [0.2, 0.5].  80 bins
    ``0.05 + 0.005 j``, 11 time shifts.  ``offset`` moves ``t`` and ``tau``."""
    rng = np.random.default_rng(20261020)
    t = np.sort(rng.uniform(0, 100, 300))
    t = t[(t <= 40) | (t >= 55)]
    y = np.sin(2 * np.pi * (0.2 + 0.001 * t) * t) * (1 + t / 200) + 0.3 * rng.standard_normal(t.size) + 5
    err = rng.uniform(0.2, 0.5, t.size)
    return t + offset, y, err, 0.05 + 0.005 * np.arange(80), np.linspace(0, 100, 11) + offset


def dense_curve(n=4000, span=1000.0):
    """The support-cut input: ``n`` uniform times on [0, span), a sinusoid at 0.8 plus noise, unit weights; 60 bins
    ``0.5 + 0.01 j``, 5 time shifts from 10 % to 90 % of the span."""
    rng = np.random.default_rng(7)
    t = np.sort(rng.uniform(0, span, n))
    y = np.sin(2 * np.pi * 0.8 * t) + 0.2 * rng.standard_normal(n)
    return t, y, None, 0.5 + 0.01 * np.arange(60), np.linspace(0.1 * span, 0.9 * span, 5)


def planes(t, y, err, freq, tau, decay=FOSTER, dtype=np.longdouble):
    """``(wwz, wwa, neff)``, each ``[ntau][nf]`` in ``dtype``."""
    t, y = np.asarray(t, dtype=dtype), np.asarray(y, dtype=dtype)
    s = np.ones_like(t) if err is None else np.asarray(err, dtype=dtype) ** -2
    freq, tau = np.asarray(freq, dtype=dtype), np.asarray(tau, dtype=dtype)
    two_pi = 2 * np.arccos(dtype(-1))
    omega = two_pi * freq[:, None]                                   # [nf, 1]
    theta = omega * (t - t[0])[None, :]
    c, sn = np.cos(theta), np.sin(theta)
    nan = dtype(np.nan)
    out = np.empty((3, tau.size, freq.size), dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        for r in range(tau.size):
            w = s * np.exp(-dtype(decay) * omega ** 2 * ((t - tau[r]) ** 2)[None, :])   # [nf, n]
            W = w.sum(axis=1)
            neff = W * W / (w * w).sum(axis=1)

            def ip(a, b):
                return (w * a * b).sum(axis=1) / W

            one = np.ones_like(c)
            S11, S12, S13, S22, S23, S33 = ip(one, one), ip(one, c), ip(one, sn), ip(c, c), ip(c, sn), ip(sn, sn)
            b1, b2, b3 = ip(one, y), ip(c, y), ip(sn, y)
            # Cholesky S = L L^T, forward and back substitution: a = S^-1 b
            bad = ~(S11 > 0) | ~np.isfinite(S11)
            l11 = np.sqrt(S11)
            l21, l31 = S12 / l11, S13 / l11
            d2 = S22 - l21 * l21
            bad |= ~(d2 > 0) | ~np.isfinite(d2)
            l22 = np.sqrt(d2)
            l32 = (S23 - l31 * l21) / l22
            d3 = S33 - l31 * l31 - l32 * l32
            bad |= ~(d3 > 0) | ~np.isfinite(d3)
            l33 = np.sqrt(d3)
            z1 = b1 / l11
            z2 = (b2 - l21 * z1) / l22
            z3 = (b3 - l31 * z1 - l32 * z2) / l33
            a3 = z3 / l33
            a2 = (z2 - l32 * a3) / l22
            a1 = (z1 - l21 * a2 - l31 * a3) / l11
            vx = ip(y, y) - b1 * b1
            vy = (a1 * b1 + a2 * b2 + a3 * b3) - b1 * b1
            wwz = (neff - 3) * vy / (2 * (vx - vy))
            wwa = np.sqrt(a2 * a2 + a3 * a3)
            dead = ~(W > 0)
            out[0, r] = np.where(bad | dead, nan, wwz)
            out[1, r] = np.where(bad | dead, nan, wwa)
            out[2, r] = np.where(dead, dtype(0), neff)
    return out[0], out[1], out[2]


def reductions(wwz, wwa, neff, min_neff=MIN_NEFF):
    """Ridge and best cell by the numpy expressions of the definition, on float64 planes:
    ``(ridge_bin, ridge_wwz, ridge_wwa, (best value, row, bin))``."""
    ntau = wwz.shape[0]
    eligible = np.where(neff >= min_neff, wwz, np.nan)
    has = ~np.all(np.isnan(eligible), axis=1)
    bins = np.full(ntau, -1, dtype=np.int64)
    bins[has] = np.nanargmax(eligible[has], axis=1)
    rows = np.arange(ntau)
    ridge_wwz = np.where(has, wwz[rows, np.maximum(bins, 0)], np.nan)
    ridge_wwa = np.where(has, wwa[rows, np.maximum(bins, 0)], np.nan)
    if not has.any():
        return bins, ridge_wwz, ridge_wwa, (np.nan, -1, -1)
    row = int(np.nanargmax(ridge_wwz))
    return bins, ridge_wwz, ridge_wwa, (float(ridge_wwz[row]), row, int(bins[row]))


def compare(got, exact, neff_exact):
    """``(worst error over its gate, share left out)`` of a plane against the oracle's: the cells with oracle
    ``Neff >= MIN_NEFF`` by Tier E, ``|d| <= RTOL |exact| + ATOL``; every other cell must be NaN or finite."""
    got = np.asarray(got, dtype=np.longdouble)
    keep = np.asarray(neff_exact >= MIN_NEFF)
    rest = got[~keep]
    assert np.all(np.isnan(rest) | np.isfinite(rest))
    singular = keep & np.isnan(exact)          # a pivot that is not positive in the oracle: NaN on both sides
    assert np.all(np.isnan(got[singular]))
    value = keep & ~singular
    assert np.all(np.isfinite(got[value]))
    ratio = np.abs(got[value] - exact[value]) / (RTOL * np.abs(exact[value]) + ATOL)
    return float(ratio.max()) if ratio.size else 0.0, 1.0 - keep.mean()
