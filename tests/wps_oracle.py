"""Test-local oracle of the Morlet wavelet power spectrum (``timefrequency.WPS``, csrc/wps.hip): PyWavelets' published
``cwt`` algorithm for "cmor2.0-1.0" restated literally - the integrated wavelet on 1024 points over [-8, 8], resampled
per scale, ``np.convolve``, ``np.diff``, the centred cut - in ``np.clongdouble``, with the float64 evaluation of the
same recipe, the change points of the resampling rule, the per-cell rounding budget of the kernel's tap sum, and the
numpy cone-of-influence mask and marginals.  PyWavelets itself is not a dependency: PARITY UNPINNED BY THE REFERENCE.

The table is built in float64 FIRST and then widened, so the oracle, the float64 recipe and the device all start from
the same bits; what is compared is the arithmetic behind the table."""
import functools
import warnings

import numpy as np

POINTS = 1024                 # 2 ** precision, precision = 10
LOWER, UPPER = -8.0, 8.0      # the wavelet's support
BANDWIDTH, CENTER = 2.0, 1.0  # cmor2.0-1.0
U = 2.0 ** -53
# roundings of a coefficient beyond the tap sum's own (one per tap): the weight's difference, sqrt(s), their product,
# and one spare for a square root that is not correctly rounded
C0 = 4
SCALES = (1 / 16, 0.4, 1.0, 3.7, 63.9375, 64.0, 100.3, 700.0)
TAP_SCALES = (1 / 16, 0.4, 1.0, 3.7, 63.9375, 64.0, 2 * 63.9375, 700.0)


@functools.lru_cache(maxsize=None)
def table():
    """``(xg, step, int_psi)``: the float64 table every side shares."""
    xg = np.linspace(LOWER, UPPER, POINTS)
    step = xg[1] - xg[0]
    psi = (np.pi * BANDWIDTH) ** -0.5 * np.exp(2j * np.pi * CENTER * xg) * np.exp(-xg ** 2 / BANDWIDTH)
    int_psi = np.conj(np.cumsum(psi) * step)
    return xg, step, int_psi


def filter_indices(s):
    """``j``: the table entries of the filter at scale ``s``, by the numpy rule."""
    xg, step, _ = table()
    j = (np.arange(s * (xg[-1] - xg[0]) + 1) / (s * step)).astype(int)
    return j[j < POINTS]


def change_points(s):
    """``(m, before, after, L)``: the positions 0 .. L of the filter where the table entry changes, with the entries on
    either side (-1: outside the filter).  Position 0 and position L are the filter's two edges."""
    j = filter_indices(s)
    L = j.size
    padded = np.concatenate([[-1], j, [-1]])
    m = np.flatnonzero(padded[1:] != padded[:-1])
    return m, padded[m], padded[m + 1], L


def _filter(s, ctype):
    _, _, int_psi = table()
    j = filter_indices(s)
    if j.size < 2:
        raise ValueError("Selected scale is too small.")
    return int_psi.astype(ctype)[j][::-1]


def literal(x, s, ctype=np.clongdouble):
    """``coef[N]`` at one scale: convolve, diff, cut - in ``ctype`` throughout."""
    rtype = np.real(np.zeros(1, dtype=ctype)).dtype
    x = np.asarray(x, dtype=rtype)
    s = rtype.type(s)
    h = _filter(float(s), ctype)
    conv = np.convolve(x.astype(ctype), h)
    coef = -np.sqrt(s) * np.diff(conv)
    d = (coef.size - x.size) / 2
    if d > 0:
        coef = coef[int(np.floor(d)):-int(np.ceil(d))]
    assert coef.size == x.size
    return coef


def spectrum(x, scales, ctype=np.clongdouble):
    """``(coefs, spectrum)`` ``[n_scales][N]``: the literal recipe per scale, ``|coef|^2 / s``."""
    coefs = np.stack([literal(x, s, ctype) for s in scales])
    rtype = coefs.real.dtype
    return coefs, (coefs.real ** 2 + coefs.imag ** 2) / np.asarray(scales, dtype=rtype)[:, None]


def tap_sum(x, s):
    """``coef[N]`` by the identity the kernel is built on, in float64: per change point one weight
    ``-sqrt(s) (h[k] - h[k-1])`` times a shifted copy of ``x``."""
    _, _, int_psi = table()
    x = np.asarray(x, dtype=float)
    m, before, after, L = change_points(s)
    table0 = np.concatenate([int_psi, [0.0]])   # entry -1: outside the filter
    weights = -np.sqrt(s) * (table0[before] - table0[after])
    n = np.arange(x.size)
    coef = np.zeros(x.size, dtype=complex)
    for mk, wk in zip(m, weights):
        at = n + mk - (L + 1) // 2
        ok = (at >= 0) & (at < x.size)
        coef[ok] += wk * x[at[ok]]
    return coef


def budget(x, s):
    """``(bound_c, taps)``: per cell the rounding budget of the kernel's coefficient,
    ``(taps + C0) 2^-53 sqrt(s) sum_k |h[k] - h[k-1]| |x[...]|``, in long double.  |h[k] - h[k-1]| of a complex
    difference is taken as |re| + |im|, an upper bound that covers both parts."""
    x = np.abs(np.asarray(x, dtype=np.longdouble))
    h = _filter(s, np.clongdouble)
    dh = np.diff(np.concatenate([[0], h, [0]]))
    taps = int(np.count_nonzero(dh))
    mag = np.abs(dh.real) + np.abs(dh.imag)
    L = h.size
    conv = np.convolve(x, mag)
    first = 1 + (L - 2) // 2
    return (taps + C0) * np.longdouble(U) * np.sqrt(np.longdouble(s)) * conv[first:first + x.size], taps


def gates(x, scales, coefs):
    """``(bound_c, bound_spectrum)`` ``[n_scales][N]`` for ``coefs`` of the oracle:
    ``(2 |c| bound_c + bound_c^2) / s`` plus four ulp of the spectrum for the epilogue's own roundings."""
    bc = np.stack([budget(x, s)[0] for s in scales])
    sc = np.asarray(scales, dtype=np.longdouble)[:, None]
    mag = np.abs(coefs)
    return bc, (2 * mag * bc + bc ** 2) / sc + 4 * np.longdouble(U) * mag ** 2 / sc


def mask_coi(time, periods):
    """The reference's cone-of-influence mask ``[n_periods][N]``."""
    corr = np.exp2(0.5)
    t_max, t_min = np.max(time), np.min(time)
    t_mesh, p_mesh = np.meshgrid(time, periods)
    return corr * p_mesh < np.minimum(t_mesh - t_min, t_max - t_mesh)


def marginals(plane, mask):
    """``gwps, sav, masked_gwps, masked_sav, gwps_count, sav_count`` of a returned plane, as numpy gives them."""
    masked = np.where(mask, plane, np.nan)
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return (plane.mean(axis=1), plane.mean(axis=0), np.nanmean(masked, axis=1), np.nanmean(masked, axis=0),
                mask.sum(axis=1), mask.sum(axis=0))


def curve(n, seed=20261021):
    """An evenly sampled test curve: two sinusoids, a drift and noise, dt = 0.02."""
    rng = np.random.default_rng(seed + n)
    t = 0.02 * np.arange(n) + 3.0
    y = np.sin(2 * np.pi * t / 0.31) + 0.5 * np.sin(2 * np.pi * t / 2.9 + 1) + 0.1 * t + 0.3 * rng.standard_normal(n) + 7
    return t, y
