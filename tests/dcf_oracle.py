"""Test-local numpy oracle of the discrete correlation function (Edelson & Krolik 1988, ApJ 333, 646) as
include/periodicity_hip.h defines it, the gate its sums are held to, and the inputs tests/test_dcf_host.py and
tests/test_dcf_gpu.py share.  The reference has no such function - PARITY UNPINNED BY THE REFERENCE - so the oracle
restates the definition: every pair's lag is one float64 subtraction, its bin comes from ``np.searchsorted`` on the
float64 edges, the counts from ``np.bincount``, and the six sums and their sums of absolute terms are accumulated term
by term in ``np.longdouble``.

The gate is derived, not measured: any summation tree over M terms is within (M - 1) u sum |term| of the exact sum to
first order, u = 2^-53, adding an empty partial is exact, and the roundings of b^2, a^2, a sum b, a^2 sum b^2 and a n
are covered by the 8 of

    |got - exact| <= (pairs[k] + 8) 2^-53 T_x[k],     T_x[k] = sum |term| over the bin's pairs.

An empty bin has T = 0: its sums must be exactly 0.0."""
import collections

import numpy as np

SUMS = ("Sa", "Sb", "Saa", "Sbb", "Sab", "Sabab")
U = 2.0 ** -53

Oracle = collections.namedtuple("Oracle", ["pairs", "sums", "abs_sums", "i", "j", "k"])


def scan(ta, a, tb, b, edges, skip_same_index=False, dtype=np.longdouble):
    """The counts [nlag], the sums and the sums of absolute terms [6][nlag] in ``dtype``, and the pairs (i, j, bin)."""
    ta, a, tb, b, edges = (np.asarray(x, dtype=np.float64) for x in (ta, a, tb, b, edges))
    nlag = edges.size - 1
    d = tb[None, :] - ta[:, None]
    k = np.searchsorted(edges, d, side="right") - 1
    keep = (k >= 0) & (k < nlag) & (d < edges[-1])
    if skip_same_index:
        assert ta.size == tb.size
        keep &= ~np.eye(ta.size, dtype=bool)
    i, j = np.nonzero(keep)
    k = k[keep]
    pairs = np.bincount(k, minlength=nlag).astype(np.int64)
    ai, bj = a[i].astype(dtype), b[j].astype(dtype)
    terms = (ai, bj, ai * ai, bj * bj, ai * bj, (ai * bj) ** 2)
    sums, abs_sums = np.zeros((6, nlag), dtype=dtype), np.zeros((6, nlag), dtype=dtype)
    for q, term in enumerate(terms):
        np.add.at(sums[q], k, term)
        np.add.at(abs_sums[q], k, np.abs(term))
    return Oracle(pairs, sums, abs_sums, i, j, k)


def gate(oracle):
    """The bound [6][nlag] on |got - exact|."""
    return (oracle.pairs.astype(np.longdouble) + 8) * np.longdouble(U) * oracle.abs_sums


def worst_ratio(pairs, sums, oracle):
    """Counts equal, every sum of every bin inside the gate (an empty bin: exactly 0.0); the worst error / gate."""
    assert np.array_equal(pairs, oracle.pairs), np.flatnonzero(pairs != oracle.pairs)
    err = np.abs(np.asarray(sums).astype(np.longdouble) - oracle.sums)
    bound = gate(oracle)
    assert np.all(err <= bound), {SUMS[q]: np.flatnonzero(~(err[q] <= bound[q])) for q in range(6) if np.any(~(err[q] <= bound[q]))}
    empty = oracle.pairs == 0
    assert np.all(np.asarray(sums)[:, empty] == 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


def fft_acf(x, max_lag):
    """The reference's mask-corrected ACF (core.py:603-607) restated: the inverse FFT of the power spectrum of the
    centred, zero-padded series over the same transform of ones, normalised at lag 0."""
    x = np.asarray(x, dtype=float)
    n = x.size
    ryy = np.fft.ifft(np.abs(np.fft.fft(x - x.mean(), 2 * n)) ** 2).real
    ryy /= np.fft.ifft(np.abs(np.fft.fft(np.ones(n), 2 * n)) ** 2).real
    return ryy[:max_lag] / ryy[0]


def random_walk(n, seed=3):
    """A centred random walk on ``arange(n)``."""
    x = np.cumsum(np.random.default_rng(seed).standard_normal(n))
    return np.arange(float(n)), x - x.mean()


def uneven_auto():
    """Uneven times at a Julian-date offset: 692 to 949 pairs a bin, 52 389 in all."""
    rng = np.random.default_rng(1)
    t = np.sort(rng.uniform(0, 100, 500)) + 2450000.0
    x = rng.standard_normal(500)
    return t, x - x.mean(), 0.37 * np.arange(65)


def rounding_case():
    """Lags that scatter by ulps around every edge: t = 2450000 + 0.1 arange(300) against edges 0.1 arange(41)."""
    t = 2450000 + 0.1 * np.arange(300)
    x = np.random.default_rng(2).standard_normal(300)
    return t, x - x.mean(), 0.1 * np.arange(41)


def cross_case(nlag):
    """257 against 130 samples on different baselines, lags from negative to positive."""
    rng = np.random.default_rng(4)
    ta = np.sort(rng.uniform(0, 80, 257))
    tb = np.sort(rng.uniform(20, 70, 130))
    a, b = rng.standard_normal(257) + 0.3, rng.standard_normal(130) - 1.0
    return ta, a, tb, b, np.linspace(-30.0, 35.0, nlag + 1)


def wandering_sinusoid():
    """A sinusoid of period 17.3 whose phase is a random walk, 400 uneven samples over 300, noise 0.2."""
    rng = np.random.default_rng(20261021)
    t = np.sort(rng.uniform(0, 300, 400))
    grid = np.linspace(0, 300, 3001)
    phase = np.interp(t, grid, np.cumsum(0.12 * rng.standard_normal(3001)))
    return t, np.sin(2 * np.pi * t / 17.3 + phase) + 0.2 * rng.standard_normal(400)


def period_rule(lags, dcf):
    """``DCF.period`` restated on scipy: the most prominent peak over the finite bins of positive lag."""
    from scipy.signal import find_peaks
    keep = np.isfinite(dcf) & (lags > 0)
    at, res = find_peaks(dcf[keep], prominence=0.0)
    if at.size == 0:
        return None, res
    return float(lags[keep][at[np.argmax(res["prominences"])]]), res
