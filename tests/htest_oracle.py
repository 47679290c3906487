"""Test-local oracle of the Z^2_m and H-test periodograms of an event list (plain numpy; imports nothing from
``periodicity_amd``).  The reference has no such class - PARITY UNPINNED BY THE REFERENCE: what is restated here is the
published statistic (Buccheri et al. 1983; de Jager, Raubenheimer & Swanepoel 1989; weights as Kerr 2011).

Every ``cos(k theta)``, ``sin(k theta)`` is evaluated directly per (event, frequency) pair - no recurrence - so the
oracle shares no shortcut with the kernel it checks."""
import numpy as np

CHUNK = 256   # frequencies per block of the dense evaluation, unless the caller names another
LONG_FREQUENCY = 10.0123   # Hz: the pulsation of ``long_events``
SEEDS = {5: 1, 63: 2, 64: 3, 65: 4, 129: 5, 200: 6}   # events(n, SEEDS[n]): the lists the host and the GPU tests share


def events(n, seed, period=7.3, pulsed=0.35, width=0.06):
    """The test event list of size ``n`` and its photon weights: a share ``pulsed`` of the events in a Gaussian pulse
    of ``width`` cycles at phase 0.3 of ``period``, the rest uniform over a span of 3 n.  Draws in the order pulse
    cycles, pulse phases, uniform events, weights."""
    rng = np.random.default_rng(seed)
    span = 3.0 * n
    n_p = int(round(pulsed * n))
    cycles = rng.integers(0, int(span / period), n_p)
    t_p = (cycles + (0.3 + width * rng.standard_normal(n_p)) % 1) * period
    t_u = rng.uniform(0, span, n - n_p)
    t = np.sort(np.concatenate([t_p, t_u])) + 1234.5
    w = rng.uniform(0.2, 1, n)
    return t, w


def long_events(n=300, seed=32, span=1.0e5, offset=5.0e8, frequency=LONG_FREQUENCY, pulsed=0.35, width=0.06):
    """A long-baseline event list and its photon weights: ``n`` events over ``span`` seconds at a mission-clock
    ``offset``, a share ``pulsed`` of them in a Gaussian pulse of ``width`` cycles at phase 0.3 of ``frequency`` - about
    1e6 cycles over the baseline.  Draws in the order of ``events``."""
    rng = np.random.default_rng(seed)
    n_p = int(round(pulsed * n))
    cycles = rng.integers(0, int(span * frequency), n_p)
    t_p = (cycles + (0.3 + width * rng.standard_normal(n_p)) % 1) / frequency
    t_u = rng.uniform(0, span, n - n_p)
    t = np.sort(np.concatenate([t_p, t_u])) + offset
    w = rng.uniform(0.2, 1, n)
    return t, w


def z2(t, w, freq, M, dtype=np.float64, chunk=CHUNK):
    """Cumulative ``Z2_m`` for ``m = 1 .. M``, ``[M][F]``: ``(2 / sum w**2) sum_{k <= m} (C_k**2 + S_k**2)`` with
    ``theta = 2 pi f (t - min t)``; ``w`` None: unit weights.  ``chunk`` frequencies at a time."""
    t = np.asarray(t, dtype=dtype)
    w = np.ones_like(t) if w is None else np.asarray(w, dtype=dtype)
    freq = np.asarray(freq, dtype=dtype)
    tp = t - t.min()
    two_pi = 2 * np.arccos(dtype(-1))
    scale = 2 / np.sum(w * w)
    out = np.empty((M, freq.size), dtype=dtype)
    for lo in range(0, freq.size, chunk):
        theta = two_pi * freq[lo:lo + chunk, None] * tp[None, :]
        cum = np.zeros(theta.shape[0], dtype=dtype)
        for k in range(1, M + 1):
            c = np.sum(w * np.cos(k * theta), axis=1)
            s = np.sum(w * np.sin(k * theta), axis=1)
            cum = cum + (c * c + s * s)
            out[k - 1, lo:lo + chunk] = scale * cum
    return out


def candidates(Z):
    """``Z2_m - 4 m + 4`` for every row ``m - 1`` of a cumulative ``Z``."""
    m = np.arange(1, Z.shape[0] + 1, dtype=Z.dtype)
    return Z - 4 * m[:, None] + 4


def h_and_m(Z):
    """``H = max_m (Z2_m - 4 m + 4)`` and the lowest ``m`` that reaches it (``np.argmax`` keeps the first)."""
    cand = candidates(Z)
    best = np.argmax(cand, axis=0)
    return cand[best, np.arange(Z.shape[1])], best + 1


def gate(Z):
    """The value gate per bin, ``1e-6 Z2 + 1e-9`` with the bin's largest ``Z2_m`` (H itself cancels to about 0)."""
    return 1e-6 * np.max(Z, axis=0) + 1e-9


def decided(Z):
    """Bins whose best ``m`` the values decide: the best and the second-best candidate differ by more than twice the
    gate (always, with one harmonic)."""
    if Z.shape[0] == 1:
        return np.ones(Z.shape[1], dtype=bool)
    cand = np.sort(candidates(Z), axis=0)
    return cand[-1] - cand[-2] > 2 * gate(Z)
