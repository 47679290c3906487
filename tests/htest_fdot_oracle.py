"""Test-local oracle of the Z^2_m / H-test plane over frequency and spin-down (plain numpy; imports only
``htest_oracle``).  PARITY UNPINNED BY THE REFERENCE: what is restated here is the published statistic with the phase
``f tau + fdot tau**2 / 2`` cycles, ``tau = t - epoch``.  Every ``cos(k theta)``, ``sin(k theta)`` is evaluated directly
per (event, frequency) pair from the whole phase - no recurrence, no split of the phase into a frequency part and an
offset - so the oracle shares no shortcut with the kernel it checks."""
import numpy as np

import htest_oracle as ho

EPOCHS = ("first", "middle", "before")        # t[0], the midpoint of the list, t[0] - 50
CYCLES = (0.0, 2.0, -4.5, 1.2e6)              # drift at the event farthest from the epoch; the last: the exact reduction


def z2_fdot(t, w, freq, fdot, epoch, M, dtype=np.float64, chunk=ho.CHUNK):
    """Cumulative ``Z2_m`` for ``m = 1 .. M`` of one row ``fdot``, ``[M][F]``, as ``htest_oracle.z2`` with
    ``theta = 2 pi (f tau + fdot tau**2 / 2)``, ``tau = t - epoch``; ``w`` None: unit weights.  ``chunk`` frequencies at a time."""
    t = np.asarray(t, dtype=dtype)
    w = np.ones_like(t) if w is None else np.asarray(w, dtype=dtype)
    freq = np.asarray(freq, dtype=dtype)
    tau = t - dtype(epoch)
    drift = dtype(fdot) * tau * tau / 2
    two_pi = 2 * np.arccos(dtype(-1))
    scale = 2 / np.sum(w * w)
    out = np.empty((M, freq.size), dtype=dtype)
    for lo in range(0, freq.size, chunk):
        theta = two_pi * (freq[lo:lo + chunk, None] * tau[None, :] + drift[None, :])
        cum = np.zeros(theta.shape[0], dtype=dtype)
        for k in range(1, M + 1):
            c = np.sum(w * np.cos(k * theta), axis=1)
            s = np.sum(w * np.sin(k * theta), axis=1)
            cum = cum + (c * c + s * s)
            out[k - 1, lo:lo + chunk] = scale * cum
    return out


def epoch_of(t, which):
    return {"first": t[0], "middle": 0.5 * (t[0] + t[-1]), "before": t[0] - 50.0}[which]


def rows_of(t, epoch, cycles=CYCLES):
    """The rows ``fdot = 2 c / max |tau|**2``: a drift of ``c`` cycles at the event farthest from the epoch."""
    far = np.max(np.abs(np.asarray(t, dtype=float) - epoch))
    return np.array([2.0 * c / far ** 2 for c in cycles])


def pulsar(n, seed, f0=0.137, fdot=-8e-6, span=1200.0, pulsed=0.5, width=0.05):
    """An event list of a spinning-down source and its photon weights: a share ``pulsed`` of the ``n`` events in a
    Gaussian pulse of ``width`` cycles at phase 0.3 of ``f0 tau + fdot tau**2 / 2``, ``tau`` from the middle of
    ``span`` (rejection sampling), the rest uniform.  Draws in the order: (candidate times, acceptance) until enough
    pulse events are kept, uniform events, weights."""
    rng = np.random.default_rng(seed)
    n_p = int(round(pulsed * n))
    kept = np.empty(0)
    while kept.size < n_p:
        tt = rng.uniform(0, span, 4 * n_p)
        tau = tt - span / 2
        ph = (f0 * tau + 0.5 * fdot * tau * tau) % 1
        d = np.abs(((ph - 0.3 + 0.5) % 1) - 0.5)
        kept = np.concatenate([kept, tt[rng.uniform(0, 1, tt.size) < np.exp(-0.5 * (d / width) ** 2)]])
    t_p = kept[:n_p]
    t_u = rng.uniform(0, span, n - n_p)
    t = np.sort(np.concatenate([t_p, t_u])) + 1234.5
    w = rng.uniform(0.2, 1, n)
    return t, w
