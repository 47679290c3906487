"""Test-local oracle of the empirical mode decompositions (periodicity_amd/decomposition.py, csrc/emd.hip).

Two evaluations of one definition (include/periodicity_hip.h has it in full):

* ``literal`` makes exactly the reference's calls - ``scipy.signal.find_peaks``, ``np.pad`` / ``np.delete`` for the
  reflected extrema, ``splrep`` / ``splev`` for the envelopes - on numpy arrays;
* ``exact`` follows the same steps with the not-a-knot spline solved and evaluated in ``np.longdouble``; mu is rounded to
  float64 once and subtracted in float64, so its trajectory is the correctly rounded one.

The reference's own classes need xarray, which is not installed: parity with them is UNPINNED, what is pinned is parity with
these calls.  ``Margins`` records how far every discrete decision of a run was from a tie.
"""
import numpy as np
from scipy.interpolate import splev, splrep
from scipy.signal import find_peaks

LD = np.longdouble


class Margins:
    """Smallest distances from a tie seen in a run: ``sigma`` = |sigma - theta| / theta over both thresholds, ``extremum``
    = the smallest non-zero neighbour difference at an extremum over max|mode|, ``sign`` = the smallest non-zero |mode| at
    a sign change over max|mode|."""

    def __init__(self):
        self.sigma = self.extremum = self.sign = np.inf

    def see_mode(self, v, M, D):
        top = np.max(np.abs(v))
        if top == 0:
            return
        ext = np.concatenate([M, D]).astype(int)
        if ext.size:
            d = np.abs(np.concatenate([v[ext] - v[ext - 1], v[ext + 1] - v[ext]]))
            d = d[d > 0]
            if d.size:
                self.extremum = min(self.extremum, float(d.min() / top))
        (z,) = np.where(np.diff(np.signbit(v)))
        if z.size:
            a = np.abs(np.concatenate([v[z], v[z + 1]]))
            a = a[a > 0]
            if a.size:
                self.sign = min(self.sign, float(a.min() / top))

    def see_sigma(self, sigma, theta_1, theta_2):
        s = np.asarray(sigma, dtype=np.float64)
        s = s[np.isfinite(s)]
        if s.size:
            self.sigma = min(self.sigma, float(np.min(np.abs(s - theta_1)) / theta_1),
                             float(np.min(np.abs(s - theta_2)) / theta_2))

    def smallest(self):
        return min(self.sigma, self.extremum, self.sign)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def noise(n, seed):
    return np.arange(n, dtype=np.float64), np.random.default_rng(seed).standard_normal(n)


def tones(n):
    t = np.arange(n, dtype=np.float64)
    x = np.sin(2 * np.pi * 0.065 * t)
    lo, hi = n // 2, 3 * n // 4
    x[lo:hi] += np.sin(2 * np.pi * 0.255 * (t[lo:hi] - n // 2))
    return t, x


def mix():
    rng = np.random.default_rng(4)
    t = np.sort(rng.uniform(0, 30, 300))
    x = np.sin(2 * np.pi * t / 1.7) + 0.5 * np.sin(2 * np.pi * t / 7.3) + 0.02 * t + 0.05 * rng.standard_normal(300)
    return t, x


# ---- one sift ----------------------------------------------------------------------------------------------------------
def extrema(v):
    return find_peaks(v, prominence=0.0)[0], find_peaks(-v, prominence=0.0)[0]


def n_zero(v):
    return int(np.count_nonzero(np.diff(np.signbit(v))))


def knots_reference(t, v, idx, p):
    """The reference's way: the list with both edges, np.pad(reflect; odd for the times), the two edge points dropped."""
    full = np.hstack([0, idx, -1])
    kt = np.pad(t[full], p, mode="reflect", reflect_type="odd")
    kv = np.pad(v[full], p, mode="reflect")
    drop = [p, -p - 1]
    return np.delete(kt, drop), np.delete(kv, drop)


def knots_rule(t, v, idx, p):
    """The rule as the header states it."""
    m, last = len(idx), len(t) - 1
    kt = [2 * t[0] - t[idx[p - 1 - j]] for j in range(p)] + [t[i] for i in idx] + \
         [2 * t[last] - t[idx[m - 1 - j]] for j in range(p)]
    kv = [v[idx[p - 1 - j]] for j in range(p)] + [v[i] for i in idx] + [v[idx[m - 1 - j]] for j in range(p)]
    return np.array(kt, dtype=np.float64), np.array(kv, dtype=np.float64)


def is_monotonic(M, D, p):
    return len(M) < p or len(D) < p or len(M) + 2 * p < 4 or len(D) + 2 * p < 4


def spline_literal(kt, kv, t):
    return splev(t, splrep(kt, kv))


def spline_exact(kt, kv, t):
    """The not-a-knot cubic spline through (kt, kv) at t, solved (slope form, Thomas) and evaluated in long double."""
    x = [LD(a) for a in kt]
    y = [LD(a) for a in kv]
    K = len(x)
    h = [x[j + 1] - x[j] for j in range(K - 1)]
    d = [(y[j + 1] - y[j]) / h[j] for j in range(K - 1)]
    sub, diag, sup, rhs = [LD(0)] * K, [LD(0)] * K, [LD(0)] * K, [LD(0)] * K
    span = x[2] - x[0]
    diag[0], sup[0] = h[1], span
    rhs[0] = ((h[0] + 2 * span) * h[1] * d[0] + h[0] * h[0] * d[1]) / span
    for j in range(1, K - 1):
        sub[j], diag[j], sup[j] = h[j], 2 * (h[j - 1] + h[j]), h[j - 1]
        rhs[j] = 3 * (h[j] * d[j - 1] + h[j - 1] * d[j])
    span = x[K - 1] - x[K - 3]
    sub[K - 1], diag[K - 1] = span, h[K - 3]
    rhs[K - 1] = (h[K - 2] * h[K - 2] * d[K - 3] + (2 * span + h[K - 2]) * h[K - 3] * d[K - 2]) / span
    cp, rp = [LD(0)] * K, [LD(0)] * K
    cp[0], rp[0] = sup[0] / diag[0], rhs[0] / diag[0]
    for j in range(1, K):
        m = diag[j] - sub[j] * cp[j - 1]
        cp[j] = sup[j] / m
        rp[j] = (rhs[j] - sub[j] * rp[j - 1]) / m
    s = [LD(0)] * K
    s[K - 1] = rp[K - 1]
    for j in range(K - 2, -1, -1):
        s[j] = rp[j] - cp[j] * s[j + 1]
    xs, ys, ss = np.array(x, dtype=LD), np.array(y, dtype=LD), np.array(s, dtype=LD)
    j = np.clip(np.searchsorted(np.asarray(kt, dtype=np.float64), t, side="right") - 1, 0, K - 2)
    hh = xs[j + 1] - xs[j]
    slope = (ys[j + 1] - ys[j]) / hh
    tt = (ss[j] + ss[j + 1] - 2 * slope) / hh
    c2, c3 = (slope - ss[j]) / hh - tt, tt / hh
    dx = np.asarray(t, dtype=LD) - xs[j]
    return ((c3 * dx + c2) * dx + ss[j]) * dx + ys[j]


def sift(t, v, p, how="literal"):
    """One sift evaluation: dict with M, D, n_zero, monotonic and - unless monotonic - upper, lower (float64 for
    ``literal``, long double for ``exact``)."""
    M, D = extrema(v)
    out = {"M": M, "D": D, "n_zero": n_zero(v), "monotonic": is_monotonic(M, D, p)}
    if not out["monotonic"]:
        spline = spline_literal if how == "literal" else spline_exact
        out["upper"] = spline(*knots_reference(t, v, M, p), t)
        out["lower"] = spline(*knots_reference(t, v, D, p), t)
    return out


# ---- the decomposition ---------------------------------------------------------------------------------------------------
def emd(t, x, max_iter=2000, pad_width=2, theta_1=0.05, theta_2=0.50, alpha=0.05, max_modes=None, how="literal",
        margins=None):
    """``(modes, residue, sifts, flags)``: the reference's EMD.__call__ / iter / sift on arrays; flags as the device's."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if max_modes is None:
        max_modes = np.inf
    modes, sifts, flags = [], [], 0
    monotonic = x.size < 4
    residue = x.copy()
    while not monotonic and len(modes) < max_modes:
        mode, count, is_imf = residue.copy(), 0, False
        for _ in range(max_iter):
            s = sift(t, mode, pad_width, how)
            if s["monotonic"]:
                monotonic = True
                break
            if margins is not None:
                margins.see_mode(mode, s["M"], s["D"])
            with np.errstate(divide="ignore", invalid="ignore"):
                mu = (s["upper"] + s["lower"]) / 2
                amp = (s["upper"] - s["lower"]) / 2
                sigma = np.abs(mu / amp)
            if margins is not None:
                margins.see_sigma(sigma, theta_1, theta_2)
            with np.errstate(invalid="ignore"):
                is_imf = np.mean(sigma > theta_1) < alpha
                is_imf = is_imf and np.all(sigma < theta_2)
            is_imf = bool(is_imf and (np.abs(s["n_zero"] - (len(s["M"]) + len(s["D"]))) <= 1))
            if is_imf:
                break
            mode = mode - np.asarray(mu, dtype=np.float64)
            count += 1
        if not monotonic:
            if not is_imf:
                flags |= 1
            modes.append(mode)
            sifts.append(count)
            residue = residue - mode
    if not monotonic and x.size >= 4:
        M, D = extrema(residue)
        if not is_monotonic(M, D, pad_width):
            flags |= 2
    return modes, residue, sifts, flags


def ceemdan(t, x, ensemble_size=50, random_seed=None, epsilon=0.2, min_energy=0.0, max_modes=None, how="literal",
            margins=None, **emd_kwargs):
    """The reference's CEEMDAN.__call__ on arrays: ``(imfs, noise_trajectories, stage_trajectories)`` with a trajectory
    = the list of (n_modes, sifts of the first mode) per realisation."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if max_modes is None:
        max_modes = np.inf
    rng = np.random.default_rng(random_seed)
    run = lambda y, **kw: emd(t, y, how=how, margins=margins, **emd_kwargs, **kw)
    sigma_x = np.std(x)
    noise_modes, noise_traj = [], []
    for _ in range(ensemble_size):
        m, _, s, _ = run(rng.standard_normal(x.size))
        noise_modes.append(m)
        noise_traj.append((len(m), list(s)))
    imfs, stages = [], []
    residue = x / sigma_x
    while len(imfs) < max_modes:
        k = len(imfs)
        mu, traj = 0, []
        for i in range(ensemble_size):
            noisy = residue.copy()
            if len(noise_modes[i]) > k:
                beta = epsilon * np.std(residue)
                if k == 0:
                    beta /= np.std(noise_modes[i][k])
                noisy = noisy + beta * noise_modes[i][k]
            m, _, s, _ = run(noisy, max_modes=1)
            mode = m[0] if m else noisy.copy()
            traj.append((len(m), s[0] if s else 0))
            mu = mu + (noisy - mode) / ensemble_size
        stages.append(traj)
        imfs.append(residue - mu)
        residue = mu.copy()
        if np.var(residue) < min_energy:
            break
        residue_imfs = run(residue)[0]
        if len(residue_imfs) <= 1:
            if len(imfs) < max_modes and len(residue_imfs) == 1:
                imfs.append(residue)
            break
    return [m * sigma_x for m in imfs], noise_traj, stages
