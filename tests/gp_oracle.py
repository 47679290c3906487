"""Test-local oracle of the celerite likelihood (numpy only; nothing of the package's compute path is imported).

(a) ``dense_loglike``: the covariance matrix written out and a Cholesky factorisation in long double, O(N^3), N <= 48.
(b) ``recursion``: the O(N J^2) celerite2 recursion, vectorised over candidates, in ``np.longdouble`` (the exact side of
    every parity test) or in float64 (what a careful CPU implementation gives: the yardstick of the gate's constant).
(c) ``fold``: per period the best cell, the marginal, and the best period of a cube of likelihoods.

Both take what the device gets: ``tau = t - t[0]`` in float64 and coefficients ``(a, b, c, nu)`` with ``nu = d / 2 pi``
in cycles per time unit:  k(D) = sum_j exp(-c_j |D|) (a_j cos(2 pi nu_j D) + b_j sin(2 pi nu_j |D|)).

THE GATE of a candidate:  |got - exact| <= GATE_CONSTANT * kappa * 2^-53 * mag  with
    kappa = max_n (|A_n| + |U_n| |S_n| |U_n|^T) / D_n      the cancellation in D_n = A_n - U_n S_n U_n^T,
    mag   = sum_n (z_n^2 / D_n + |ln D_n|)                 what ln L is summed from;
with and without a profiled mean alike.  With a profiled mean ln L gains T = q01^2 / q11 (q01 = sum z z1 / D, q11 = sum
z1^2 / D); what that term adds to the sums, 2 |q01| sum |z z1| / D / q11 + T, is returned as ``mag_profile`` and printed by
the tests beside the ratio - it is no part of the gate.
"""
import functools

import numpy as np

LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))
GATE_CONSTANT = 16.0


# ---- kernels: an independent statement of the SHO algebra ----------------------------------------------------------
def sho(S0, w0, Q):
    """``[J][4]`` of (a, b, c, d): one complex term for Q > 1/2, two real ones for Q < 1/2."""
    amp, rate = S0 * w0 * Q, w0 / (2 * Q)
    if Q > 0.5:
        f = np.sqrt(4 * Q * Q - 1)
        return np.array([[amp, amp / f, rate, rate * f]])
    f = np.sqrt(1 - 4 * Q * Q)
    return np.array([[0.5 * amp * (1 + 1 / f), 0.0, rate * (1 - f), 0.0], [0.5 * amp * (1 - 1 / f), 0.0, rate * (1 + f), 0.0]])


def sho_kernel(S0, w0, Q, lag):
    """The SHO covariance in closed form (Foreman-Mackey et al. 2017, eq. 23), for Q < 1/2 and Q > 1/2."""
    lag = np.abs(np.asarray(lag, dtype=float))
    eta = np.sqrt(abs(1 - 1 / (4 * Q * Q)))
    envelope = S0 * w0 * Q * np.exp(-w0 * lag / (2 * Q))
    if Q < 0.5:
        return envelope * (np.cosh(eta * w0 * lag) + np.sinh(eta * w0 * lag) / (2 * eta * Q))
    return envelope * (np.cos(eta * w0 * lag) + np.sin(eta * w0 * lag) / (2 * eta * Q))


def rotation(sigma, period, Q0, dQ, f):
    amp = sigma ** 2 / (1 + f)
    Q1, Q2 = 0.5 + Q0 + dQ, 0.5 + Q0
    w1 = 4 * np.pi * Q1 / (period * np.sqrt(4 * Q1 ** 2 - 1))
    w2 = 8 * np.pi * Q2 / (period * np.sqrt(4 * Q2 ** 2 - 1))
    return np.concatenate([sho(amp / (w1 * Q1), w1, Q1), sho(f * amp / (w2 * Q2), w2, Q2)])


def to_device(terms):
    """(a, b, c, d) -> (a, b, c, nu = d / 2 pi), one float64 division: what both the device and the oracles take."""
    coeff = np.array(terms, dtype=np.float64)
    coeff[..., 3] = coeff[..., 3] / (2 * np.pi)
    return coeff


def kernel_value(coeff, lag, dtype=LD):
    """k(lag) of one candidate's ``[J][4]`` device coefficients."""
    lag = np.abs(np.asarray(lag, dtype=dtype))
    a, b, c, nu = (coeff[:, k].astype(dtype)[:, None] for k in range(4))
    cycles = nu * lag[None, :]
    phase = 2 * PI_LD.astype(dtype) * (cycles - np.rint(cycles))
    return np.sum(np.exp(-c * lag[None, :]) * (a * np.cos(phase) + b * np.sin(phase)), axis=0)


# ---- (a) dense --------------------------------------------------------------------------------------------------------
def cholesky(K):
    """Lower factor of a symmetric positive definite long-double matrix, written out (numpy's is float64 only)."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for i in range(n):
        for j in range(i + 1):
            s = K[i, j] - np.dot(L[i, :j], L[j, :j])
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    return L


def forward(L, rhs):
    out = np.zeros_like(rhs)
    for i in range(L.shape[0]):
        out[i] = (rhs[i] - np.dot(L[i, :i], out[:i])) / L[i, i]
    return out


def dense_loglike(tau, y, var, coeff, jitter=0.0, mean=0.0, fit_mean=False):
    """``(ln L, mean)`` of one candidate by the dense factorisation, in long double."""
    tau = np.asarray(tau, dtype=LD)
    n = tau.size
    K = kernel_value(coeff, (tau[:, None] - tau[None, :]).ravel()).reshape(n, n)
    K[np.arange(n), np.arange(n)] += np.asarray(var, dtype=LD) + LD(jitter)
    L = cholesky(K)
    zy = forward(L, np.asarray(y, dtype=LD) - (LD(0) if fit_mean else LD(mean)))
    ll = -0.5 * np.dot(zy, zy) - np.sum(np.log(np.diag(L))) - 0.5 * n * np.log(2 * PI_LD)
    if not fit_mean:
        return ll, LD(mean)
    z1 = forward(L, np.ones(n, dtype=LD))
    q01, q11 = np.dot(zy, z1), np.dot(z1, z1)
    return ll + 0.5 * q01 * q01 / q11, q01 / q11


# ---- (b) the recursion ------------------------------------------------------------------------------------------------
def recursion(tau, y, var, coeff, jitter=0.0, mean=None, fit_mean=False, dtype=LD):
    """The celerite2 recursion for ``coeff`` ``[M][J][4]``.  Returns a dict of ``[M]`` arrays: ``loglike`` (-inf where a
    D_n is not positive and finite), ``mean``, ``status`` (0 or the 1-based sample of the first such D_n), ``mag`` and
    ``kappa`` of the gate, ``mean_mag`` of ``mean_gate``, ``mag_profile`` (a figure to print, see above)."""
    coeff = np.asarray(coeff, dtype=np.float64)
    M, J = coeff.shape[:2]
    R = 2 * J
    two_pi = (2 * PI_LD).astype(dtype)
    a, b, c, nu = (coeff[:, :, k].astype(dtype) for k in range(4))
    tau = np.asarray(tau, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    var = np.asarray(var, dtype=dtype)
    diag = np.broadcast_to(np.asarray(jitter, dtype=dtype), (M,)) + np.sum(a, axis=1)
    mu = np.zeros(M, dtype=dtype) if (fit_mean or mean is None) else np.broadcast_to(np.asarray(mean, dtype=dtype), (M,))
    S = np.zeros((M, R, R), dtype=dtype)
    f = np.zeros((M, R), dtype=dtype)
    f1 = np.zeros((M, R), dtype=dtype)
    q, q01, q11, m01 = (np.zeros(M, dtype=dtype) for _ in range(4))
    lnd, mag, kappa = (np.zeros(M, dtype=dtype) for _ in range(3))
    status = np.zeros(M, dtype=np.int32)
    U = np.zeros((M, R), dtype=dtype)
    V = np.zeros((M, R), dtype=dtype)
    P = np.zeros((M, R), dtype=dtype)
    W = np.zeros((M, R), dtype=dtype)
    D = np.ones(M, dtype=dtype)
    z = np.zeros(M, dtype=dtype)
    z1 = np.zeros(M, dtype=dtype)
    with np.errstate(all="ignore"):
        for n in range(tau.size):
            cycles = nu * tau[n]
            phase = two_pi * (cycles - np.rint(cycles))
            cs, sn = np.cos(phase), np.sin(phase)
            U[:, 0::2], U[:, 1::2] = a * cs + b * sn, a * sn - b * cs
            V[:, 0::2], V[:, 1::2] = cs, sn
            if n > 0:
                decay = np.exp(-c * (tau[n] - tau[n - 1]))
                P[:, 0::2], P[:, 1::2] = decay, decay
                S = P[:, :, None] * (S + D[:, None, None] * W[:, :, None] * W[:, None, :]) * P[:, None, :]
                f = P * (f + W * z[:, None])
                f1 = P * (f1 + W * z1[:, None])
            SU = np.einsum("mik,mk->mi", S, U)
            usu = np.einsum("mi,mi->m", U, SU)
            A = var[n] + diag
            D = A - usu
            W = (V - SU) / D[:, None]
            z = (y[n] - mu) - np.einsum("mi,mi->m", U, f)
            z1 = 1 - np.einsum("mi,mi->m", U, f1)
            bad = ~((D > 0) & np.isfinite(D))
            status = np.where((status == 0) & bad, n + 1, status).astype(np.int32)
            q += z * z / D
            q01 += z * z1 / D
            q11 += z1 * z1 / D
            m01 += np.abs(z * z1) / D
            lnd += np.log(D)
            mag += z * z / D + np.abs(np.log(D))
            kappa = np.maximum(kappa, (np.abs(A) + np.einsum("mi,mik,mk->m", np.abs(U), np.abs(S), np.abs(U))) / D)
        ll = -0.5 * (q + lnd) - 0.5 * tau.size * np.log(two_pi)
        out_mean = mu.copy()
        mean_mag = np.abs(mu)
        mag_profile = np.zeros(M, dtype=dtype)
        if fit_mean:
            mean_mag = m01 / q11 + np.abs(q01 / q11)
            ll = ll + 0.5 * q01 * q01 / q11
            out_mean = q01 / q11
            mag_profile = (2 * np.abs(q01) * m01 + q01 * q01) / q11
    failed = status != 0
    return dict(loglike=np.where(failed, -np.inf, ll), mean=np.where(failed, np.nan, out_mean), status=status,
                mag=mag, kappa=kappa, mean_mag=mean_mag, mag_profile=mag_profile)


def mean_gate(exact):
    """The allowed |mean - exact mean| of a profiled mean q01 / q11: the roundings of q01 (absolute sum m01) and q11 by
    the same kappa, GATE_CONSTANT * kappa * 2^-53 * (m01 / q11 + |mean|)."""
    return (GATE_CONSTANT * exact["kappa"] * 2.0 ** -53 * exact["mean_mag"]).astype(np.float64)


def gate(exact):
    """The allowed |got - exact| per candidate, from the long-double run."""
    return (GATE_CONSTANT * exact["kappa"] * 2.0 ** -53 * exact["mag"]).astype(np.float64)


def ratio(got, exact):
    """max over candidates of |got - exact| / gate (every candidate of ``exact`` must be positive definite)."""
    assert np.all(exact["status"] == 0)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - exact["loglike"]).astype(np.float64) / gate(exact)))


# ---- (c) the fold -----------------------------------------------------------------------------------------------------
def fold(cube):
    """``(profile, cell, marginal, best)`` of a ``[np][nq]`` cube: per period the largest finite value (the first of equal
    ones; NaN and -1 if none), ln of the mean of exp over all nq cells counting the finite ones (-inf if none), and
    ``best`` = (value, period, cell) of the largest profile value (the first; NaN, -1, -1 if none)."""
    cube = np.asarray(cube, dtype=np.float64)
    n_periods, nq = cube.shape
    profile, marginal = np.full(n_periods, np.nan), np.full(n_periods, -np.inf)
    cell = np.full(n_periods, -1, dtype=np.int32)
    for i, row in enumerate(cube):
        ok = np.isfinite(row)
        if not ok.any():
            continue
        profile[i] = row[ok].max()
        cell[i] = int(np.flatnonzero(ok & (row == profile[i]))[0])
        total = 0.0
        for v in row[ok]:            # in ascending cell order, as the device adds them
            total += np.exp(v - profile[i])
        marginal[i] = (profile[i] + np.log(total)) - np.log(float(nq))
    if np.all(cell < 0):
        return profile, cell, marginal, (np.nan, -1, -1)
    at = int(np.nanargmax(profile))
    return profile, cell, marginal, (float(profile[at]), at, int(cell[at]))


# ---- inputs -----------------------------------------------------------------------------------------------------------
PERIOD = 3.1


def curve(n, seed=5):
    """Uniform times on [0, 80] with one duplicate (from 3 samples on), a sine of period 3.1 plus 0.05 noise, and
    err^2 in [1e-4, 4e-3].  Returns ``(tau, y, var)`` with tau[0] == 0."""
    rng = np.random.default_rng(seed + 1000 * n)
    t = np.sort(rng.uniform(0.0, 80.0, n))
    if n >= 3:
        t[n // 2] = t[n // 2 - 1]
    var = rng.uniform(1e-4, 4e-3, n)
    y = np.sin(2 * np.pi * t / PERIOD) + 0.05 * rng.standard_normal(n)
    return t - t[0], y, var


def kernels(J, M):
    """``[M][J][4]`` device coefficients: every family of J terms in turn, at periods spread over [2, 6] - complex and
    real terms, overdamped oscillators with their negative amplitude, quality factors up to Q0 = 300.  Every kernel has
    k(0) <= 0.35, so with the curve's err^2 + jitter <= 4.3e-3 every D_n <= A_n < 1 / e and every |ln D_n| > 1: mag
    exceeds N.  (mag leaves out the constant N/2 ln 2 pi of ln L; a kernel with A_n near 1 and a short curve makes mag -
    and the gate - smaller than the spacing of doubles at ln L itself, which no float64 result can meet.)"""
    out = []
    for m in range(M):
        p = 2.0 + 4.0 * ((m * 37) % 101) / 100.0
        w = 2 * np.pi / p
        pick = m % 3
        if J == 1:
            terms = [sho(0.3 / (w * 3.0), w, 3.0), np.array([[0.25, 0.0, 0.3 / p, 0.0]]), sho(0.2 / (w * 40.0), w, 40.0)][pick]
        elif J == 2:
            terms = [rotation(0.5, p, 2.0, 1.0, 0.5), rotation(0.45, p, 300.0, 0.5, 0.2), sho(0.25 / (w * 0.1), w, 0.1)][pick]
        elif J == 3:
            terms = [np.concatenate([sho(0.2 / (w * 5.0), w, 5.0), sho(0.1 / (w * 0.05), w, 0.05)]),
                     np.concatenate([rotation(0.4, p, 20.0, 1.0, 0.5), np.array([[0.1, 0.0, 0.05, 0.0]])]),
                     np.concatenate([np.array([[0.1, 0.0, 0.1, 0.0]]), sho(0.2 / (w * 0.2), w, 0.2)])][pick]
        else:
            terms = [np.concatenate([rotation(0.5, p, 2.0, 1.0, 0.5), sho(0.08 / (w * 0.05), w, 0.05)]),
                     np.concatenate([rotation(0.4, p, 300.0, 2.0, 0.3), rotation(0.3, 1.7 * p, 5.0, 0.0, 1.0)]),
                     np.concatenate([sho(0.15 / (w * 0.3), w, 0.3), sho(0.1 / (2 * w * 0.02), 2 * w, 0.02)])][pick]
        assert np.sum(terms[:, 0]) <= 0.35
        assert terms.shape == (J, 4)
        out.append(terms)
    return to_device(np.array(out))


JITTER = 2.5e-4


@functools.lru_cache(maxsize=None)
def parity_case(J, n, M, fit_mean):
    """A curve, M kernels and the long-double answer, computed once and shared (read-only)."""
    tau, y, var = curve(n)
    coeff = kernels(J, M)
    exact = recursion(tau, y, var, coeff, JITTER, fit_mean=fit_mean)
    for v in (tau, y, var, coeff, *exact.values()):
        v.setflags(write=False)
    return tau, y, var, coeff, exact


def spot_curve(n=120, seed=21):
    """Uneven samples of a spot-like signal of period 3.1: two harmonics whose phase wanders slowly (a decaying
    coherence), noise 0.05.  Returns ``(t, y, err)``."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 40.0, n))
    drift = 0.25 * np.sin(2 * np.pi * t / 17.0)
    y = np.sin(2 * np.pi * t / PERIOD + drift) + 0.4 * np.sin(4 * np.pi * t / PERIOD + 1.0 + 2 * drift)
    err = rng.uniform(0.03, 0.07, n)
    return t, y + err * rng.standard_normal(n), err
