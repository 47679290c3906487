"""Test-local oracle of the Keplerian periodogram (include/periodicity_hip.h, pdc_kepler_scan).  Plain numpy, nothing
from the package.  The reference has no such statistic - PARITY UNPINNED BY THE REFERENCE.

Nothing here is shared with the kernel: the phase frac(f t') comes from an error-free product (Veltkamp split, Dekker
product, exact in float64) whose two parts are reduced and added in long double; Kepler's equation is solved by a
bracketed Newton iteration with a bisection fallback, run to a fixed point, from the middle of the bracket (no starter);
cos nu and sin nu are taken in the textbook form; the normal equations are solved in long double by an LDL^T
factorisation typed out for up to three columns.  ``cond`` is np.linalg.cond of the float64 normal matrix.

Keep rule (the one of tests/mhgls_oracle.py): cells with cond <= 1e6 are held to Tier E, |got - exact| <= 1e-6 |exact|
+ 1e-9; every other cell must be NaN or finite; at most 5 % of a cube may be left out."""
import numpy as np

LD = np.longdouble
COND_LIMIT = 1e6
LEFT_OUT_CAP = 0.05
PI = LD(4) * np.arctan(LD(1))

# the parity input of tests/test_kepler_gpu.py: an orbit of P = 17.3, e = 0.6, omega = 1.1, K = 30, periastron at t = 4
PERIOD, ECC, OMEGA, SEMI_AMPLITUDE, T_PERI = 17.3, 0.6, 1.1, 30.0, 4.0
BEST_BIN, BEST_ECC = 38, 0.6


def solve_kepler(M, e, dtype=LD):
    """E with E - e sin E = M for M in [0, pi] (arrays broadcast), to a fixed point of the bracketed iteration (or to
    the pair of neighbouring values it alternates between)."""
    M, e = np.broadcast_arrays(np.asarray(M, dtype=dtype), np.asarray(e, dtype=dtype))
    lo, hi = np.zeros(M.shape, dtype=dtype), np.full(M.shape, PI, dtype=dtype)
    E = before = (lo + hi) / 2
    for _ in range(200):
        g = E - e * np.sin(E) - M
        lo, hi = np.where(g < 0, E, lo), np.where(g > 0, E, hi)
        step = E - g / (1 - e * np.cos(E))
        step = np.where((step >= lo) & (step <= hi), step, (lo + hi) / 2)
        if np.all((step == E) | (step == before)):   # a fixed point, or the two neighbours it alternates between
            break
        before, E = E, step
    return E


def true_anomaly(cycles, e, dtype=LD):
    """(cos nu, sin nu) at mean anomaly ``cycles`` (already in long double where the caller has it exactly)."""
    m = np.asarray(cycles, dtype=dtype)
    m = m - np.rint(m)
    e = np.asarray(e, dtype=dtype)
    E = solve_kepler(2 * PI.astype(dtype) * np.abs(m), e, dtype)
    inv = 1 / (1 - e * np.cos(E))
    return (np.cos(E) - e) * inv, np.sign(m) * np.sqrt(1 - e * e) * np.sin(E) * inv


def exact_cycles(a, b):
    """frac(a * b) in long double from the error-free float64 product."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    hi = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    a1, b1 = ca - (ca - a), cb - (cb - b)
    a2, b2 = a - a1, b - b1
    lo = ((a1 * b1 - hi) + a1 * b2 + a2 * b1) + a2 * b2     # hi + lo == a * b exactly
    return (hi - np.rint(hi)).astype(LD) + lo.astype(LD)


def _weights(y, err, fit_mean, dtype):
    y = np.asarray(y, dtype=dtype)
    w = np.ones(y.size, dtype=dtype) if err is None else np.asarray(err, dtype=dtype) ** -2
    W = w.sum()
    w = w / W
    ybar = (w * y).sum() if fit_mean else dtype(0)
    return w, y - ybar, W, ybar


def _quadratic(Mat, b):
    """b^T M^-1 b for stacks of symmetric matrices [..., D, D] and vectors [..., D], D <= 3, by LDL^T."""
    D = b.shape[-1]
    L = np.zeros(Mat.shape, dtype=Mat.dtype)
    d = np.zeros(b.shape, dtype=Mat.dtype)
    z = np.zeros(b.shape, dtype=Mat.dtype)
    with np.errstate(all="ignore"):
        for j in range(D):
            d[..., j] = Mat[..., j, j] - sum(L[..., j, q] ** 2 * d[..., q] for q in range(j))
            z[..., j] = b[..., j] - sum(L[..., j, q] * z[..., q] for q in range(j))
            for i in range(j + 1, D):
                L[..., i, j] = (Mat[..., i, j] - sum(L[..., i, q] * L[..., j, q] * d[..., q] for q in range(j))) / d[..., j]
        return (z * z / d).sum(axis=-1)


def _normal(cols, w, yc):
    """Normal matrix [..., D, D] and right-hand side [..., D] of design columns [..., n] each."""
    D = len(cols)
    shape = np.broadcast_shapes(*(c.shape for c in cols))[:-1]
    Mat = np.empty(shape + (D, D), dtype=w.dtype)
    b = np.empty(shape + (D,), dtype=w.dtype)
    for r in range(D):
        b[..., r] = (w * yc * cols[r]).sum(axis=-1)
        for c in range(r + 1):
            Mat[..., r, c] = Mat[..., c, r] = (w * cols[r] * cols[c]).sum(axis=-1)
    return Mat, b


def anomalies(t, freq, ecc, m0, dtype=LD):
    """(cos nu, sin nu) [nf][ne][nm][n] of every cell and sample: what a cube costs, and all that does not depend on
    the values, the weights or the options."""
    t = np.asarray(t, dtype=np.float64)
    freq, ecc, m0 = (np.asarray(a, dtype=np.float64) for a in (freq, ecc, m0))
    phi = exact_cycles(freq[:, None], (t - t[0])[None, :])                       # [nf][n]
    cycles = (phi[:, None, None, :] - m0.astype(LD)[None, None, :, None]).astype(dtype)
    return true_anomaly(cycles, ecc[None, :, None, None], dtype)


def cube(t, y, err, freq, ecc, m0, fit_mean=True, psd=False, dtype=LD, nu=None):
    """(cells [nf][ne][nm] in ``dtype``, cond [nf][ne][nm] of the float64 normal matrix); ``nu``: the result of
    ``anomalies`` for the same times, grid and lists, where the caller keeps it."""
    w, yc, W, _ = _weights(y, err, fit_mean, dtype)
    YY = (w * yc * yc).sum()
    c, s = anomalies(t, freq, ecc, m0, dtype) if nu is None else nu
    cols = [c, s] + ([np.ones_like(c)] if fit_mean else [])
    Mat, b = _normal(cols, w, yc)
    quad = _quadratic(Mat, b)
    with np.errstate(all="ignore"):
        cond = np.linalg.cond(Mat.astype(np.float64))
        value = quad * (W / 2) if psd else quad / YY
    return value, cond


def gls_power(t, y, err, freq, fit_mean=True, dtype=LD):
    """The GLS power by the closed form of Zechmeister & Kurster 2009 (eqs. 4-15), nothing shared with ``cube``."""
    t = np.asarray(t, dtype=np.float64)
    w, yc, _, _ = _weights(y, err, fit_mean, dtype)
    arg = 2 * PI.astype(dtype) * exact_cycles(np.asarray(freq)[:, None], (t - t[0])[None, :]).astype(dtype)
    co, si = np.cos(arg), np.sin(arg)
    C, S = (w * co).sum(axis=1), (w * si).sum(axis=1)
    if not fit_mean:
        C, S = 0 * C, 0 * S
    YY = (w * yc * yc).sum()
    YC, YS = (w * yc * co).sum(axis=1), (w * yc * si).sum(axis=1)
    CC, SS, CS = (w * co * co).sum(axis=1) - C * C, (w * si * si).sum(axis=1) - S * S, (w * co * si).sum(axis=1) - C * S
    return (SS * YC ** 2 + CC * YS ** 2 - 2 * CS * YC * YS) / (YY * (CC * SS - CS ** 2))


def fit(t, y, err, f, e, m0, fit_mean=True):
    """The long-double orbit at one cell: dict K, omega, gamma (y = K (cos(nu + omega) + e cos omega) + gamma)."""
    t = np.asarray(t, dtype=np.float64)
    w, yc, _, ybar = _weights(y, err, fit_mean, LD)
    c, s = true_anomaly(exact_cycles(f, t - t[0]) - LD(m0), e)
    cols = [c, s] + ([np.ones_like(c)] if fit_mean else [])
    Mat, b = _normal(cols, w, yc)
    D = len(cols)
    # Cramer's rule in long double (D <= 3)
    det = _det(Mat)
    theta = []
    for k in range(D):
        Mk = Mat.copy()
        Mk[:, k] = b
        theta.append(_det(Mk) / det)
    A, B = theta[0], theta[1]
    const = theta[2] if fit_mean else LD(0)
    return {"K": float(np.hypot(A, B)), "omega": float(np.arctan2(-B, A) % (2 * PI)), "gamma": float(const - A * LD(e) + ybar)}


def _det(M):
    if M.shape[0] == 2:
        return M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
            + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


def compare(got, want, cond):
    """(worst |got - want| / gate over the kept cells, share left out); the cells left out must be NaN or finite."""
    got = np.asarray(got, dtype=np.float64)
    keep = cond <= COND_LIMIT
    assert not np.any(np.isinf(got)), "a cell is infinite"
    want64 = np.asarray(want, dtype=np.float64)
    gate = 1e-6 * np.abs(want64[keep]) + 1e-9
    with np.errstate(invalid="ignore"):
        err = np.abs(got[keep].astype(LD) - np.asarray(want, dtype=LD)[keep]).astype(np.float64)
    err = np.where(np.isnan(err), np.inf, err)   # a kept cell must have a value
    return (float(np.max(err / gate)) if keep.any() else 0.0), float(1 - keep.mean())


def reductions(cells):
    """(power [nf], cell [nf] int32, best = (value, bin, cell)) of a cube by np.nanmax / np.nanargmax."""
    flat = np.asarray(cells).reshape(cells.shape[0], -1)
    some = ~np.all(np.isnan(flat), axis=1)
    cell = np.full(flat.shape[0], -1, dtype=np.int32)
    power = np.full(flat.shape[0], np.nan)
    if some.any():
        cell[some] = np.nanargmax(flat[some], axis=1)
        power[some] = flat[some, cell[some]]
    if not some.any():
        return power, cell, (np.nan, -1, -1)
    j = int(np.nanargmax(power))
    return power, cell, (float(power[j]), j, int(cell[j]))


def signal(t, period=PERIOD, e=ECC, omega=OMEGA, K=SEMI_AMPLITUDE, t_peri=T_PERI):
    c, s = true_anomaly((np.asarray(t, dtype=LD) - LD(t_peri)) / LD(period), e)
    c, s = c.astype(np.float64), s.astype(np.float64)
    return K * (c * np.cos(omega) - s * np.sin(omega) + e * np.cos(omega))


def kepler_curve(n, offset=0.0):
    """(t, y, err, freq, ecc, m0): ``n`` samples of the orbit above on [0, 200) with noise of 1 .. 3 and an offset of
    100; 80 bins from 0.02, 7 eccentricities to 0.9, 12 phases.  ``offset`` moves the times only (a Julian date)."""
    rng = np.random.default_rng(20261021 + n)
    t = np.sort(rng.uniform(0, 200, n))
    err = rng.uniform(1, 3, n)
    y = signal(t) + err * rng.standard_normal(n) + 100
    return t + offset, y, err, 0.02 + 0.001 * np.arange(80), np.linspace(0, 0.9, 7), np.arange(12) / 12


def many_cycles_curve():
    """64 samples over a baseline of 1e6, 8 bins near 0.1 (f t' reaches 1e5 cycles), 3 x 4 cells; the orbit has the
    period of bin 3 so that the cells are well conditioned and differ."""
    rng = np.random.default_rng(20261021)
    t = np.sort(rng.uniform(0, 1e6, 64))
    err = rng.uniform(1, 3, 64)
    freq = 0.1 + 1e-7 * np.arange(8)
    y = signal(t, period=1 / freq[3], t_peri=2.0) + err * rng.standard_normal(64) + 100
    return t, y, err, freq, np.array([0.0, 0.5, 0.9]), np.arange(4) / 4


# ---- the small inputs of the seam tests: 24 samples, few bins, few cells ----------------------------------------------
def tile_seam_case(nf):
    """``nf`` bins on [0.02, 0.1), 2 x 2 cells."""
    t, y, err = kepler_curve(24)[:3]
    return t, y, err, 0.02 + (0.08 / nf) * np.arange(nf), np.array([0.0, 0.6]), np.array([0.0, 0.5])


def cell_seam_case(count):
    """8 bins, ``count`` cells as the most nearly square ne x nm."""
    t, y, err = kepler_curve(24)[:3]
    ne = max(d for d in range(1, int(count ** 0.5) + 1) if count % d == 0)
    ecc = np.linspace(0.9, 0.0, ne) if ne > 1 else np.array([0.5])
    return t, y, err, 0.03 + 0.009 * np.arange(8), ecc, (0.3 + np.arange(count // ne) / (count // ne)) % 1


def no_trace_case():
    """8 bins, 5 x 6 cells up to the cap on e."""
    t, y, err = kepler_curve(24)[:3]
    return t, y, err, 0.03 + 0.009 * np.arange(8), np.array([0.0, 0.3, 0.6, 0.9, 0.95]), np.arange(6) / 6


def slab_case():
    """600 bins (three tiles), 2 x 3 cells."""
    t, y, err = kepler_curve(24)[:3]
    return t, y, err, 0.02 + (0.08 / 600) * np.arange(600), np.array([0.0, 0.6]), np.arange(3) / 3
