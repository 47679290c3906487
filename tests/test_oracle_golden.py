"""The oracle against the golden vectors generated from the reference's own code
(tests/golden/make_golden.py), including both known-answer tests of
/root/reference/tests/test_spectral.py.  CPU only."""
import os

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import scan_oracle as so


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def test_reference_grid_known_answer(golden_dir):
    # tests/test_spectral.py:7-24
    g = load(golden_dir, "g1_grid")
    t0, ts = 2.5, 0.1
    freq, df, fmin = so.gls_grid(g["time"], n=1)
    assert np.array_equal(freq, g["frequency"])
    assert sorted(freq) == list(freq)
    assert freq[0] == (1 / t0) / 2
    assert np.round(freq[-1], 6) == (1 / ts) / 2
    assert np.max(np.abs(np.diff(freq) - 1 / t0)) < 1e-10


def test_reference_sine_known_answer(golden_dir):
    # tests/test_spectral.py:27-31: period_at_highest_peak == 10.0 exactly, index 49 of 248
    from periodicity_amd.core import FSeries
    g = load(golden_dir, "g2_sine100")
    freq, power = so.gls(np.arange(100), g["values"])
    assert np.array_equal(freq, g["frequency"]) and freq.size == 248
    assert np.array_equal(power, g["power_ref"])
    assert int(np.nanargmax(power)) == int(g["argmax"]) == 49
    assert FSeries(freq, power).period_at_highest_peak == 10.0 == float(g["period_at_highest_peak"])
    exact = so.gls(np.arange(100), g["values"], sums="exact")[1]
    # integer times: bin 148 is an exact zero and the last bin sits on the Nyquist singularity
    # (sin(pi t) == 0 -> 0/0), both pure rounding noise in any implementation
    ok = np.abs(g["power_exact"]) > 1e-20
    ok[-1] = False
    np.testing.assert_allclose(exact[ok], g["power_exact"][ok], rtol=1e-9)
    assert int(np.nanargmax(exact)) == 49


@pytest.mark.parametrize("fit_mean", [True, False])
@pytest.mark.parametrize("psd", [False, True])
def test_spotted_star_fft_path_is_bit_exact(golden_dir, fit_mean, psd):
    g = load(golden_dir, "g3_spotted_star")
    freq, power = so.gls(g["t"], g["y"], g["dy"], fit_mean=fit_mean, psd=psd)
    assert np.array_equal(freq, g["frequency"])
    assert np.array_equal(power, g[f"power_ref_fm{int(fit_mean)}_psd{int(psd)}"])


def test_spotted_star_exact_path(golden_dir):
    g = load(golden_dir, "g3_spotted_star")
    sel = slice(0, 1500)
    f = g["frequency"]
    for fm in (True, False):
        p = co.gls_power_exact(g["t"], g["y"], g["dy"], f[sel], fit_mean=fm)
        np.testing.assert_allclose(p, g[f"power_exact_fm{int(fm)}_psd0"][sel], rtol=2e-8)
    p = co.gls_power_exact(g["t"], g["y"], None, f[sel])
    np.testing.assert_allclose(p, g["power_exact_noerr"][sel], rtol=2e-8)
    # tier R fact: the approximate and the exact spectrum peak in the same bin
    assert np.argmax(g["power_exact_fm1_psd0"]) == np.argmax(g["power_ref_fm1_psd0"])


@pytest.mark.parametrize("n", [1000, 5000])
def test_synthetic_seams_and_power(golden_dir, n):
    g = load(golden_dir, f"g4_synth{n}")
    t, y, dy, f = g["t"], g["y"], g["dy"], g["frequency"]
    df, fmin = float(g["df"]), float(g["fmin"])
    w, yc, _ = so.gls_weights(y, dy, True)
    S, C = so.trig_sum_fft(t, w, df, f.size, fmin)
    assert np.array_equal(S, g["S_fft"]) and np.array_equal(C, g["C_fft"])
    Sh, Ch = so.trig_sum_fft(t, w * yc, df, f.size, fmin)
    assert np.array_equal(Sh, g["Sh_fft"]) and np.array_equal(Ch, g["Ch_fft"])
    S2, C2 = so.trig_sum_fft(t, w, 2 * df, f.size, 2 * fmin)
    assert np.array_equal(S2, g["S2_fft"]) and np.array_equal(C2, g["C2_fft"])
    assert np.array_equal(so.gls(t, y, dy)[1], g["power_ref"])
    sel = slice(0, 600)
    Se, Ce = so.trig_sum_exact(t, w * yc, f[sel])
    np.testing.assert_allclose(Se, g["Sh_exact"][sel], rtol=0, atol=1e-13)
    np.testing.assert_allclose(Ce, g["Ch_exact"][sel], rtol=0, atol=1e-13)
    Sc, Cc = co.trig_sums_exact(t, w * yc, f[sel])
    np.testing.assert_allclose(Sc, Se, rtol=0, atol=1e-15)
    np.testing.assert_allclose(Cc, Ce, rtol=0, atol=1e-15)
    p = co.gls_power_exact(t, y, dy, f)
    np.testing.assert_allclose(p, g["power_exact"], rtol=1e-8)


def test_window_and_bootstrap(golden_dir):
    g = load(golden_dir, "g5_window")
    freq, df, fmin = so.gls_grid(g["t"])
    p = so.gls_power(g["t"], np.ones_like(g["t"]), None, freq, df, fmin, fit_mean=False)
    assert np.array_equal(p, g["power_ref"])
    g = load(golden_dir, "g6_bootstrap")
    reps = so.gls_bootstrap_maxima(g["t"], g["y"], g["dy"], 20, random_seed=42)
    assert np.array_equal(reps, g["replicates_ref"])
    assert np.mean(0.3 < reps) == float(g["fap_at_0p3_ref"])
    assert np.quantile(reps, 0.9) == float(g["fal_at_0p1_ref"])


@pytest.mark.parametrize("nb,nc", [(5, 2), (10, 3)])
def test_pdm_seam_and_call(golden_dir, nb, nc):
    g = load(golden_dir, "g7_pdm")
    periods = g[f"periods_{nb}_{nc}"]
    theta = so.pdm_scan(g["t"], g["y"], periods, nb, nc)
    assert np.array_equal(theta, g[f"theta_seam_{nb}_{nc}"])
    freq, th = so.pdm(g["t"], g["y"], nb, nc, p_min=1.0, p_max=60.0, n_periods=200)
    assert np.array_equal(freq, g[f"frequency_{nb}_{nc}"])
    assert np.array_equal(th, g[f"theta_call_{nb}_{nc}"])
    np.testing.assert_allclose(co.pdm_scan(g["t"], g["y"], periods, nb, nc), theta, rtol=1e-13)


def test_pdm_variants(golden_dir):
    g = load(golden_dir, "g7_pdm")
    freq, th = so.pdm(g["t"], g["y"], p_min=1.0, p_max=60.0, n_periods=200, do_subharmonic=True)
    assert np.array_equal(freq, g["frequency_sub"]) and np.array_equal(th, g["theta_call_sub"])
    freq, th = so.pdm(g["t"], g["y"], n_periods=150)
    assert np.array_equal(freq, g["frequency_default"])
    assert np.array_equal(th, g["theta_call_default"])
    freq, th = so.pdm(g["t_negative"], g["y"], p_min=1.0, p_max=60.0, n_periods=200)
    assert np.array_equal(th, g["theta_call_negative"])
    assert float(g["sigma"]) == np.var(g["y"], ddof=1)


def test_stringlength_seam(golden_dir):
    g = load(golden_dir, "g8_stringlength")
    assert np.array_equal(so.stringlength_scale(g["y"]), g["m"])
    assert np.array_equal(so.stringlength_periods(g["t"][-1] - g["t"][0], 0.1, 200), g["periods"])
    assert np.array_equal(so.stringlength_scan(g["t"], g["m"], g["periods"]), g["ell"])
    assert np.array_equal(so.stringlength_scan(g["t_even"], g["m_even"], g["periods_even"]),
                          g["ell_even"])
    np.testing.assert_allclose(co.stringlength_scan(g["t"], g["m"], g["periods"]), g["ell"],
                               rtol=1e-13)
    np.testing.assert_allclose(co.stringlength_scan(g["t_even"], g["m_even"], g["periods_even"]),
                               g["ell_even"], rtol=1e-13)


# ---- the two scans the reference only lists as TODO (phase.py:11-15) ---------------------------------
def test_aov_restatement_is_tied_to_the_reference_pdm():
    """With non-overlapping bins (nc = 1) Stellingwerf's theta and the AoV statistic are functions of the
    same two sums of squares: Theta_AoV = ((N - 1) / theta - (N - r)) / (r - 1).  `pdm_scan` is pinned bit
    for bit to the reference's `_pdm` (test_oracle_vs_reference, G7), so this ties the AoV restatement -
    its bins, means and degrees of freedom - to code the reference does have."""
    rng = np.random.default_rng(41)
    n = 3000
    t = np.sort(rng.uniform(0, float(n), n)) - 400.0
    x = 1.0 + 0.5 * np.sin(2 * np.pi * t / 13.7) + 0.1 * rng.standard_normal(n)
    periods = np.linspace(2.0, 50.0, 60)
    for r in (5, 10, 16):
        theta = so.pdm_scan(t, x, periods, nb=r, nc=1)
        np.testing.assert_allclose(so.aov_scan(t, x, periods, r), ((n - 1) / theta - (n - r)) / (r - 1), rtol=1e-10)


def test_aov_restatement_is_scipy_one_way_anova():
    """An independent third-party pin of the AoV restatement: Theta_AoV is the one-way ANOVA F statistic of
    the samples grouped by phase bin; scipy.stats.f_oneway over groups built with numpy alone."""
    from scipy.stats import f_oneway
    rng = np.random.default_rng(321)
    n = 4000
    t = np.sort(rng.uniform(0, float(n), n)) - 77.25
    x = 1.0 + 0.5 * np.sin(2 * np.pi * t / 13.7) + rng.uniform(0.05, 0.2, n) * rng.standard_normal(n)
    periods = np.concatenate([np.linspace(1.5, 50.0, 40), [13.7, 27.4, 6.85]])
    for r in (4, 10, 16):
        mine = so.aov_scan(t, x, periods, r)
        for i, period in enumerate(periods):
            phi = (t / period) % 1
            k = np.clip(np.searchsorted(np.arange(r + 1) / r, phi, side="right") - 1, 0, r - 1)
            f_stat = f_oneway(*[x[k == j] for j in range(r)]).statistic
            assert abs(mine[i] / f_stat - 1) < 1e-10


def test_conditional_entropy_restatement_equals_joint_minus_marginal_entropy():
    """H_c = H(m, phi) - H(phi), computed here with numpy's own 2-d histogram and scipy's entropy."""
    from scipy.stats import entropy
    rng = np.random.default_rng(43)
    n = 4000
    t = np.sort(rng.uniform(0, float(n), n))
    x = np.sin(2 * np.pi * t / 7.3) + 0.3 * rng.standard_normal(n)
    mag = so.magnitude_bins(x, 6)
    for period in (3.1, 7.3, 14.6, 29.0):
        phi = (t / period) % 1
        cells, _, _ = np.histogram2d(phi, mag, bins=(12, 6), range=((0.0, 1.0), (-0.5, 5.5)))
        want = entropy(cells.ravel()) - entropy(cells.sum(axis=1))
        np.testing.assert_allclose(so.cond_entropy(t, mag, period, 12, 6), want, rtol=1e-10)


def test_gregory_loredo_restatement_is_the_multinomial_multiplicity():
    """An independent pin of the Gregory-Loredo restatement: m^N / W_m with W_m = N! / prod n_j! in exact
    integer arithmetic (math.factorial), the bin counts of every offset from numpy's own histogram of the
    shifted phases."""
    import math
    rng = np.random.default_rng(99)
    t = np.sort(rng.uniform(0, 400.0, 150))
    for period, m, n_off in ((7.3, 3, 4), (19.1, 5, 2), (2.2, 2, 8), (50.0, 4, 1)):
        phi = (t / period) % 1
        terms = []
        for off in range(n_off):
            shifted = (phi - off / (m * n_off)) % 1
            counts, _ = np.histogram(shifted, bins=m, range=(0.0, 1.0))
            w = math.factorial(t.size)
            for c in counts:
                w //= math.factorial(int(c))
            terms.append(m ** t.size / w)          # exact rational -> float
        want = math.log(sum(terms) / n_off)
        assert abs(so.gl_log_s(t, period, m, n_off) - want) < 1e-9 * abs(want)
    assert np.isnan(so.gl_log_s(np.array([np.nan, np.nan]), 3.0, 2, 2))


# ---- the fast C checkers used for EXHAUSTIVE parity at the BASELINE sizes ------------------------------
@pytest.mark.parametrize("n", [1000, 5000])
def test_double_precision_direct_sums_are_pinned_to_the_long_double_ones(golden_dir, n):
    """`oracle_gls_sums_f64` (pairwise evaluation in double: exact cycle reduction + Cephes polynomials) against
    the goldens' long-double seam sums and spectrum - the chain that lets the GPU suite check ALL 1e6 bins of C2."""
    g = load(golden_dir, f"g4_synth{n}")
    t, y, dy, f = g["t"], g["y"], g["dy"], g["frequency"]
    w, yc, _ = so.gls_weights(y, dy, True)
    Sh, Ch, S, C, S2, C2 = co.gls_sums_f64(t, w * yc, w, f)
    scale_h, scale_w = np.abs(w * yc).sum(), np.abs(w).sum()
    assert np.max(np.abs(Sh - g["Sh_exact"])) <= 1e-13 * scale_h and np.max(np.abs(Ch - g["Ch_exact"])) <= 1e-13 * scale_h
    Se, Ce = co.trig_sums_exact(t, w, f)
    S2e, C2e = co.trig_sums_exact(t, w, 2 * f)
    for got, want in ((S, Se), (C, Ce), (S2, S2e), (C2, C2e)):
        assert np.max(np.abs(got - want)) <= 1e-13 * scale_w
    for fit_mean in (True, False):
        p = co.gls_power_f64(t, y, dy, f, fit_mean=fit_mean)
        want = co.gls_power_exact(t, y, dy, f, fit_mean=fit_mean)
        ok = np.abs(want) > 1e-13 * np.abs(want).max()
        assert np.max(np.abs(p[ok] - want[ok]) / np.abs(want[ok])) <= 1e-10
        assert np.argmax(p) == np.argmax(want)
    np.testing.assert_allclose(co.gls_power_f64(t, y, dy, f), g["power_exact"], rtol=1e-8)


def test_double_precision_direct_sums_at_large_phases():
    """Julian-date stamps and frequencies to 50 cycles per unit: phases of 1e8 cycles, where the reduction (not the
    polynomial) decides the accuracy.  Also every quadrant boundary and an odd sample count (SIMD remainder)."""
    rng = np.random.default_rng(11)
    n = 1031
    t = np.sort(rng.uniform(0, 90.0, n)) + 2454900.5
    h = rng.standard_normal(n)
    f = np.concatenate([rng.uniform(0.001, 50.0, 300), [0.0, 0.125, 0.25, 0.5, 1.0]])
    Sh, Ch, S, C, S2, C2 = co.gls_sums_f64(t, h, np.abs(h), f)
    Se, Ce = co.trig_sums_exact(t, h, f)
    # the long-double reference itself carries 2 pi f t rounded to 64 bits: |phase| 8e8 rad x 5.4e-20 = 4e-11
    tol = 1e-10 * np.abs(h).sum()
    assert np.max(np.abs(Sh - Se)) <= tol and np.max(np.abs(Ch - Ce)) <= tol
    S2e, C2e = co.trig_sums_exact(t, np.abs(h), 2 * f)
    assert np.max(np.abs(S2 - S2e)) <= 2 * tol and np.max(np.abs(C2 - C2e)) <= 2 * tol
    # exact multiples of an eighth of a cycle at f = 1: the quadrant logic, against the known values 0, +-sqrt(1/2), +-1
    known = {0: 0.0, 1: np.sqrt(0.5), 2: 1.0, 3: np.sqrt(0.5), 4: 0.0, 5: -np.sqrt(0.5), 6: -1.0, 7: -np.sqrt(0.5)}
    for k in range(-8, 9):
        s, c, *_ = co.gls_sums_f64(np.array([k / 8.0]), np.ones(1), np.ones(1), np.array([1.0]))
        assert abs(s[0] - known[k % 8]) <= 1.2e-16 and abs(c[0] - known[(k + 2) % 8]) <= 1.2e-16, k


def test_c_restatements_of_aov_entropy_gregory_loredo_equal_the_numpy_ones():
    rng = np.random.default_rng(3)
    n = 3000
    t = np.sort(rng.uniform(0, 300.0, n)) - 50.0                  # negative stamps included
    x = 1 + np.sin(2 * np.pi * t / 13.7) + 0.2 * rng.standard_normal(n)
    periods = np.linspace(0.5, 40.0, 300)
    for r in (3, 10, 7):
        np.testing.assert_allclose(co.aov_scan(t, x, periods, r), so.aov_scan(t, x, periods, r), rtol=1e-11)
    assert np.all(np.isnan(co.aov_scan(t[:5], x[:5], periods[:3], 10)))     # n <= r: nan, as the numpy form
    mag = so.magnitude_bins(x, 5)
    np.testing.assert_allclose(co.cond_entropy_scan(t, mag, periods, 10, 5),
                               so.cond_entropy_scan(t, mag, periods, 10, 5), rtol=1e-13)
    for m, n_off in ((4, 8), (12, 8), (2, 1), (7, 5)):
        got, want = co.gl_scan(t, periods, m, n_off), so.gl_scan(t, periods, m, n_off)
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-9)
        assert np.argmax(got) == np.argmax(want)
    # a period that puts a phase on a bin edge and phi == 1.0 (t just below a multiple of the period)
    te = np.array([0.0, 0.5, 1.0, 1.5, 2.0 - 2.0 ** -52, 3.0, 3.25, 7.75, 9.0, 9.5, 10.0, 11.0])
    xe = np.arange(te.size, dtype=float) ** 1.5
    pe = np.array([1.0, 2.0, 0.5, 2.5, 3.0])
    np.testing.assert_allclose(co.aov_scan(te, xe, pe, 4), so.aov_scan(te, xe, pe, 4), rtol=1e-12)
    np.testing.assert_allclose(co.gl_scan(te, pe, 2, 2), so.gl_scan(te, pe, 2, 2), rtol=1e-12)


# ---- the C restatement of the Supersmoother oracle (oracle_ss_smooth / oracle_supersmoother_scan) ----------------
def test_c_supersmoother_window_sums_equal_the_literal_updating_formulas():
    """`c_oracle.ss_smooth` on the cases the numpy smoother is pinned on (tests/test_supersmoother_gpu.py: Friedman's
    updating formulas, ties included, `supsmu` built on either; same atol = 1e-12), and against the numpy smoother."""
    from test_supersmoother_gpu import window_sums_equal_the_literal_updating_formulas
    window_sums_equal_the_literal_updating_formulas(co.ss_smooth)
    rng = np.random.default_rng(1)
    for n in (40, 101, 400):
        x = np.sort(rng.uniform(0, 1, n))
        y = np.sin(2 * np.pi * x) + 0.3 * rng.standard_normal(n)
        if n == 101:
            x[10] = x[11]
            x[50:53] = x[50]
        v = (1e-3 * (x[3 * (n // 4) - 1] - x[n // 4 - 1])) ** 2
        for span in so.SS_SPANS:
            for cv in (True, False):
                for got, want in zip(co.ss_smooth(x, y, span, v, cv), so.ss_smooth(x, y, span, v, cv)):
                    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        co.ss_smooth(np.arange(4.0) / 4, np.ones(4), 0.5, 0.0, True)       # 2 ibw + 1 = 5 points do not fit, as in numpy


def test_c_supersmoother_window_sums_stay_exact_for_phases_crowded_into_a_sliver_of_the_cycle():
    """`c_oracle.ss_smooth` against the brute-force locally centred long-double fit (spreads 1e-5, 1e-7; atol = 1e-13)."""
    from test_supersmoother_gpu import window_sums_stay_exact_for_phases_crowded_into_a_sliver_of_the_cycle
    window_sums_stay_exact_for_phases_crowded_into_a_sliver_of_the_cycle(co.ss_smooth)


def ss_restatement_cases():
    """(label, t, y, periods, alphas): sizes either side of the device's dispatch limits; uneven sampling, even sampling
    at commensurate periods (long tied runs), duplicated stamps, a Julian-date offset; periods from a tenth of the
    cadence to 3000 baselines."""
    rng = np.random.default_rng(17)
    for n in (5, 6, 40, 63, 64, 300, 4097, 20_000):
        alphas = (0.0, 0.1, 5.0, 10.0) if n < 20_000 else (0.0, 5.0)
        for variant in ("uneven", "even", "duplicates", "julian"):
            if n == 20_000 and variant in ("duplicates", "julian"):
                continue                                    # (0.15 s a period in numpy: the two variants with the long runs)
            t = np.arange(float(n)) * 0.1 if variant == "even" else np.sort(rng.uniform(0, 0.1 * n, n))
            if variant == "duplicates" and n > 20:
                t[5:n:7] = t[4:n - 1:7]
                t[-n // 10:] = t[-n // 10]
            if variant == "julian":
                t = t + 2454953.5
            y = np.sin(2 * np.pi * t / 7.3) + 0.3 * np.cos(4 * np.pi * t / 7.3) + 0.2 * rng.standard_normal(n)
            base = t[-1] - t[0]
            periods = [0.01, 0.037, 0.61, 7.3, 0.31 * base, 0.999 * base, 1.001 * base, 57.0 * base, 3000.0 * base]
            if variant == "even":
                periods += [0.1, 0.15, 0.25, 0.3, 0.7, 1.0, 5.0, 2.0 / 15.0]
            if variant == "julian":
                periods += [2454953.5, 2454953.5 / 2]
            if n == 20_000:
                periods = periods[::2]
            yield f"n={n} {variant}", t, y, np.array(periods), alphas


def test_c_supersmoother_scan_equals_the_numpy_oracle():
    """`c_oracle.supersmoother_scan` does the numpy oracle's operations in the same 80-bit type and sums ties and the
    final mean in numpy's pairwise order, so the two differ only where numpy's vectorised `power` and libm's `pow`
    round the bass control differently.  Measured over these cases: 1 306 of 1 316 periods bit-identical, largest
    relative difference 2.13e-16 (n = 40, duplicated stamps, alpha = 5).  Gate: ten times that, 2.2e-15 - far under the
    1e-12 at which the C oracle may stand in for the numpy one (the device is held to 1e-9)."""
    gate = 2.2e-15
    assert gate <= 1e-12
    worst, where, count, same = 0.0, None, 0, 0
    for label, t, y, periods, alphas in ss_restatement_cases():
        for alpha in alphas:
            want = so.supersmoother_scan(t, y, periods, alpha)
            got = co.supersmoother_scan(t, y, periods, alpha)
            assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)), (label, alpha)
            rel = np.abs(got - want) / np.abs(want)
            count += rel.size
            same += int((got == want).sum())
            if rel.max() > worst:
                worst, where = float(rel.max()), (label, alpha, float(periods[rel.argmax()]))
    print(f"C vs numpy Supersmoother oracle: {count} periods, {same} bit-identical, largest relative difference {worst:.2e} at {where}")
    assert worst <= gate, (worst, where)
    assert np.all(np.isnan(co.supersmoother_scan(np.arange(4.0), np.ones(4), [1.0, 2.0])))     # below five samples: no fit
