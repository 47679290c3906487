"""Tier F: the device FFT-extirpolation path (GLS(method="fft"), pdc_gls_scan_fft,
pdc_trig_sums_fft) reproduces the UNMODIFIED reference — `power_ref` goldens and the numpy
restatement of spectral.py:11-40 — including its approximation error.

Gate: |d| <= 1e-9 |ref| + 1e-12 max|ref| (the FFT path computes every bin with an absolute error
of a few ulps of the largest one, so tiny bins carry no relative accuracy in the reference
either)."""
import os

import numpy as np
import pytest

from oracle import scan_oracle as so
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.spectral import GLS

pytestmark = pytest.mark.gpu


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def assert_tier_f(got, ref, rtol=1e-9, afloor=1e-12):
    ref = np.asarray(ref)
    ok = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), ok)
    scale = np.max(np.abs(ref[ok]))
    err = np.abs(got[ok] - ref[ok])
    bound = rtol * np.abs(ref[ok]) + afloor * scale
    assert np.all(err <= bound), (np.max(err / bound), int(np.argmax(err / bound)))


def synth(n, seed, t_offset=0.0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, float(n), n)) + t_offset
    dy = rng.uniform(0.05, 0.2, n)
    y = 1.0 + 0.5 * np.sin(2 * np.pi * t / 37.3) + dy * rng.standard_normal(n)
    return t, y, dy


@pytest.mark.parametrize("n", [1000, 5000])
def test_trig_sum_seam_matches_reference_fft(golden_dir, n):
    g = load(golden_dir, f"g4_synth{n}")
    t, y, dy, f = g["t"], g["y"], g["dy"], g["frequency"]
    df, fmin = float(g["df"]), float(g["fmin"])
    w, yc, _ = so.gls_weights(y, dy, True)
    for h, d, f0, sname, cname in ((w * yc, df, fmin, "Sh_fft", "Ch_fft"),
                                   (w, 2 * df, 2 * fmin, "S2_fft", "C2_fft"),
                                   (w, df, fmin, "S_fft", "C_fft")):
        S, C = _cabi.trig_sums_fft(t, h, d, f.size, f0)
        amp = np.max(np.hypot(g[sname], g[cname]))
        assert np.max(np.abs(S - g[sname])) <= 1e-13 * amp * np.sqrt(n)
        assert np.max(np.abs(C - g[cname])) <= 1e-13 * amp * np.sqrt(n)


def test_reference_known_answers_through_the_fft_path(golden_dir):
    g = load(golden_dir, "g2_sine100")
    ls = GLS(method="fft")(TSeries(values=g["values"]))
    assert np.array_equal(ls.frequency, g["frequency"])
    assert ls.period_at_highest_peak == 10.0 and ls.argmax() == 49
    ok = np.abs(g["power_ref"]) > 1e-9        # bins 148/247: exact zero / Nyquist singularity
    assert_tier_f(ls.values[ok], g["power_ref"][ok], afloor=1e-11)
    # the >1 maximum of the reference (extirpolation error made visible) is reproduced
    assert abs(ls.values.max() - g["power_ref"].max()) < 1e-12


@pytest.mark.parametrize("fit_mean", [True, False])
@pytest.mark.parametrize("psd", [False, True])
def test_spotted_star_power_ref(golden_dir, fit_mean, psd):
    g = load(golden_dir, "g3_spotted_star")
    ls = GLS(psd=psd, method="fft")(TSeries(g["t"], g["y"]), err=g["dy"], fit_mean=fit_mean)
    ref = g[f"power_ref_fm{int(fit_mean)}_psd{int(psd)}"]
    assert_tier_f(ls.values, ref)
    assert ls.argmax() == int(np.nanargmax(ref))


def test_spotted_star_without_errors_and_window(golden_dir):
    g = load(golden_dir, "g3_spotted_star")
    ls = GLS(method="fft")(TSeries(g["t"], g["y"]))
    assert_tier_f(ls.values, g["power_ref_noerr"])
    g = load(golden_dir, "g5_window")
    gls = GLS(method="fft")
    gls(TSeries(g["t"], g["y"]), err=g["dy"])
    assert_tier_f(gls.window().values, g["power_ref"], afloor=1e-11)


def test_bootstrap_through_the_fft_path_reproduces_reference_replicates(golden_dir):
    g = load(golden_dir, "g6_bootstrap")
    gls = GLS(method="fft")
    gls(TSeries(g["t"], g["y"]), err=g["dy"])
    reps = gls.bootstrap(20, random_seed=42)
    np.testing.assert_allclose(reps, g["replicates_ref"], rtol=1e-9)
    assert gls.fap(0.3) == float(g["fap_at_0p3_ref"])
    np.testing.assert_allclose(gls.fal(0.1), float(g["fal_at_0p1_ref"]), rtol=1e-9)


@pytest.mark.parametrize("n", [1000, 5000])
def test_synthetic_power_ref(golden_dir, n):
    g = load(golden_dir, f"g4_synth{n}")
    ls = GLS(method="fft")(TSeries(g["t"], g["y"]), err=g["dy"])
    assert_tier_f(ls.values, g["power_ref"])
    # and it differs from the exact sums by the reference's own approximation error
    assert 1e-7 < np.max(np.abs(ls.values - g["power_exact"])) < 1e-3


@pytest.mark.parametrize("kw", [dict(n=1), dict(n=3.3), dict(fmin=0.01, fmax=0.4),
                                dict(fmin=0.2, fmax=0.2004)])
def test_grids_and_time_offsets_vs_numpy_restatement(kw):
    for off in (0.0, 2454953.5, -321.25):
        t, y, dy = synth(700, 3, t_offset=off)
        freq, power = so.gls(t, y, dy, **kw)
        ls = GLS(method="fft", **kw)(TSeries(t, y), err=dy)
        assert np.array_equal(ls.frequency, freq)
        assert_tier_f(ls.values, power, rtol=1e-8, afloor=1e-10)


def test_fft_sizes_cover_every_radix_combination():
    # nfft = 2^k for k = 3 .. 21: every mix of radix-16/8/4/2 passes and both ping-pong parities
    t, y, dy = synth(300, 8)
    w, yc, _ = so.gls_weights(y, dy, True)
    for k in range(3, 22):
        nf = max(1, (1 << k) // 5)
        assert 1 << int(nf * 5 - 1).bit_length() == 1 << k
        df, fmin = 0.37 / (1 << k), 0.11 / (1 << k)
        S, C = _cabi.trig_sums_fft(t, w * yc, df, nf, fmin)
        Sr, Cr = so.trig_sum_fft(t, w * yc, df, nf, fmin)
        amp = np.max(np.hypot(Sr, Cr))
        assert np.max(np.abs(S - Sr)) <= 1e-12 * amp and np.max(np.abs(C - Cr)) <= 1e-12 * amp, k


def test_fft_path_is_bitwise_reproducible_and_order_free_deposits_agree_with_the_atomic_ones():
    """Sorted time stamps on a grid that does not wrap: the extirpolation deposits are added in sample order
    by the threads that own the cells (no atomics) - the same bits on every call, for single curves, batches
    and bootstrap replicates.  Shuffled time stamps (raw C-ABI callers) take the atomic kernels: same
    periodogram to rounding."""
    t, y, dy = synth(20_000, 91)
    nf = 60_000
    df = 1.0 / (t[-1] - t[0]) / 5
    fmin = 0.5 * df
    first = _cabi.gls_scan_fft(t, y, dy, fmin, df, nf)
    for _ in range(3):
        assert np.array_equal(_cabi.gls_scan_fft(t, y, dy, fmin, df, nf), first)
    perm = np.random.default_rng(5).permutation(t.size)
    shuffled = _cabi.gls_scan_fft(t[perm], y[perm], dy[perm], fmin, df, nf)
    assert_tier_f(shuffled, first, 1e-9, 1e-12)
    assert_tier_f(first, so.gls(t, y, dy, fmin=fmin, fmax=fmin + (nf - 1.5) * df)[1], 1e-9, 1e-12)
    # clustered stamps: thousands of samples reach the same cells
    tc = np.sort(np.concatenate([np.full(3000, 17.25), np.linspace(0.0, 40.0, 2000), 17.25 + 1e-9 * np.arange(3000)]))
    yc = np.sin(tc) + 0.1 * np.cos(37 * tc)
    dfc = 1.0 / 40.0 / 5
    pc = _cabi.gls_scan_fft(tc, yc, None, 0.5 * dfc, dfc, 500)
    assert np.array_equal(_cabi.gls_scan_fft(tc, yc, None, 0.5 * dfc, dfc, 500), pc)
    assert_tier_f(pc, so.gls(tc, yc, None, fmin=0.5 * dfc, fmax=0.5 * dfc + 498.5 * dfc)[1], 1e-9, 1e-11)
    S, C = _cabi.trig_sums_fft(t, y, df, nf, fmin)
    S2, C2 = _cabi.trig_sums_fft(t, y, df, nf, fmin)
    assert np.array_equal(S, S2) and np.array_equal(C, C2)
    # batches and bootstrap replicates
    lens = [700, 701, 333]
    offs = np.concatenate([[0], np.cumsum(lens)])
    tb = np.concatenate([np.sort(np.random.default_rng(s).uniform(0, 700.0, n)) for s, n in enumerate(lens)])
    yb = np.sin(tb / 3.0) + 0.2 * np.random.default_rng(9).standard_normal(tb.size)
    b1 = _cabi.gls_scan_fft_batch(tb, yb, None, offs, 0.001, 0.0003, 4000)[0]
    b2 = _cabi.gls_scan_fft_batch(tb, yb, None, offs, 0.001, 0.0003, 4000)[0]
    assert np.array_equal(b1, b2)
    for b in range(3):
        sl = slice(offs[b], offs[b + 1])
        assert_tier_f(b1[b], _cabi.gls_scan_fft(tb[sl], yb[sl], None, 0.001, 0.0003, 4000), 1e-9, 1e-12)   # (other prologue)
    ls = GLS(method="fft")
    ls(TSeries(t[:3000], y[:3000]), err=dy[:3000])
    assert np.array_equal(ls.bootstrap(40, random_seed=7), ls.bootstrap(40, random_seed=7))


def test_full_size_c2_matches_cpu_reference_path():
    n, nf = 100_000, 1_000_000
    t, y, dy = synth(n, 20241010)
    df = 1.0 / (t[-1] - t[0]) / 5
    fmin = 0.5 * df
    got = _cabi.gls_scan_fft(t, y, dy, fmin, df, nf)
    freq = fmin + df * np.arange(nf)
    want = so.gls_power(t, y, dy, freq, df, fmin, sums="fft")
    assert_tier_f(got, want, rtol=1e-8, afloor=1e-11)
    assert int(np.argmax(got)) == int(np.argmax(want))
    direct = _cabi.gls_scan(t, y, dy, fmin, df, nf)
    assert int(np.argmax(direct)) == int(np.argmax(got))      # tier R, the other way round


def test_batched_fft_path_equals_single_calls():
    rng = np.random.default_rng(12)
    lens = [50, 300, 301, 1000, 7]
    curves = [synth(n, 200 + i) for i, n in enumerate(lens)]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    t, y, dy = (np.concatenate([c[i] for c in curves]) for i in range(3))
    nf, df, fmin = 3000, 0.00021, 0.0004
    for fit_mean in (True, False):
        power, amax, argmax = _cabi.gls_scan_fft_batch(t, y, dy, offsets, fmin, df, nf, fit_mean,
                                                       want_peaks=True)
        for b, (tb, yb, dyb) in enumerate(curves):
            single = _cabi.gls_scan_fft(tb, yb, dyb, fmin, df, nf, fit_mean)
            assert_tier_f(power[b], single, rtol=1e-9, afloor=1e-12)   # (global atomics: rounding only)
            assert argmax[b] == np.nanargmax(power[b]) and amax[b] == np.nanmax(power[b])
    # shared time axis (bootstrap shape), equal weights
    tt, yy, _ = curves[3]
    picks = rng.integers(0, 1000, (9, 1000))
    offs = np.arange(10) * 1000
    power, _, _ = _cabi.gls_scan_fft_batch(tt, yy[picks].ravel(), None, offs, fmin, df, nf, shared_t=True)
    for b in range(9):
        assert_tier_f(power[b], _cabi.gls_scan_fft(tt, yy[picks[b]], None, fmin, df, nf), 1e-9, 1e-12)


def _shuffled_inside_curves(offsets, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([offsets[b] + rng.permutation(offsets[b + 1] - offsets[b]) for b in range(offsets.size - 1)])


def test_batch_with_shuffled_stamps_takes_the_atomic_route_and_agrees_with_the_sorted_batch():
    lens = [300, 301, 7]
    curves = [synth(n, 300 + i) for i, n in enumerate(lens)]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    t, y, dy = (np.concatenate([c[i] for c in curves]) for i in range(3))
    perm = _shuffled_inside_curves(offsets, 17)
    nf, df, fmin = 3000, 0.00021, 0.0004
    for fit_mean in (True, False):
        ordered = _cabi.gls_scan_fft_batch(t, y, dy, offsets, fmin, df, nf, fit_mean)[0]
        shuffled = _cabi.gls_scan_fft_batch(t[perm], y[perm], dy[perm], offsets, fmin, df, nf, fit_mean)[0]
        for b in range(len(lens)):
            assert_tier_f(shuffled[b], ordered[b])
    # a shuffled shared axis, three replicates
    tt, yy, _ = curves[0]
    picks = np.random.default_rng(18).integers(0, 300, (3, 300))
    offs = np.arange(4) * 300
    p1 = np.random.default_rng(19).permutation(300)
    for fit_mean in (True, False):
        ordered = _cabi.gls_scan_fft_batch(tt, yy[picks].ravel(), None, offs, fmin, df, nf, fit_mean, shared_t=True)[0]
        shuffled = _cabi.gls_scan_fft_batch(tt[p1], yy[picks][:, p1].ravel(), None, offs, fmin, df, nf, fit_mean,
                                            shared_t=True)[0]
        for b in range(3):
            assert_tier_f(shuffled[b], ordered[b])


def test_raw_sums_with_shuffled_stamps_take_the_atomic_route_and_agree_with_the_sorted_call():
    t, y, dy = synth(300, 8)
    w, yc, _ = so.gls_weights(y, dy, True)
    h = w * yc
    perm = np.random.default_rng(23).permutation(300)
    nf, df, fmin = 3000, 0.00021, 0.0004
    S, C = _cabi.trig_sums_fft(t, h, df, nf, fmin)
    Ss, Cs = _cabi.trig_sums_fft(t[perm], h[perm], df, nf, fmin)
    amp = np.max(np.hypot(S, C))
    assert np.max(np.abs(Ss - S)) <= 1e-12 * amp and np.max(np.abs(Cs - C)) <= 1e-12 * amp


@pytest.mark.parametrize("fit_mean", [True, False])
def test_a_grid_that_wraps_takes_the_atomics_behind_sorted_stamps(fit_mean):
    """df = 1.5 / span: positions pass the end of every grid, `deposit_in_order` is false for all of them."""
    t, y, dy = synth(300, 41)
    nf = 40
    df = 1.5 / (t[-1] - t[0])
    fmin = 0.5 * df
    freq = fmin + df * np.arange(nf)
    want = so.gls_power(t, y, dy, freq, df, fmin, fit_mean, sums="fft")
    assert np.all(np.isfinite(want))
    assert_tier_f(_cabi.gls_scan_fft(t, y, dy, fmin, df, nf, fit_mean), want)
    # batch: the curve, and its first half, whose grid at 2 df wraps and whose grids at df do not
    half = 150
    offsets = np.array([0, 300, 300 + half])
    cat = [np.concatenate([a, a[:half]]) for a in (t, y, dy)]
    power = _cabi.gls_scan_fft_batch(*cat, offsets, fmin, df, nf, fit_mean)[0]
    assert_tier_f(power[0], want)
    assert_tier_f(power[1], so.gls_power(t[:half], y[:half], dy[:half], freq, df, fmin, fit_mean, sums="fft"))
    w, yc, _ = so.gls_weights(y, dy, fit_mean)
    S, C = _cabi.trig_sums_fft(t, w * yc, df, nf, fmin)
    Sr, Cr = so.trig_sum_fft(t, w * yc, df, nf, fmin)
    amp = np.max(np.hypot(Sr, Cr))
    assert np.max(np.abs(S - Sr)) <= 1e-12 * amp and np.max(np.abs(C - Cr)) <= 1e-12 * amp


@pytest.mark.parametrize("nf", [7, 3000])           # below one wave; every wave busy
@pytest.mark.parametrize("fit_mean", [True, False])
def test_row_maxima_where_ties_and_nan_decide(nf, fit_mean):
    """An all-zero curve: every bin NaN without psd (argmax -1, amax NaN), every bin 0.0 with it (the first of
    equal maxima: argmax 0) - as the reference's epilogue gives them."""
    lens = [50, 40, 60]
    curves = [synth(n, 500 + i) for i, n in enumerate(lens)]
    curves[1] = (curves[1][0], np.zeros(lens[1]), curves[1][2])
    offsets = np.concatenate([[0], np.cumsum(lens)])
    t, y, dy = (np.concatenate([c[i] for c in curves]) for i in range(3))
    df, fmin = 0.00021, 0.0004
    freq = fmin + df * np.arange(nf)
    for psd in (False, True):
        zero_row = so.gls_power(*curves[1], freq, df, fmin, fit_mean, psd, sums="fft")
        assert np.all(zero_row == 0.0) if psd else np.all(np.isnan(zero_row))
        power, amax, argmax = _cabi.gls_scan_fft_batch(t, y, dy, offsets, fmin, df, nf, fit_mean, psd, want_peaks=True)
        assert np.array_equal(power[1], zero_row, equal_nan=True)
        if psd:
            assert argmax[1] == 0 and amax[1] == 0.0
        else:
            assert argmax[1] == -1 and np.isnan(amax[1])
        for b in (0, 2):
            assert argmax[b] == np.nanargmax(power[b]) and amax[b] == np.nanmax(power[b])


def test_bootstrap_1000_replicates_through_both_paths_agree_on_the_false_alarm_level():
    t, y, dy = synth(400, 31)
    fft, direct = GLS(method="fft"), GLS()
    fft(TSeries(t, y), err=dy)
    direct(TSeries(t, y), err=dy)
    r_fft = fft.bootstrap(300, random_seed=7)
    r_dir = direct.bootstrap(300, random_seed=7)
    assert np.max(np.abs(r_fft - r_dir)) < 5e-3          # same draws, approximation error only
    assert abs(fft.fal(0.05) - direct.fal(0.05)) < 5e-3
