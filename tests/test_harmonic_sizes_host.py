"""The oracles behind tests/test_harmonic_sizes_gpu.py, without a GPU: the float64 evaluation the device is compared with
against its own 80-bit evaluation at 1025 samples and at about 1e6 cycles over the baseline, the shapes against the
constants of the kernels they are chosen for, and - for EVERY shape the GPU tests run - how many bins the comparison
leaves out (tests/harmonic_sizes.py holds the inputs, the grids and the rules).  PARITY UNPINNED BY THE REFERENCE.

Bounds.  At 1025 samples the float64 oracle is its 80-bit evaluation to the bounds tests/test_mhgls_host.py,
tests/test_mbgls_host.py and tests/test_htest_host.py use: 1e-11 absolute on the kept bins of a GLS power,
1e-11 Z2 + 1e-12 on Z2_m.  At 1e6 cycles those do not hold - the argument of cos(k theta) is 2 pi 1e6 k, rounded to
about 1e-9 k rad in float64: measured 1.3e-10 absolute on the powers, 330 times the bound on Z2_20 - so there the oracle
is held to 1 / 100 of the value gate of the device comparison instead (measured: 2.1e-3 of the gate for the powers,
3.3e-3 for Z2_m)."""
import numpy as np
import pytest

import harmonic_sizes as hs
import htest_oracle as ho
import mbgls_oracle as mb
import mhgls_oracle as mo


# ---- float64 against 80 bits ------------------------------------------------------------------------------------------
def gls_pair(oracle, eq64, eq80, columns):
    """(float64 power, 80-bit power, kept bins) of the leading ``columns``."""
    p64, keep = hs.gls_oracle(oracle, eq64, columns)
    p80 = oracle.power_from(eq80[0][:, :columns, :columns], eq80[1][:, :columns], eq80[2], eq80[3])
    return p64, p80, keep


GLS_PINS = {
    "mhgls": (mo, lambda key, dtype: hs.mh_equations(key, True, True, False, dtype), {1025: 1025, "long": "long"}, (3, 9)),
    "mbgls": (mb, lambda key, dtype: hs.mb_equations(key, 3, False, dtype), {1025: "random-1025-3", "long": "long"}, (5, 9)),
}


@pytest.mark.parametrize("family", list(GLS_PINS))
def test_float64_and_longdouble_powers_agree_at_1025_samples(family):
    oracle, equations, keys, columns = GLS_PINS[family]
    for d in columns:   # one and all harmonics
        p64, p80, keep = gls_pair(oracle, equations(keys[1025], np.float64), equations(keys[1025], np.longdouble), d)
        err = float(np.max(np.abs(p64[keep] - p80[keep])))
        print(f"{family} N=1025 columns={d}: max |p64 - p80| {err:.3e}")
        assert err <= 1e-11
        assert np.all((p80[keep] >= 0) & (p80[keep] <= 1 + 1e-12))   # a share of the weighted variance


@pytest.mark.parametrize("family", list(GLS_PINS))
def test_float64_and_longdouble_powers_agree_at_1e6_cycles(family):
    oracle, equations, keys, columns = GLS_PINS[family]
    for d in columns:
        p64, p80, keep = gls_pair(oracle, equations(keys["long"], np.float64), equations(keys["long"], np.longdouble), d)
        assert keep.all()
        err = np.abs(p64 - p80).astype(np.float64)
        share = float(np.max(err / hs.gls_gate(p64)))
        print(f"{family} 1e6 cycles columns={d}: max |p64 - p80| {err.max():.3e}, {share:.3e} of the gate")
        assert share <= 0.01
        assert np.all((p80 >= 0) & (p80 <= 1 + 1e-12))


def test_float64_and_longdouble_z2_agree_at_1025_events():
    """On the 128 picked bins: the 80-bit evaluation of 20 harmonics costs 8 s on all 1025."""
    z64, z80 = hs.ht_exact(1025, True, True), hs.ht_exact(1025, True, True, np.longdouble)
    err = np.abs(z64 - z80)
    print(f"htest N=1025: max err / (1e-11 Z2 + 1e-12) = {float(np.max(err / (1e-11 * z80 + 1e-12))):.3e}")
    assert np.all(err <= 1e-11 * z80 + 1e-12)
    assert np.all(np.diff(z80, axis=0) >= 0)          # cumulative in m


@pytest.mark.parametrize("drift", [None, 0.0, 2.0, -4.5])
def test_float64_and_longdouble_z2_agree_at_1e6_cycles(drift):
    """``drift`` None: the frequency axis alone; else one row of the plane, the drift in cycles at the ends of the list."""
    if drift is None:
        z64, z80 = hs.ht_exact("long"), hs.ht_exact("long", True, False, np.longdouble)
    else:
        z64, z80 = hs.fd_row("long", drift), hs.fd_row("long", drift, np.longdouble)
    share = float(np.max(np.abs(z64 - z80).astype(np.float64) / ho.gate(z64)))
    print(f"htest 1e6 cycles drift={drift}: {share:.3e} of the gate")
    assert share <= 0.01
    assert np.all(np.diff(z80, axis=0) >= 0)


# ---- the inputs are what the GPU tests need them to be ------------------------------------------------------------------
def test_the_draws_of_the_existing_sizes_have_not_moved():
    """The generators took a seed parameter and a long-baseline sibling: the curves and lists of the sizes the other test
    files use are the draws they always were."""
    rng = np.random.default_rng(5)
    t = np.sort(rng.uniform(0, 3.0 * 65, 65))
    err = rng.uniform(0.1, 0.3, 65)
    y = 1 + 0.7 * np.sin(2 * np.pi * t / 6.3) + 0.3 * np.sin(4 * np.pi * t / 6.3 + 1) + err * rng.standard_normal(65)
    rng = np.random.default_rng(105)
    band = rng.integers(0, 3, 65)
    band[:3] = np.arange(3)
    rng.shuffle(band)
    got = mb.curve(65, 3)
    assert all(np.array_equal(a, b) for a, b in zip(got, (t, y + 0.5 * band, err, band)))
    assert all(np.array_equal(a, b) for a, b in zip(mo.curve(65, 5), (t, y, err)))
    assert all(np.array_equal(a, b) for a, b in zip(mb.curve(65, 3, seed=5), got))
    rng = np.random.default_rng(4)
    n_p = int(round(0.35 * 65))
    cycles = rng.integers(0, int(195.0 / 7.3), n_p)
    t_p = (cycles + (0.3 + 0.06 * rng.standard_normal(n_p)) % 1) * 7.3
    t_u = rng.uniform(0, 195.0, 65 - n_p)
    want = np.sort(np.concatenate([t_p, t_u])) + 1234.5, rng.uniform(0.2, 1, 65)
    assert all(np.array_equal(a, b) for a, b in zip(ho.events(65, ho.SEEDS[65]), want))


def test_the_long_baselines_span_a_million_cycles():
    t, y, err = hs.mh_curve("long")
    assert t.size == 300 and t[0] >= 2454900.5 and 2900 < t[-1] - t[0] < 3000
    f0, delta, nf = hs.mh_grid("long")
    assert 0.9e6 < f0 * (t[-1] - t[0]) < 1.1e6 and nf == hs.NF and f0 < 1 / mo.LONG_PERIOD < f0 + (nf - 1) * delta
    tb = hs.mb_inputs("long")
    assert np.array_equal(tb[0], t) and tb[4] == 3 and hs.mb_grid("long") == (f0, delta, nf)
    t, w = hs.ht_events("long")
    assert t.size == 300 and t[0] >= 5.0e8 and 0.97e5 < t[-1] - t[0] < 1.0e5
    f0, delta, nf = hs.ht_grid("long")
    assert 0.9e6 < f0 * (t[-1] - t[0]) < 1.1e6 and nf == hs.NF and f0 < ho.LONG_FREQUENCY < f0 + (nf - 1) * delta


def test_the_label_layouts_sit_where_the_segment_walk_is_exercised():
    """mbgls.hip: 16 waves, a segment of roundup64(ceil(n / 16)) samples each, walked 256 at a time."""
    seg = lambda n: (-(-n // 16) + 63) // 64 * 64
    assert [seg(n) for n in hs.SEGMENTS] == [64, 128, 256, 320, 576]
    assert sum(seg(n) % 256 != 0 for n in hs.SEGMENTS) >= 3                  # a last trip with dead 64-sample groups
    band = hs.mb_inputs("runs-4097")[3]
    owner = np.arange(4097) // seg(4097)
    assert set(owner[band == 1]) == {1} and len(set(owner[band == 2])) == 2 and set(owner[band == 0]) == set(range(13))
    band = hs.mb_inputs("single-4097")[3]
    assert np.flatnonzero(band == 2).tolist() == [4096] and 4096 == 12 * seg(4097) + 256   # alone in its wave's second trip
    band = hs.mb_inputs("single-1025")[3]
    assert np.flatnonzero(band == 2).tolist() == [1024] and 1024 == 8 * seg(1025)          # alone in the ninth segment
    assert np.array_equal(hs.mb_inputs("interleaved-4097")[3], np.arange(4097) % 3)
    for n, B, _ in hs.MANY:
        assert np.array_equal(np.unique(hs.mb_inputs(f"many-{n}-{B}")[3]), np.arange(32))
    for n in hs.GAPS:
        assert np.array_equal(np.unique(hs.mb_inputs(f"gap-{n}")[3]), [0, 1])


# ---- left-out bins of every shape the GPU tests run (gls_oracle and assert_htest refuse more than 5 % / 1 %) -------------
def report(label, exact, keep, nf):
    peak = int(np.argmax(np.where(keep, exact, -np.inf)))
    print(f"{label}: {int((~keep).sum())} of {keep.size} bins left out, highest bin {peak} ({exact[peak]:.4f})")
    assert exact.size == nf and abs(peak - nf // 2) <= 2        # the signal is inside the grid: its peak is the centre


@pytest.mark.parametrize("n", hs.TRIPS + ("long",))
def test_left_out_bins_mhgls(n):
    for nterms in (1, 4):
        for fit_mean in (True, False):
            for with_err in (True, False):
                if n == "long" and not (fit_mean and with_err):
                    continue
                exact, keep = hs.mh_oracle(n, nterms, with_err, fit_mean)
                report(f"mhgls N={n} nterms={nterms} fit_mean={int(fit_mean)} err={int(with_err)}", exact, keep, hs.NF)


MB_SHAPES = ([(f"random-{n}-{B}", 3) for n in hs.SEGMENTS for B in (3, 4)] + [(name, 3) for name in hs.LAYOUTS]
             + [(f"many-{n}-{B}", h) for n, B, h in hs.MANY] + [(f"gap-{n}", 3) for n in hs.GAPS] + [("long", 3)])


@pytest.mark.parametrize("name,top", MB_SHAPES, ids=[s[0] for s in MB_SHAPES])
def test_left_out_bins_mbgls(name, top):
    for nterms in range(1, top + 1):
        exact, keep = hs.mb_oracle(name, nterms, top)
        report(f"mbgls {name} nterms={nterms}", exact, keep, hs.mb_grid(name)[2])


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", hs.TRIPS + ("long",))
def test_left_out_bins_htest(n, weighted):
    if n == "long" and not weighted:
        return
    for nharm in (2, 20):
        Z = hs.ht_exact(n, weighted)[:nharm]
        hs.assert_htest(f"htest N={n} nharm={nharm} weights={int(weighted)}", Z)
        h = ho.h_and_m(Z)[0]
        print(f"htest N={n} nharm={nharm} weights={int(weighted)}: {int((~ho.decided(Z)).sum())} of {h.size} bins left out")
        assert abs(int(np.argmax(h)) - hs.NF // 2) <= 2


@pytest.mark.parametrize("n,drift", [(1025, 0.0), (1025, 2.0), (4097, 0.0), (4097, 2.0), ("long", 0.0), ("long", 2.0), ("long", -4.5)])
def test_left_out_bins_htest_fdot(n, drift):
    for nharm in (2, 20):
        hs.assert_htest(f"fdot N={n} drift={drift} nharm={nharm}", hs.fd_row(n, drift)[:nharm])


def test_left_out_bins_on_the_wide_grid():
    """9217 bins from half a step up: only the lowest few, where the harmonics are constant over the baseline, go."""
    assert hs.WIDE > 8 * 1024 and hs.wide_grid(hs.mh_curve(65)[0])[2] == hs.WIDE
    for nterms in (1, 4):
        exact, keep = hs.gls_oracle(mo, hs.mh_wide_equations(), 2 * nterms + 1)
        print(f"mhgls wide nterms={nterms}: {int((~keep).sum())} of {keep.size} bins left out")
    for nterms in (1, 3):
        exact, keep = hs.gls_oracle(mb, hs.mb_wide_equations(), mb.columns(3, nterms, True))
        print(f"mbgls wide nterms={nterms}: {int((~keep).sum())} of {keep.size} bins left out")


def test_left_out_bins_at_20000_samples():
    assert hs.PICK.size == 128
    exact, keep = hs.mh_oracle(hs.BIG, 4, picked=True)
    print(f"mhgls N={hs.BIG}: {int((~keep).sum())} of 128 picked bins left out, peak {exact.max():.4f}")
    exact, keep = hs.mb_oracle("big", 3, picked=True)
    print(f"mbgls N={hs.BIG}: {int((~keep).sum())} of 128 picked bins left out, peak {exact.max():.4f}")
    hs.assert_htest(f"htest N={hs.BIG}", hs.ht_exact(hs.BIG, True, True))
