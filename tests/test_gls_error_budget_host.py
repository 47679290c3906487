"""What the GLS error-budget gate (tests/gls_error_budget.py, tests/test_gls_error_budget_gpu.py) rests on, checked
without a device:

* ``oracle_gls_sums_reduced`` is pinned by integer arithmetic: on lattice inputs the fractional phase is
  ``(F T' mod 2^38) / 2^38`` in integers, and numpy long-double sin / cos of that, summed, must agree with the C oracle to
  ``4 2^-64 sum |h|`` at 4e3 and at 4e6 cycles (no fma anywhere in the pin); at <= 4e3 cycles it also agrees with
  ``oracle_trig_sums_exact`` to ``1e-16 sum |h|``;
* the lattice properties: the grid and ``t - t[0]`` are exact, and on the high slabs ``f t'`` needs more than 53 bits for
  most pairs (``lo != 0`` in ``frac_product``);
* for every case of the GPU test, on the oracle alone: at most 1 % of the picked bins carry ``bound_p > 1e-10``;
* the restated epilogue equals ``scan_oracle.gls_epilogue``, and the constants are what DESIGN.md 4.1m derives.
"""
from fractions import Fraction

import numpy as np
import pytest

import gls_error_budget as eb
from oracle import c_oracle as co
from oracle import scan_oracle as so

LD_EPS = np.longdouble(2.0) ** -64


def integer_pin(t, T, h, F):
    """Sums of h sin / cos (2 pi frac) with frac from integers: numpy long double, no fma."""
    Tp = T - T[0]
    out = np.empty((F.size, 2), dtype=np.longdouble)
    hl = np.asarray(h, dtype=np.longdouble)
    for j, f in enumerate(F):
        ang = so.TWO_PI_L * eb.exact_fraction(np.full(Tp.size, f, dtype=np.int64), Tp)
        out[j] = np.dot(hl, np.sin(ang)), np.dot(hl, np.cos(ang))
    return out


@pytest.mark.parametrize("cycles", [4e3, 4e6])
def test_reduced_oracle_is_pinned_by_integer_arithmetic(cycles):
    n, span = 1500, 4000
    t, y, dy, T = eb.lattice_curve(n, 3, 37.3, span)
    F0, D = eb.lattice_step(span)
    freq, F = eb.lattice_grid(F0, D, 96, eb.high_j_begin(D, span, cycles))
    assert 0.9 * cycles < freq[0] * (t[-1] - t[0]) < 1.1 * cycles
    w, yc, YY, err = eb.prologue_ld(y, dy, True)
    hy = w * yc
    got = co.gls_sums_reduced(t, hy, w, freq)
    pin_y, pin_w = integer_pin(t, T, hy, F), integer_pin(t, T, w, F)
    pin_2 = integer_pin(t, T, w, 2 * F)
    A_y, A_w = np.abs(hy).sum(), np.abs(w).sum()
    worst = max(np.abs(got[:, 0:2] - pin_y).max() / A_y, np.abs(got[:, 2:4] - pin_w).max() / A_w,
                np.abs(got[:, 4:6] - pin_2).max() / A_w)
    print(f"BUDGET-ORACLE {cycles:.0e} cycles: worst |reduced - integer pin| / sum|h| = {float(worst / LD_EPS):.2f} x 2^-64")
    assert worst <= 4 * LD_EPS
    if cycles <= 4e3:
        S, C = co.trig_sums_exact(t - t[0], np.asarray(hy, dtype=float), freq)
        h64 = np.asarray(hy, dtype=float).astype(np.longdouble)      # (the older oracle takes double weights)
        ref = co.gls_sums_reduced(t, h64, h64, freq)
        assert max(np.abs(ref[:, 0] - S).max(), np.abs(ref[:, 1] - C).max()) <= 1e-16 * float(np.abs(h64).sum())


def every_curve():
    for group, g in eb.GROUPS.items():
        for case in g["cases"]:
            yield group, case


def test_lattice_inputs_are_exact_and_fill_the_product():
    """Grid values and t - t[0] exact (checked in rational arithmetic); on every high slab more than half of the
    (f, t') products need more than 53 bits."""
    seen_high = 0
    for group, case in every_curve():
        arrays = eb.case_arrays(group, case)
        for label, t, y, dy, F0, D, j_begin, nf, row, off in eb.case_curves(group, case, arrays)[:1]:
            n = t.size
            T = arrays["T"][:n]
            assert T.max() < 2 ** 28 and np.all(np.diff(T) >= 0)
            tp = t - t[0]
            for i in (0, 1, n // 2, n - 1):
                assert Fraction(float(t[i])) == Fraction(eb.JD) + Fraction(int(T[i]), 2 ** eb.TBITS)
                assert Fraction(float(tp[i])) == Fraction(int(T[i] - T[0]), 2 ** eb.TBITS)
            freq, F = eb.lattice_grid(F0, D, nf, j_begin)
            f0, delta = F0 / 2.0 ** eb.FBITS, D / 2.0 ** eb.FBITS
            device_rule = f0 + (j_begin + np.arange(nf)) * delta           # one product, one sum, two roundings
            assert np.array_equal(device_rule, freq)
            for j in (0, nf // 2, nf - 1):
                assert Fraction(float(freq[j])) == Fraction(int(F[j]), 2 ** eb.FBITS)
            if int(F[0]) * 2.0 ** -eb.FBITS * (t[-1] - t[0]) > 1e6:
                prod = F[:64, None].astype(object) * (T - T[0])[None, ::max(1, n // 64)].astype(object)
                bits = np.array([[(int(v) // (int(v) & -int(v))).bit_length() if v else 0 for v in r] for r in prod])
                assert (bits > 53).mean() > 0.5, (group, case["name"], float((bits > 53).mean()))
                seen_high += 1
    assert seen_high >= 20


def test_restated_epilogue_is_the_oracles():
    t, y, dy, T = eb.lattice_curve(300, 5, 37.3, 300)
    freq = eb.lattice_grid(*eb.lattice_step(300), 200)[0]
    for fit_mean in (True, False):
        for psd in (True, False):
            sums, w, yc, YY, err = eb.exact_sums(t, y, dy, freq, fit_mean)
            a = eb.power_of(sums, YY, err, fit_mean, psd)
            b = eb.epilogue_ld(sums[:, 0], sums[:, 1], sums[:, 4], sums[:, 5], sums[:, 2], sums[:, 3], YY, fit_mean, psd, err)[0]
            assert a.dtype == np.longdouble and np.max(np.abs(a - b) / np.abs(a)) <= 8 * float(LD_EPS)


def test_constants_are_the_derivations():
    """DESIGN.md 4.1m, D3 - D6 and D10 - D11, by hand for the shapes the kernels have."""
    assert (eb.E_SC, eb.E_SC2, eb.RHO, eb.ETA, eb.E_HALF) == (8, 12, 2, 7, 72)
    # K = 16, COLS = 4: lane 68, column 9 + 31 * 10 = 319, seed 389; walk 15 * 8 + 2 * 15 + 7 * 105 = 885
    assert eb.c_trig(16, 4) == 68 + 319 + 2 + 120 + 30 + 735 == 1274
    assert eb.c_trig(4, 1) == 68 + (9 + 7 * 10) + 2 + 24 + 6 + 21
    assert eb.c_trig(16, 2, pair=True) == 68 + (9 + 15 * 10) + 2 + 20 + 8 + 2
    rec = dict(route="general", K=16, S=4, parts=1, wide_prep=0)
    lin, quad, cw, cybar, cyy = eb.route_constants(rec, 1031)
    run = 9 * 32                                      # nine chunks of 128, a quarter of each
    assert cw == 2 + 6 + 16 and (lin, quad) == (eb.c_trig(16, 1) + run + 3 + 7 + cw, 2 * eb.c_trig(16, 1) + 1 + run + 3 + 7 + cw)
    assert eb.route_constants(dict(route="shared"), 257)[0] == 72 + 260 + 7 + (1 + 6 + 16)
    assert eb.route_constants(dict(route="parts", K=8, S=2, parts=9, z_len=2176, wide_prep=1), 18500)[0] == \
        eb.c_trig(8, 2) + 17 * 64 + 1 + (3 + 2) + 7 + eb.c_weight_sum(18500, 1024, wide=True)


@pytest.mark.parametrize("group", list(eb.GROUPS))
def test_the_bound_is_tight_on_nearly_every_bin(group):
    """On the oracle alone: at most 1 % of a case's picked bins have bound_p > 1e-10 (of the normalised power: with psd
    the spectrum and its bound are W YY / 2 times that)."""
    g = eb.GROUPS[group]
    for case in g["cases"]:
        arrays = eb.case_arrays(group, case)
        wide = total = 0
        for curve in eb.case_curves(group, case, arrays):
            consts = eb.route_constants(eb.expected_record(group, case), curve[1].size, pair=g["pair"])
            pick, p, bound, unit = eb.curve_reference(group, case, curve, consts)
            assert pick.size <= 1024 and np.all(np.isfinite(bound.astype(float)))
            wide += int((bound > eb.CAP * unit).sum())
            total += pick.size
            print(f"BUDGET-CAP {group} {case['name']} {curve[0]}: C = {consts[0]} / {consts[1]}, {pick.size} bins, "
                  f"bound median {float(np.median(bound / unit)):.2e} max {float((bound / unit).max()):.2e}, "
                  f"p max {float((p / unit).max()):.3f}")
        assert total <= 1024 and wide <= 0.01 * total, (group, case["name"], wide, total)


@pytest.mark.parametrize("name", list(eb.RAW))
def test_raw_reference_turns_back_to_absolute_time(name):
    """The long-double raw sums over the absolute times (reduced sums over t', turned by f t[0] mod 1 from integers)
    agree with ``oracle_trig_sums_exact`` on the absolute times as far as THAT oracle goes: 2^-64 of a phase of
    f t cycles, a few times over."""
    case = eb.RAW[name]
    t, h, T = eb.raw_inputs(case)
    pick = np.arange(0, case["nf"], 64)
    S, C, A = eb.raw_exact(case, pick)
    freq = eb.lattice_grid(case["F0"], case["D"], case["nf"])[0][pick]
    S0, C0 = co.trig_sums_exact(t, h, freq)
    room = 8 * float(LD_EPS) * 2 * np.pi * freq.max() * t.max() + 4 * eb.U
    assert max(np.abs(S.astype(float) - S0).max(), np.abs(C.astype(float) - C0).max()) <= room * float(A)
