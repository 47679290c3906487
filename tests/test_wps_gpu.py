"""WPS on the GPU (csrc/wps.hip through the class and the C ABI) against the test-local long-double oracle
(tests/wps_oracle.py: the literal convolve / diff / cut recipe in np.clongdouble from the shared float64 table).
PARITY UNPINNED BY THE REFERENCE.

Gate: per cell and per part (real and imaginary separately, so the minus sign and the conjugate are pinned) the rounding
budget of the kernel's tap sum as written, bound_c = (taps + C0) 2^-53 sqrt(s) sum_k |h[k] - h[k-1]| |x[...]| (one fma per
tap; C0 = 4: the weight's difference, sqrt(s), their product, one spare), computed by the oracle in long double; the
spectrum to (2 |c| bound_c + bound_c^2) / s plus four ulp for the epilogue's square, sum and quotient.  No cell is left
out.  Measured on one MI355X (profiles/r31_wps_parity.txt): at most 0.23 of the gate, at the scale of three taps where
C0 is most of the budget; 1e-3 to 3e-3 at the scales of 1025 taps.
Everything that should be the same computation is compared bit for bit."""
import functools

import numpy as np
import pytest

import wps_oracle as wo
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TFSeries, TSeries
from periodicity_amd.timefrequency import WPS, cmor_table

pytestmark = pytest.mark.gpu

DT = 0.02
SCALES = np.array(wo.SCALES)
MARGINALS = ("gwps", "sav", "masked_gwps", "masked_sav", "gwps_count", "sav_count")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def scan(t, x, scales, **kw):
    table, step, span = cmor_table()
    scales = np.asarray(scales, dtype=float)
    return _cabi.wps_scan(x, t, scales * DT, scales, table, step, span, np.exp2(0.5), **kw)


def centred(n):
    t, y = wo.curve(n)
    return t, y - np.mean(y)


@functools.lru_cache(maxsize=None)
def exact(n):
    """The oracle's coefficients and spectrum at the eight scales with their gates, once per size."""
    _, x = centred(n)
    coefs, spectrum = wo.spectrum(x, wo.SCALES)
    bound_c, bound_s = wo.gates(x, wo.SCALES, coefs)
    return coefs, spectrum, bound_c, bound_s


def assert_meets_oracle(label, out, n):
    coefs, spectrum, bound_c, bound_s = exact(n)
    got = out["coefs"]
    assert got.shape == coefs.shape and out["spectrum"].shape == spectrum.shape
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(out["spectrum"]))
    worst = {"re": np.max(np.abs(got.real - coefs.real) / bound_c, axis=1),
             "im": np.max(np.abs(got.imag - coefs.imag) / bound_c, axis=1),
             "spectrum": np.max(np.abs(out["spectrum"] - spectrum) / bound_s, axis=1)}
    for name, ratio in worst.items():
        print(f"{label} {name}: error / gate per scale = " + " ".join(f"{float(r):.3e}" for r in ratio))
    for name, ratio in worst.items():
        assert np.all(ratio <= 1.0), (label, name, [float(r) for r in ratio])


@pytest.mark.parametrize("n", [50, 257, 1000])
def test_parity_filters_shorter_and_longer_than_the_curve(n):
    t, x = centred(n)
    out = scan(t, x, SCALES, want_coefs=True)
    assert_meets_oracle(f"N={n}", out, n)


@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_parity_across_the_tile_seam(extra):
    tile = _cabi.wps_tile()
    n = 2 * tile + 1 if extra is None else tile + extra
    t, x = centred(n)
    out = scan(t, x, SCALES, want_coefs=True)
    assert_meets_oracle(f"N={n}", out, n)
    tiles, chunks, per_chunk, dense, sparse = _cabi.wps_last_dispatch()
    assert tiles == -(-n // tile) and chunks == 1 and per_chunk >= SCALES.size
    # both sides of the 1025-tap boundary: 63.9375 is the last scale whose every filter position is a tap
    lengths = np.array([wo.filter_indices(s).size for s in wo.SCALES])
    assert dense == np.sum(lengths + 1 <= wo.POINTS + 1) == 5 and sparse == 3
    assert lengths[4] + 1 == wo.POINTS + 1 and lengths[5] + 1 > wo.POINTS + 1 and lengths[7] > n


def test_the_sign_and_the_conjugate_are_pinned():
    """A gate that passed a flipped sign or a conjugated filter would pass anything: the parts are far from symmetric."""
    coefs, _, bound_c, _ = exact(257)
    assert np.max(np.abs(2 * coefs.real) / bound_c) > 1e6 and np.max(np.abs(2 * coefs.imag) / bound_c) > 1e6


def test_identical_bytes():
    n = _cabi.wps_tile() + 77
    t, x = centred(n)
    scales = np.concatenate([SCALES, np.geomspace(0.3, 40, 11)])   # 19 scales: three chunks
    full = scan(t, x, scales, want_coefs=True)
    assert _cabi.wps_last_dispatch()[1:3] == (3, 8)
    again = scan(t, x, scales, want_coefs=True)
    for name in ("spectrum", "coefs") + MARGINALS:
        assert same(full[name], again[name]), name
    bare = scan(t, x, scales, want_planes=False)
    assert bare["spectrum"] is None and bare["coefs"] is None
    for name in MARGINALS:
        assert same(full[name], bare[name]), name
    for i in (0, 4, 7, 12):   # one scale alone: its row, its coefficients, its row marginals
        alone = scan(t, x, scales[i:i + 1], want_coefs=True)
        assert same(alone["spectrum"][0], full["spectrum"][i]) and same(alone["coefs"][0], full["coefs"][i]), i
        for name in ("gwps", "masked_gwps", "gwps_count"):
            assert same(alone[name][0], full[name][i]), (name, i)


def test_marginals_follow_numpy_on_the_returned_plane():
    n = _cabi.wps_tile() + 77
    t, x = centred(n)
    scales = np.concatenate([SCALES, np.geomspace(0.3, 40, 11)])
    out = scan(t, x, scales)
    plane = out["spectrum"]
    mask = wo.mask_coi(t, scales * DT)
    assert mask.any() and not mask.all()
    gwps, sav, masked_gwps, masked_sav, gwps_count, sav_count = wo.marginals(plane, mask)
    assert np.array_equal(out["gwps_count"], gwps_count) and np.array_equal(out["sav_count"], sav_count)
    assert (gwps_count == 0).any() and (sav_count == 0).any() and (gwps_count > 0).any() and (sav_count > 0).any()
    assert np.array_equal(np.isnan(out["masked_gwps"]), gwps_count == 0)
    assert np.array_equal(np.isnan(out["masked_sav"]), sav_count == 0)
    wide = plane.astype(np.longdouble)
    inside = np.where(mask, wide, 0)
    u = np.longdouble(wo.U)
    cases = (("gwps", gwps, wide.sum(axis=1), np.full(scales.size, n)), ("sav", sav, wide.sum(axis=0), np.full(n, scales.size)),
             ("masked_gwps", masked_gwps, inside.sum(axis=1), gwps_count), ("masked_sav", masked_sav, inside.sum(axis=0), sav_count))
    for name, numpy_mean, total, terms in cases:
        keep = terms > 0
        # the gate: (terms + 2) 2^-53 sum |terms| around numpy's nanmean (the cells are not negative)
        gate = (terms[keep] + 2) * u * total[keep]
        by_numpy = float(np.max(np.abs(out[name][keep] - numpy_mean[keep]) / gate))
        # and what a sum of `terms` roundings and one quotient can cost a MEAN: the same over the number of terms
        exact_mean = total[keep] / terms[keep]
        worst = float(np.max(np.abs(out[name][keep] - exact_mean) / (gate / terms[keep])))
        print(f"{name}: error / gate = {by_numpy:.3e} against numpy's nanmean, {worst:.3e} of the gate over the number "
              "of terms against the long-double mean")
        assert by_numpy <= 1.0 and worst <= 1.0, name


def test_the_class_on_the_device():
    t = DT * np.arange(2000)
    periods = np.linspace(0.5, 5, 46)
    wps = WPS(periods)
    spectrum = wps(TSeries(t, np.sin(2 * np.pi * t / 2)), want_coefs=True)
    assert isinstance(spectrum, TFSeries) and spectrum.shape == (46, 2000) and wps.coefs.shape == (46, 2000)
    gwps = wps.gwps()
    assert isinstance(gwps, FSeries) and gwps.pmax() == pytest.approx(2.0, abs=1e-12)
    assert same(np.isnan(wps.masked_spectrum.values), ~wps.mask_coi)
    assert np.array_equal(wps.gwps_count, wps.mask_coi.sum(axis=1))
    assert np.allclose(np.abs(wps.coefs) ** 2, wps.power.values, rtol=1e-12, atol=0)
    ranged = wps.gwps(tmin=t[0], tmax=t[-1])   # numpy on the plane: the device's marginal to rounding
    assert np.allclose(ranged.values, gwps.values, rtol=1e-12, atol=0)
    bare = WPS(periods)
    assert bare(TSeries(t, np.sin(2 * np.pi * t / 2)), want_planes=False) is None
    assert same(bare.gwps().values, gwps.values) and same(bare.masked_sav().values, wps.masked_sav().values)
    with pytest.raises(ValueError):
        bare.sav(pmin=1.0)


def test_workspace_without_planes_stays_below_one_plane(monkeypatch):
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    assert 0 < _cabi.wps_work_bytes(65536, 512) < 65536 * 512 * 8


def test_a_budget_that_binds_changes_the_chunks_not_the_rows(monkeypatch):
    n = 300
    t, x = centred(n)
    scales = np.geomspace(0.3, 40, 19)
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    free = scan(t, x, scales)
    assert _cabi.wps_last_dispatch()[1:3] == (3, 8)
    fixed = _cabi.wps_work_bytes(n, scales.size) - 3 * 2 * n * 8
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", repr((fixed + 2 * 2 * n * 8 + 512) / 2 ** 30))   # room for two chunks
    tight = scan(t, x, scales)
    assert _cabi.wps_last_dispatch()[1:3] == (2, 16)
    for name in ("spectrum", "gwps", "masked_gwps", "gwps_count", "sav_count"):
        assert same(free[name], tight[name]), name
    assert np.allclose(free["sav"], tight["sav"], rtol=1e-14, atol=0)
