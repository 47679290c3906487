"""The Keplerian periodogram on the GPU (csrc/kepler.hip through the class and the C ABI) against the test-local
long-double oracle (tests/kepler_oracle.py: exact phase reduction, bracketed Newton to a fixed point, textbook anomaly
formulas, LDL^T in long double; its float64 evaluation sits below 1e-3 of the gate, tests/test_kepler_host.py).
PARITY UNPINNED BY THE REFERENCE.

Gate and keep rule: cells whose oracle cond is at most 1e6 are held to Tier E, |got - exact| <= 1e-6 |exact| + 1e-9;
every other cell must be NaN or finite; at most 5 % of a cube may be left out, which every parity test asserts (on the
inputs here nothing is left out: tests/test_kepler_host.py).  Everything that should be the same computation is compared
bit for bit.  The oracle is given the frequencies the kernel forms, f0 + j delta with delta = freq[1] - freq[0]."""
import functools

import numpy as np
import pytest

import kepler_oracle as ko
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.spectral import KeplerianGLS

pytestmark = pytest.mark.gpu


def kernel_grid(freq):
    f0, delta, nf = _cabi.grid_params(freq)
    return f0 + np.arange(nf) * (delta if nf > 1 else 1.0)


def scan(t, y, err, freq, ecc, m0, **kw):
    f0, delta, nf = _cabi.grid_params(freq)
    if nf < 2:
        delta = 1.0
    kw.setdefault("want_cube", True)
    return _cabi.kepler_scan(t, y, err, f0, delta, nf, ecc, m0, **kw)


def assert_meets_oracle(label, got, exact, cond):
    """Prints the worst error over its gate and the share left out before it asserts."""
    worst, left_out = ko.compare(got, exact, cond)
    print(f"{label}: error / gate = {worst:.3e}, left out {left_out:.4f} (cap {ko.LEFT_OUT_CAP})")
    assert left_out <= ko.LEFT_OUT_CAP, (label, left_out)
    assert worst <= 1.0, (label, worst)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_reductions_follow_numpy(out):
    """power, cell and best are the numpy expressions on the returned cube, bit for bit."""
    power, cell, best = ko.reductions(out["cube"])
    assert np.array_equal(out["cell"], cell) and out["cell"].dtype == np.int32
    assert same(out["power"][cell >= 0], power[cell >= 0]) and np.all(np.isnan(out["power"][cell < 0]))
    assert out["best"][1:] == best[1:]
    assert out["best"][0] == best[0] or (np.isnan(out["best"][0]) and np.isnan(best[0]))


@functools.lru_cache(maxsize=None)
def curve(n, offset=0.0, every=1):
    """kepler_curve(n) on every ``every``-th bin of its grid, with the oracle's anomalies (shared by every option)."""
    t, y, err, freq, ecc, m0 = ko.kepler_curve(n, offset)
    freq = freq[::every]
    return (t, y, err, freq, ecc, m0), ko.anomalies(t, kernel_grid(freq), ecc, m0)


@functools.lru_cache(maxsize=None)
def exact_cube(n, weighted, fit_mean, offset=0.0, every=1):
    (t, y, err, freq, ecc, m0), nu = curve(n, offset, every)
    return ko.cube(t, y, err if weighted else None, kernel_grid(freq), ecc, m0, fit_mean, nu=nu)


@pytest.mark.parametrize("fit_mean", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
def test_cube_parity(weighted, fit_mean):
    (t, y, err, freq, ecc, m0), _ = curve(40)
    out = scan(t, y, err if weighted else None, freq, ecc, m0, fit_mean=fit_mean)
    assert out["cube"].shape == (80, 7, 12)
    assert_meets_oracle(f"n=40 weighted={weighted} fit_mean={fit_mean}", out["cube"], *exact_cube(40, weighted, fit_mean))
    assert_reductions_follow_numpy(out)


def test_psd_normalisation():
    (t, y, err, freq, ecc, m0), nu = curve(40)
    out = scan(t, y, err, freq, ecc, m0, psd=True)
    assert_meets_oracle("n=40 psd", out["cube"], *ko.cube(t, y, err, kernel_grid(freq), ecc, m0, psd=True, nu=nu))


def test_parity_at_a_julian_date_offset():
    (t, y, err, freq, ecc, m0), _ = curve(40, 2450000.0)
    out = scan(t, y, err, freq, ecc, m0)
    assert_meets_oracle("n=40 t + 2450000", out["cube"], *exact_cube(40, True, True, 2450000.0))
    # and the oracle of the curve without the offset: the two differ by the rounding of t + 2450000 alone
    assert_meets_oracle("n=40 t + 2450000 vs the oracle at t", out["cube"], *exact_cube(40, True, True))


def test_many_cycles():
    """f t' reaches 1e5 cycles: the phase must come from the exact product."""
    t, y, err, freq, ecc, m0 = ko.many_cycles_curve()
    assert kernel_grid(freq)[-1] * (t[-1] - t[0]) > 9e4
    out = scan(t, y, err, freq, ecc, m0)
    assert_meets_oracle("1e5 cycles", out["cube"], *ko.cube(t, y, err, kernel_grid(freq), ecc, m0))
    assert_reductions_follow_numpy(out)


def test_solver_sweep():
    """cos nu and sin nu of pdc_kepler_anomaly, the scan's own device function, within 1e-12 of the long-double solver:
    what Tier E needs at the keep rule (1e-6 relative in the power at condition <= 1e6 of the normal matrix)."""
    rng = np.random.default_rng(20261021)
    special = [0.0, 2.0 ** -30, -2.0 ** -30, 0.5 - 2.0 ** -53, -0.5 + 2.0 ** -53, 1e-3, -1e-3, 7.25, -123.5]
    phases = np.concatenate([rng.uniform(-0.5, 0.5, 4096), special])
    eccs = np.array([0.0, 1e-8, 0.1, 0.5, 0.9, 0.95])
    phase, e = np.repeat(phases, eccs.size), np.tile(eccs, phases.size)
    cos_nu, sin_nu = _cabi.kepler_anomaly(phase, e)
    want_c, want_s = ko.true_anomaly(phase.astype(ko.LD), e)
    worst = 0.0
    for value in eccs:
        pick = e == value
        dc = float(np.max(np.abs(cos_nu[pick] - want_c[pick])))
        ds = float(np.max(np.abs(sin_nu[pick] - want_s[pick])))
        print(f"solver e={value:g}: worst |d cos nu| = {dc:.3e}, |d sin nu| = {ds:.3e}")
        worst = max(worst, dc, ds)
    print(f"solver worst error {worst:.3e} (bound 1e-12)")
    assert worst <= 1e-12
    at_zero = phase == 0.0
    assert np.all(cos_nu[at_zero] == 1.0) and np.all(sin_nu[at_zero] == 0.0)   # periastron is exact


@pytest.mark.parametrize("weighted", [False, True])
def test_circular_row_is_the_gls_scan(weighted):
    (t, y, err, freq, ecc, m0), _ = curve(40)
    e = err if weighted else None
    out = scan(t, y, e, freq, ecc, m0)
    f0, delta, nf = _cabi.grid_params(freq)
    gls = _cabi.gls_scan(t, y, e, f0, delta, nf)
    assert ecc[0] == 0.0
    worst = float(np.max(np.abs(out["cube"][:, 0, :] - gls[:, None]) / (1e-6 * np.abs(gls[:, None]) + 1e-9)))
    print(f"e = 0 row vs gls_scan weighted={weighted}: error / gate = {worst:.3e}")
    assert worst <= 1.0


def test_reductions_bit_for_bit():
    (t, y, err, freq, ecc, m0), _ = curve(40)
    out = scan(t, y, err, freq, ecc, m0)
    assert_reductions_follow_numpy(out)
    assert out["best"][1] == ko.BEST_BIN
    bare = scan(t, y, err, freq, ecc, m0, want_cube=False)            # cube_out = NULL: the same bits
    assert bare["cube"] is None
    assert same(bare["power"], out["power"]) and same(bare["cell"], out["cell"]) and bare["best"] == out["best"]
    only_best = scan(t, y, err, freq, ecc, m0, want_cube=False, want_bins=False)
    assert only_best["power"] is None and only_best["best"] == out["best"]


def test_bins_without_a_value():
    """Four samples at one time: phi = 0 in every bin, and with m0 = 0 every sample sits at periastron exactly
    (cos nu = 1, sin nu = 0), so sum w sin^2 nu is exactly 0 and the second pivot is not > 0: every cell is NaN.  (With
    another m0 the columns are constant only to rounding, and a pivot may come out as a positive 1e-16.)"""
    t, y = np.full(4, 3.5), np.array([1.0, 2.0, 4.0, 3.0])
    for fit_mean in (True, False):
        out = scan(t, y, None, 0.1 + 0.1 * np.arange(5), [0.0, 0.3, 0.95], [0.0], fit_mean=fit_mean)
        assert np.all(np.isnan(out["cube"])) and np.all(np.isnan(out["power"])) and np.all(out["cell"] == -1)
        assert np.isnan(out["best"][0]) and out["best"][1:] == (-1, -1)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_sample_seams(n):
    (t, y, err, freq, ecc, m0), _ = curve(n, every=4)
    for weighted in (False, True):
        out = scan(t, y, err if weighted else None, freq, ecc, m0)
        assert_meets_oracle(f"n={n} weighted={weighted}", out["cube"], *exact_cube(n, weighted, True, every=4))


@pytest.mark.parametrize("nf", [255, 256, 257])
def test_tile_seams(nf):
    assert _cabi.kepler_tile_bins() == 256
    t, y, err, freq, ecc, m0 = ko.tile_seam_case(nf)
    out = scan(t, y, err, freq, ecc, m0)
    assert out["cube"].shape == (nf, 2, 2)
    assert_meets_oracle(f"nf={nf}", out["cube"], *ko.cube(t, y, err, kernel_grid(freq), ecc, m0))
    assert_reductions_follow_numpy(out)


@pytest.mark.parametrize("count", ["kc-1", "kc", "kc+1", "2kc+1", "1"])
def test_cell_group_seams(count):
    kc = _cabi.kepler_cell_group()
    count = max(1, {"kc-1": kc - 1, "kc": kc, "kc+1": kc + 1, "2kc+1": 2 * kc + 1, "1": 1}[count])
    t, y, err, freq, ecc, m0 = ko.cell_seam_case(count)
    assert ecc.size * m0.size == count
    out = scan(t, y, err, freq, ecc, m0)
    assert_meets_oracle(f"{count} cells", out["cube"], *ko.cube(t, y, err, kernel_grid(freq), ecc, m0))
    assert_reductions_follow_numpy(out)
    got_kc, groups, launches = _cabi.kepler_last_dispatch()
    assert (got_kc, groups, launches) == (kc, -(-count // kc), 1)
    assert groups > 1 or count <= kc   # more than one group ran where the cells do not fit one


def test_grouping_leaves_no_trace():
    """No bit of a cell depends on its place in the lists, on its group or on the other cells of the call."""
    t, y, err, freq, ecc, m0 = ko.no_trace_case()   # 30 cells, more than one group
    full = scan(t, y, err, freq, ecc, m0)
    assert _cabi.kepler_last_dispatch()[1] > 1
    rng = np.random.default_rng(5)
    pe, pm = rng.permutation(ecc.size), rng.permutation(m0.size)
    mixed = scan(t, y, err, freq, ecc[pe], m0[pm])
    assert same(mixed["cube"], full["cube"][:, pe][:, :, pm])
    assert same(mixed["power"], full["power"])   # the largest cell of a bin is the same value wherever it sits
    ke, km = np.array([4, 1]), np.array([5, 0, 2])
    part = scan(t, y, err, freq, ecc[ke], m0[km])
    assert same(part["cube"], full["cube"][:, ke][:, :, km])
    one = scan(t, y, err, freq, ecc[3:4], m0[4:5])
    assert same(one["cube"][:, 0, 0], full["cube"][:, 3, 4])


@pytest.mark.parametrize("n", [40, 65])
def test_recovery(n):
    (t, y, err, freq, ecc, m0), _ = curve(n)
    out = scan(t, y, err, freq, ecc, m0, want_cube=False)
    value, bin_, cell = out["best"]
    f0, delta, nf = _cabi.grid_params(freq)
    gls_peak = float(np.nanmax(_cabi.gls_scan(t, y, err, f0, delta, nf)))
    print(f"n={n}: Keplerian peak {value:.4f} at bin {bin_}, e = {ecc[cell // m0.size]:.2f}; GLS peak {gls_peak:.4f}")
    assert bin_ == ko.BEST_BIN and ecc[cell // m0.size] == pytest.approx(ko.BEST_ECC)
    assert value > gls_peak
    want_peak, want_gls = {40: (0.969, 0.685), 65: (0.973, 0.715)}[n]
    assert value == pytest.approx(want_peak, abs=5e-4) and gls_peak == pytest.approx(want_gls, abs=5e-4)
    # the class on GLS's own grid: orbit() is the long-double fit at the best bin's cell
    k = KeplerianGLS(0.02, 0.1, ecc=7, n_phase=12)
    p = k(TSeries(t, y), err)
    assert abs(1 / k.best.frequency - ko.PERIOD) <= 0.6   # (two bins of that grid)
    assert p.values[k.best_bin] == k.best.power == np.nanmax(p.values)
    orbit, want = k.orbit(), ko.fit(t, y, err, k.best.frequency, k.best.e, k.best.m0)
    for name in ("K", "gamma", "omega"):
        print(f"n={n} orbit {name}: {orbit[name]:.9g} (long double {want[name]:.9g})")
        assert orbit[name] == pytest.approx(want[name], rel=1e-6)
    assert orbit["period"] == 1 / k.best.frequency and orbit["e"] == k.best.e
    assert abs(orbit["K"] - ko.SEMI_AMPLITUDE) <= 5
    resid = y - k.model(t).values
    assert np.sum((resid / err) ** 2) < 0.2 * np.sum(((y - np.average(y, weights=err ** -2)) / err) ** 2)


def test_class_returns_what_the_library_computes():
    (t, y, err, _, _, _), _ = curve(40)
    k = KeplerianGLS(0.02, 0.1, 3, ecc=[0.0, 0.6, 0.3], n_phase=5)
    p = k(TSeries(t, y), err, want_cube=True)
    out = scan(t, y, err, k.frequency, k.ecc, k.m0)
    assert same(p.values, out["power"]) and same(k.cell, out["cell"]) and same(k.cube, out["cube"])
    assert np.array_equal(k.eccentricity, k.ecc[out["cell"] // 5]) and np.array_equal(k.periastron_phase, k.m0[out["cell"] % 5])
    assert (k.best.power, k.best_bin) == out["best"][:2] and k.best.frequency == k.frequency[out["best"][1]]
    k(TSeries(t, y), err, fit_mean=False)
    assert k.cube is None
    assert same(k.periodogram.values, scan(t, y, err, k.frequency, k.ecc, k.m0, fit_mean=False, want_cube=False)["power"])


def test_host_entry_and_dev_twin_are_bit_identical():
    (t, y, err, freq, ecc, m0), _ = curve(40)
    f0, delta, nf = _cabi.grid_params(freq)
    host = scan(t, y, err, freq, ecc, m0)
    DB = _cabi.DeviceBuffer
    dev = _cabi.default_device()
    cells = nf * ecc.size * m0.size
    ins = [DB.from_array(a, dev) for a in (t, y, err, ecc, m0)]
    sizes = ((nf, np.float64), (nf, np.int32), (cells, np.float64), (1, np.float64), (2, np.int64))
    outs = [DB(count * np.dtype(dtype).itemsize, dev) for count, dtype in sizes]
    try:
        _cabi.check(_cabi.lib().pdc_kepler_scan_dev(dev, None, ins[0].ptr, ins[1].ptr, ins[2].ptr, t.size, f0, delta, nf,
                                                    ins[3].ptr, ecc.size, ins[4].ptr, m0.size, 1, 0,
                                                    *[b.ptr for b in outs]))
        _cabi.check(_cabi.lib().pdc_device_sync(dev))
        power, cell, cube, best, best_at = [b.to_array(dtype, count) for b, (count, dtype) in zip(outs, sizes)]
    finally:
        for b in ins + outs:
            b.free()
    assert same(power, host["power"]) and same(cell, host["cell"]) and same(cube.reshape(host["cube"].shape), host["cube"])
    assert (float(best[0]), int(best_at[0]), int(best_at[1])) == host["best"]


def test_hygiene_no_allocation_on_a_repeated_or_rejected_call():
    (t, y, err, freq, ecc, m0), _ = curve(40)
    first = scan(t, y, err, freq, ecc, m0)
    _cabi.kepler_anomaly([0.1, 0.2], [0.3, 0.4])
    counts = _cabi.alloc_counts()
    again = scan(t, y, err, freq, ecc, m0)
    _cabi.kepler_anomaly([0.3, 0.2], [0.3, 0.4])
    assert _cabi.alloc_counts() == counts
    assert all(same(first[name], again[name]) for name in ("power", "cell", "cube")) and first["best"] == again["best"]
    f0, delta, nf = _cabi.grid_params(freq)
    good = dict(t=t, y=y, dy=err, f0=f0, delta=delta, nf=nf, ecc=ecc, m0=m0)
    for kw in (dict(ecc=np.array([0.96])), dict(ecc=np.array([-0.01])), dict(m0=np.array([1.0])),
               dict(ecc=np.array([0.1, np.nan])), dict(t=t[:3], y=y[:3], dy=None), dict(delta=0.0)):
        with pytest.raises(ValueError):
            _cabi.kepler_scan(**{**good, **kw})
    with pytest.raises(ValueError):   # every output NULL
        _cabi.check(_cabi.lib().pdc_kepler_scan(_cabi._ptr(t), _cabi._ptr(y), _cabi._ptr(err), t.size, f0, delta, nf,
                                                _cabi._ptr(ecc), ecc.size, _cabi._ptr(m0), m0.size, 1, 0, None, None, None,
                                                None, None, _cabi.default_device()))
    assert _cabi.alloc_counts() == counts


def test_slabs_under_a_budget_leave_no_trace(monkeypatch):
    """PDC_WORK_BUDGET_GB cuts the grid into slabs of whole tiles scanned one after the other: more launches, the same
    bits, and the best bin in ascending order across the slabs."""
    t, y, err, freq, ecc, m0 = ko.slab_case()   # three tiles
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    whole = scan(t, y, err, freq, ecc, m0)
    assert _cabi.kepler_last_dispatch()[2] == 1
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "0.00001")   # 10 KB: one tile per slab
    slabs = scan(t, y, err, freq, ecc, m0)
    assert _cabi.kepler_last_dispatch()[2] == 3
    assert all(same(whole[name], slabs[name]) for name in ("power", "cell", "cube")) and whole["best"] == slabs["best"]
    assert_reductions_follow_numpy(slabs)
