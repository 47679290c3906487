"""The GP likelihood scans on the GPU against the test-local oracle (tests/gp_oracle.py): every J with and without a
profiled mean across the staging seams and the workgroup seams, real / mixed / overdamped terms, awkward time axes, a
candidate that is not positive definite, fixed bits, the per-period fold, and a scan end to end.

The gate of every parity assertion is the oracle's: |got - exact| <= 16 kappa 2^-53 mag per candidate, no candidate left
out, every status 0.  Each test prints its worst error / gate."""
import itertools

import numpy as np
import pytest

import gp_oracle as go
from periodicity_amd import _cabi, gp
from periodicity_amd.core import FSeries, TSeries

pytestmark = pytest.mark.gpu


def held(tau, y, var, coeff, exact, fit_mean, label, jitter=go.JITTER):
    """One device call against its long-double answer: the worst error / gate, asserted <= 1; returns the device arrays."""
    ll, mean, status = _cabi.gp_loglike(tau, y, var, coeff, jitter, fit_mean=fit_mean)
    assert np.all(status == 0) and np.all(exact["status"] == 0)
    r = go.ratio(ll, exact)
    r_mean = 0.0
    if fit_mean:
        r_mean = float(np.max(np.abs(mean.astype(go.LD) - exact["mean"]).astype(float) / go.mean_gate(exact)))
    else:
        assert np.all(mean == 0.0)
    share = float(np.max((exact["mag_profile"] / exact["mag"]).astype(float)))   # (a figure only: what profiling adds to the sums)
    print(f"{label}: ln L error / gate {r:.3g}, mean error / gate {r_mean:.3g}, kappa up to {float(exact['kappa'].max()):.3g}, "
          f"profile term / mag up to {share:.3g}")
    assert r <= 1.0 and r_mean <= 1.0
    return ll, mean, status


@pytest.mark.parametrize("fit_mean", [False, True])
@pytest.mark.parametrize("J", [1, 2, 3, 4])
def test_parity_across_the_staging_and_workgroup_seams(J, fit_mean):
    assert _cabi.gp_max_terms() == 4
    chunk = _cabi.gp_chunk_samples()
    for n in (1, 2, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        tau, y, var, coeff, exact = go.parity_case(J, n, 257, fit_mean)
        ll, mean, _ = held(tau, y, var, coeff, exact, fit_mean, f"J={J} fit_mean={fit_mean} n={n} M=257")
        assert _cabi.gp_last_dispatch() == (J, int(fit_mean), 1)
        for M in (1, 63, 64, 65):          # the same candidates in a shorter call: held to the gate, and the same bits
            part = _cabi.gp_loglike(tau, y, var, coeff[:M], go.JITTER, fit_mean=fit_mean)
            assert np.all(part[2] == 0)
            assert np.all(np.abs(part[0].astype(go.LD) - exact["loglike"][:M]).astype(float) <= go.gate(exact)[:M])
            assert part[0].tobytes() == ll[:M].tobytes() and part[1].tobytes() == mean[:M].tobytes()


def test_real_mixed_and_overdamped_terms():
    tau, y, var = go.curve(33)
    w = 2 * np.pi / 3.1
    cases = {
        "one real term": np.array([[[0.25, 0.0, 0.2, 0.0]]]),
        "two real terms": np.array([[[0.2, 0.0, 0.05, 0.0], [0.1, 0.0, 1.5, 0.0]]]),
        "real + complex": np.array([np.concatenate([[[0.1, 0.0, 0.3, 0.0]], go.sho(0.2 / (w * 4.0), w, 4.0)])]),
        "complex + real + real": np.array([np.concatenate([go.sho(0.2 / (w * 4.0), w, 4.0), [[0.05, 0.0, 0.3, 0.0]],
                                                           [[0.05, 0.0, 2.0, 0.0]]])]),
        "overdamped SHO (a- < 0)": np.array([go.sho(0.3 / (w * 0.1), w, 0.1)]),
        "overdamped + underdamped": np.array([np.concatenate([go.sho(0.2 / (w * 0.05), w, 0.05), go.rotation(0.3, 3.1, 5.0, 1.0, 0.5)])]),
    }
    assert cases["overdamped SHO (a- < 0)"][0, 1, 0] < 0
    for label, terms in cases.items():
        coeff = go.to_device(terms)
        for fit_mean in (False, True):
            exact = go.recursion(tau, y, var, coeff, go.JITTER, fit_mean=fit_mean)
            held(tau, y, var, coeff, exact, fit_mean, f"{label}, fit_mean={fit_mean}")


def test_duplicate_timestamps_and_a_gap_that_underflows():
    tau, y, var = go.curve(24)
    coeff = go.kernels(2, 9)
    # every time twice
    twice = np.repeat(tau, 2)
    y2, var2 = np.repeat(y, 2) + 0.01 * np.arange(48) % 0.03, np.repeat(var, 2)
    for fit_mean in (False, True):
        held(twice, y2, var2, coeff, go.recursion(twice, y2, var2, coeff, go.JITTER, fit_mean=fit_mean), fit_mean,
             f"every time twice, fit_mean={fit_mean}")
    # a gap of 5000: c dtau > 746 for every term, the propagator is exactly 0 and the halves' likelihoods add
    tau = np.round(tau * 2.0 ** 20) / 2.0 ** 20            # (so that tau + 5000 is exact: the halves see the same steps)
    far = np.concatenate([tau, tau + 5000.0])
    coeff = go.to_device(np.array([go.rotation(0.5, p, 2.0, 1.0, 0.5) for p in (2.5, 3.1, 4.0)]))
    assert np.all(coeff[:, :, 2] * (5000.0 - tau[-1]) > 746)
    exact_whole = go.recursion(far, np.tile(y, 2), np.tile(var, 2), coeff, go.JITTER)
    exact_half = go.recursion(tau, y, var, coeff, go.JITTER)
    whole, _, _ = held(far, np.tile(y, 2), np.tile(var, 2), coeff, exact_whole, False, "a gap of 5000")
    half, _, _ = held(tau, y, var, coeff, exact_half, False, "one half")
    assert np.all(np.isfinite(whole))
    assert np.all(np.abs(whole - 2 * half) <= go.gate(exact_whole) + 2 * go.gate(exact_half))
    assert np.all(np.abs(exact_whole["loglike"] - 2 * exact_half["loglike"]) <= 1e-15 * np.abs(exact_whole["loglike"]))


def test_julian_dates_give_the_bytes_of_the_unshifted_curve():
    tau, y, var = go.curve(65)
    tau = np.round(tau * 2.0 ** 20) / 2.0 ** 20            # t - t[0] is then the same array with and without the offset
    t0 = 2.45e6 + 0.25
    assert np.array_equal((tau + t0) - (tau + t0)[0], tau)
    terms = np.array([go.rotation(0.5, p, 2.0, 1.0, 0.5) for p in (2.5, 3.1, 4.0)])
    order = np.random.default_rng(3).permutation(65)      # and the class sorts
    plain = gp.CeleriteLikelihood((tau, y), np.sqrt(var))(terms, jitter=go.JITTER)
    shifted = gp.CeleriteLikelihood(((tau + t0)[order], y[order]), np.sqrt(var)[order])(terms, jitter=go.JITTER)
    assert plain.log_likelihood.tobytes() == shifted.log_likelihood.tobytes() and plain.mean.tobytes() == shifted.mean.tobytes()
    assert np.all(plain.status == 0) and np.all(np.isfinite(plain.log_likelihood))
    fixed = gp.CeleriteLikelihood(TSeries(tau + t0, y), np.sqrt(var))(terms, jitter=go.JITTER, mean=0.1)
    assert fixed.log_likelihood.tobytes() == gp.CeleriteLikelihood((tau, y), np.sqrt(var))(terms, go.JITTER, 0.1).log_likelihood.tobytes()


def test_a_candidate_that_is_not_positive_definite_sits_between_good_ones():
    tau, y, var = go.curve(40)
    var = var * 0.01                                        # small uncertainties: nothing props the matrix up
    good = go.kernels(1, 6)
    bad = [np.array([[-1.0, 0.0, 0.5, 0.0]]),               # a negative variance: the first D already
           go.to_device(np.array([[0.2, 3.0, 0.05, 2.0]]))]   # |b| far beyond what a valid term allows: a later D
    coeff = np.concatenate([good[:2], bad[0][None], good[2:4], bad[1][None], good[4:]])
    exact = go.recursion(tau, y, var, coeff, 0.0, fit_mean=True)
    double = go.recursion(tau, y, var, coeff, 0.0, fit_mean=True, dtype=np.float64)
    assert exact["status"][2] == 1 and exact["status"][5] > 1 and np.array_equal(exact["status"], double["status"])
    ll, mean, status = _cabi.gp_loglike(tau, y, var, coeff, 0.0, fit_mean=True)
    assert np.array_equal(status, exact["status"]) and status[[0, 1, 3, 4, 6, 7]].tolist() == [0] * 6
    assert ll[2] == -np.inf and ll[5] == -np.inf and np.isnan(mean[2]) and np.isnan(mean[5])
    alone = _cabi.gp_loglike(tau, y, var, good, 0.0, fit_mean=True)
    keep = [0, 1, 3, 4, 6, 7]
    assert ll[keep].tobytes() == alone[0].tobytes() and mean[keep].tobytes() == alone[1].tobytes()
    assert np.all(np.isfinite(alone[0])) and np.all(alone[2] == 0)


def test_fixed_bits(monkeypatch):
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    tau, y, var, coeff, _ = go.parity_case(2, 129, 257, True)
    jitter = np.linspace(1e-4, 5e-4, 257)
    ll, mean, status = _cabi.gp_loglike(tau, y, var, coeff, jitter, fit_mean=True)
    assert _cabi.gp_last_dispatch() == (2, 1, 1)
    again = _cabi.gp_loglike(tau, y, var, coeff, jitter, fit_mean=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((ll, mean, status), again))          # two calls
    order = np.random.default_rng(11).permutation(257)
    moved = _cabi.gp_loglike(tau, y, var, coeff[order], jitter[order], fit_mean=True)
    assert moved[0].tobytes() == ll[order].tobytes() and moved[1].tobytes() == mean[order].tobytes()   # its position
    for M in (1, 64, 130):
        part = _cabi.gp_loglike(tau, y, var, coeff[100:100 + M], jitter[100:100 + M], fit_mean=True)
        assert part[0].tobytes() == ll[100:100 + M].tobytes()                                  # M and its neighbours
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "0.00001")                                        # slabs of one workgroup
    slabbed = _cabi.gp_loglike(tau, y, var, coeff, jitter, fit_mean=True)
    assert _cabi.gp_last_dispatch() == (2, 1, 5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((ll, mean, status), slabbed))
    scanned = _cabi.gp_scan(tau, y, var, coeff[:256], 64, jitter[:256], fit_mean=True, want_cube=True)
    assert _cabi.gp_last_dispatch() == (2, 1, 4) and scanned["cube"].tobytes() == ll[:256].tobytes()
    monkeypatch.delenv("PDC_WORK_BUDGET_GB")
    # the `_dev` entry on resident arrays
    DB = _cabi.DeviceBuffer
    fixed_mean = np.linspace(-0.1, 0.1, 257)
    host = _cabi.gp_loglike(tau, y, var, coeff, jitter, mean=fixed_mean)
    bufs = [DB.from_array(a) for a in (tau, y, var, coeff, jitter, fixed_mean)] + [DB(257 * 8), DB(257 * 8), DB(257 * 4)]
    try:
        _cabi.check(_cabi.lib().pdc_gp_loglike_dev(0, None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 129, bufs[3].ptr, 2,
                                                   bufs[4].ptr, bufs[5].ptr, 257, 0, bufs[6].ptr, bufs[7].ptr, bufs[8].ptr))
        _cabi.check(_cabi.lib().pdc_device_sync(0))
        assert bufs[6].to_array(np.float64, 257).tobytes() == host[0].tobytes()
        assert bufs[7].to_array(np.float64, 257).tobytes() == host[1].tobytes() == fixed_mean.tobytes()
        assert bufs[8].to_array(np.int32, 257).tobytes() == host[2].tobytes()
        _cabi.check(_cabi.lib().pdc_gp_loglike_dev(0, None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 129, bufs[3].ptr, 2,
                                                   bufs[4].ptr, None, 257, 1, bufs[6].ptr, bufs[7].ptr, None))
        _cabi.check(_cabi.lib().pdc_device_sync(0))
        assert bufs[6].to_array(np.float64, 257).tobytes() == ll.tobytes()
        assert bufs[7].to_array(np.float64, 257).tobytes() == mean.tobytes()
    finally:
        for b in bufs:
            b.free()
    # a mean per candidate is the mean taken off the curve
    one = _cabi.gp_loglike(tau, y - 0.05, var, coeff[:5], jitter[:5])
    per = _cabi.gp_loglike(tau, y, var, coeff[:5], jitter[:5], mean=np.full(5, 0.05))
    exact = go.recursion(tau, y, var, coeff[:5], jitter[:5], mean=np.full(5, 0.05))
    assert go.ratio(per[0], exact) <= 1.0 and go.ratio(one[0], exact) <= 1.0


def check_fold(out, n_periods, nq):
    cube = out["cube"]
    profile, cell, marginal, best = go.fold(cube)
    assert out["profile"].tobytes() == profile.tobytes() and out["cell"].tobytes() == cell.tobytes()
    assert out["best"][1:] == best[1:] and (out["best"][0] == best[0] or (np.isnan(best[0]) and np.isnan(out["best"][0])))
    some = cell >= 0
    assert np.all(out["marginal"][~some] == -np.inf) and np.all(np.isnan(out["mean"][~some]))
    err = np.abs(out["marginal"][some] - marginal[some])
    bound = 4 * 2.0 ** -52 * (np.abs(marginal[some]) + np.log(nq))
    print(f"fold {n_periods} x {nq}: marginal error / bound {float(np.max(err / bound)) if some.any() else 0.0:.3g}")
    assert np.all(err <= bound)
    return profile, cell, marginal, best


def test_the_fold_is_the_numpy_expression_on_the_returned_cube():
    tau, y, var = go.curve(17)
    var = var * 0.01
    good = go.kernels(2, 30).reshape(6, 5, 2, 4).copy()
    bad = np.array([[-1.0, 0.0, 0.5, 0.0], [0.0, 0.0, 0.0, 0.0]])
    good[1, :] = bad                          # a period without a positive definite cell
    good[2, 0] = bad                          # ... with some
    good[2, 3] = bad
    good[3, 4] = good[3, 1]                   # ties: the first cell wins
    good[4, :] = good[4, 2]
    out = _cabi.gp_scan(tau, y, var, good.reshape(30, 2, 4), 6, 0.0, fit_mean=True, want_cube=True)
    profile, cell, marginal, best = check_fold(out, 6, 5)
    assert cell[1] == -1 and np.isnan(profile[1]) and cell[4] == 0 and cell[3] != 4 and np.all(np.isinf(out["cube"][1]))
    assert np.isneginf(out["cube"][2, [0, 3]]).all() and cell[2] in (1, 2, 4)
    # the cube is what the likelihood entry gives, and the means are those of the best cells
    ll, mean, _ = _cabi.gp_loglike(tau, y, var, good.reshape(30, 2, 4), 0.0, fit_mean=True)
    assert out["cube"].tobytes() == ll.tobytes()
    some = cell >= 0
    assert out["mean"][some].tobytes() == mean.reshape(6, 5)[np.flatnonzero(some), cell[some]].tobytes()
    # nothing positive definite anywhere
    none = _cabi.gp_scan(tau, y, var, np.tile(bad, (6, 1, 1)), 3, 0.0, want_cube=True)
    assert np.isnan(none["best"][0]) and none["best"][1:] == (-1, -1) and np.all(none["cell"] == -1)
    check_fold(none, 3, 2)
    # more periods than one fold tile, the best in a later tile, equal maxima in two tiles: the first period wins
    many = go.kernels(2, 700).reshape(350, 2, 2, 4).copy()
    many[300] = many[20]
    wide = _cabi.gp_scan(tau, y, var, many.reshape(700, 2, 4), 350, go.JITTER, fit_mean=False, want_cube=True)
    profile, cell, _, best = check_fold(wide, 350, 2)
    assert profile[300] == profile[20]
    top = many.copy()
    at = int(np.argmax(profile))
    top[299], top[340] = many[at], many[at]
    tied = _cabi.gp_scan(tau, y, var, top.reshape(700, 2, 4), 350, go.JITTER, fit_mean=False, want_cube=True)
    assert check_fold(tied, 350, 2)[3][1] == min(at, 299)
    # the `_dev` scan on resident arrays, no cube asked for: the same fold
    DB = _cabi.DeviceBuffer
    jit = np.full(700, go.JITTER)
    bufs = [DB.from_array(a) for a in (tau, y, var, many.reshape(700, 2, 4), jit)] + [DB(350 * 8), DB(350 * 4), DB(350 * 8),
                                                                                       DB(350 * 8), DB(8), DB(16)]
    try:
        _cabi.check(_cabi.lib().pdc_gp_scan_dev(0, None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 17, bufs[3].ptr, 2, bufs[4].ptr,
                                                None, 700, 0, 350, 2, bufs[5].ptr, bufs[6].ptr, bufs[7].ptr, bufs[8].ptr,
                                                None, bufs[9].ptr, bufs[10].ptr))
        _cabi.check(_cabi.lib().pdc_device_sync(0))
        assert bufs[5].to_array(np.float64, 350).tobytes() == wide["profile"].tobytes()
        assert bufs[6].to_array(np.int32, 350).tobytes() == wide["cell"].tobytes()
        assert bufs[7].to_array(np.float64, 350).tobytes() == wide["marginal"].tobytes()
        assert bufs[8].to_array(np.float64, 350).tobytes() == wide["mean"].tobytes()
        assert float(bufs[9].to_array(np.float64, 1)[0]) == wide["best"][0]
        assert tuple(bufs[10].to_array(np.int64, 2)) == wide["best"][1:]
    finally:
        for b in bufs:
            b.free()


def test_a_scan_end_to_end():
    t, y, err = go.spot_curve()
    periods = np.linspace(2.0, 5.0, 64)
    nearest = periods[np.argmin(np.abs(periods - go.PERIOD))]
    lists = ([1.0, 5.0, 25.0], [0.5, 5.0], [0.2, 1.0])
    h = gp.HarmonicGP(TSeries(t, y), err)
    s = h.scan(periods, *lists, want_cube=True)
    assert s.cube.shape == (64, 12) and np.all(np.isfinite(s.cube))
    # the oracle on the same grid: its own best period is the nearest one, and the device holds the gate on every cell
    cells = np.array(list(itertools.product(*lists)))
    coeff = go.to_device(np.array([go.rotation(h.sigma, p, *c) for p in periods for c in cells]))
    exact = go.recursion(h.tau, h.y - np.mean(h.y), h.var, coeff, h.jitter, fit_mean=True)
    want = go.fold(exact["loglike"].astype(np.float64).reshape(64, 12))
    assert periods[want[3][1]] == nearest
    r = go.ratio(s.cube.ravel(), exact)
    print(f"HarmonicGP.scan 64 x 12: ln L error / gate {r:.3g}; best period {s.best['period']:.4f}, ln L {s.best['log_likelihood']:.3f}")
    assert r <= 1.0
    assert s.best["period"] == nearest and s.best["index"] == want[3][1] and s.best["cell"] == want[3][2]
    # the fields agree with the cube
    profile, cell, marginal, best = go.fold(s.cube)
    assert s.log_likelihood.tobytes() == profile.tobytes() and s.cell.tobytes() == cell.tobytes()
    assert np.all(np.abs(s.marginal - marginal) <= 4 * 2.0 ** -52 * (np.abs(marginal) + np.log(12)))
    assert np.all(s.marginal <= s.log_likelihood) and np.all(s.marginal >= s.log_likelihood - np.log(12))
    for i in (0, best[1], 63):
        assert s.params(i) == dict(zip(("Q0", "dQ", "f"), cells[cell[i]]))
    assert {k: s.best[k] for k in ("Q0", "dQ", "f")} == s.params(best[1]) and s.best["log_likelihood"] == best[0]
    assert np.all(np.abs(s.mean.astype(go.LD) - (exact["mean"].reshape(64, 12)[np.arange(64), cell] + np.mean(h.y)))
                  <= go.mean_gate(exact).reshape(64, 12)[np.arange(64), cell] + 1e-16)
    assert s.best["mean"] == s.mean[best[1]] and abs(s.best["mean"]) < 0.2
    assert isinstance(s.periodogram, FSeries) and np.array_equal(s.periodogram.values, profile[::-1])
    assert s.periodogram.period_at_highest_peak == pytest.approx(nearest)
    # without fit_mean the curve's mean is used, and no likelihood is above the profiled one
    fixed = h.scan(periods, *lists, fit_mean=False, want_cube=True)
    assert np.all(fixed.cube <= s.cube + 2 * go.gate(exact).max()) and np.all(fixed.mean == np.mean(h.y)) and fixed.best["period"] == nearest
    # the Brownian kernel (J = 3) through its class, against the oracle
    b = gp.BrownianGP(TSeries(t, y), err)
    sb = b.scan(periods[16:32], tau=[1.0, 4.0], mix=[0.1, 0.4], tau_in_periods=True, want_cube=True)
    cb = go.to_device(gp.brownian_terms(b.sigma, np.repeat(periods[16:32], 4) * np.tile([1.0, 1.0, 4.0, 4.0], 16),
                                        np.repeat(periods[16:32], 4), np.tile([0.1, 0.4], 32)))
    eb = go.recursion(b.tau, b.y - np.mean(b.y), b.var, cb, b.jitter, fit_mean=True)
    rb = go.ratio(sb.cube.ravel(), eb)
    print(f"BrownianGP.scan 16 x 4: ln L error / gate {rb:.3g}; best period {sb.best['period']:.4f}")
    wb = go.fold(eb["loglike"].astype(np.float64).reshape(16, 4))[3]
    assert rb <= 1.0 and _cabi.gp_last_dispatch()[0] == 3 and (sb.best["index"], sb.best["cell"]) == wb[1:]
