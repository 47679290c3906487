"""The GP likelihood scans without a GPU: the test-local oracle (tests/gp_oracle.py) against itself - the recursion against
the dense long-double Cholesky, float64 against long double inside the gate -, the term builders against closed forms,
the profiled mean, every refusal of the C entries, the size functions, the host classes' argument rules.  Nothing here
computes a likelihood with the package: without a GPU the package refuses."""
import itertools

import numpy as np
import pytest

import gp_oracle as go
from periodicity_amd import _cabi, gp
from periodicity_amd.core import TSeries


@pytest.mark.parametrize("J", [1, 2, 3, 4])
def test_recursion_oracle_matches_the_dense_cholesky(J):
    for n in (1, 2, 3, 17, 48):
        tau, y, var = go.curve(n)
        coeff = go.kernels(J, 6)
        for fit_mean in (False, True):
            rec = go.recursion(tau, y, var, coeff, go.JITTER, fit_mean=fit_mean)
            assert np.all(rec["status"] == 0)
            for m in range(6):
                ll, mean = go.dense_loglike(tau, y, var, coeff[m], go.JITTER, fit_mean=fit_mean)
                assert abs(rec["loglike"][m] - ll) <= 1e-12 * abs(ll)
                assert abs(rec["mean"][m] - mean) <= 1e-12 * max(abs(mean), 1.0)


@pytest.mark.parametrize("J", [1, 2, 3, 4])
def test_float64_oracle_stays_inside_a_quarter_of_the_gate(J):
    """The reference side alone: the same recursion in float64 against long double, every candidate positive definite."""
    worst = 0.0
    for n in (1, 2, 3, 33, 200, 600):
        tau, y, var = go.curve(n)
        coeff = go.kernels(J, 12)
        for fit_mean in (False, True):
            exact = go.recursion(tau, y, var, coeff, go.JITTER, fit_mean=fit_mean)
            double = go.recursion(tau, y, var, coeff, go.JITTER, fit_mean=fit_mean, dtype=np.float64)
            assert np.all(double["status"] == 0)
            r = go.ratio(double["loglike"], exact)
            print(f"J={J} n={n} fit_mean={fit_mean}: float64 / gate = {r:.3g}, kappa up to {float(exact['kappa'].max()):.3g}, "
                  f"gates {go.gate(exact).min():.2e} .. {go.gate(exact).max():.2e}")
            worst = max(worst, r)
    assert worst <= 0.25


def test_oracle_takes_a_gap_that_underflows_and_a_bad_candidate():
    """c dtau > 746: the propagator is exactly 0 and the halves' likelihoods add; a = -1 is not positive definite."""
    tau, y, var = go.curve(24)
    tau = np.round(tau * 2.0 ** 20) / 2.0 ** 20      # (so that tau + 5000 is exact: the halves see the same steps)
    far = np.concatenate([tau, tau + 5000.0])
    coeff = go.to_device(np.array([go.rotation(0.5, 3.1, 2.0, 1.0, 0.5)]))
    assert np.all(coeff[0, :, 2] * (5000.0 - tau[-1]) > 746)
    whole = go.recursion(far, np.tile(y, 2), np.tile(var, 2), coeff, go.JITTER)
    half = go.recursion(tau, y, var, coeff, go.JITTER)
    assert abs(whole["loglike"][0] - 2 * half["loglike"][0]) <= 1e-15 * abs(whole["loglike"][0])
    bad = go.recursion(tau, y, var, np.array([[[-1.0, 0.0, 0.5, 0.0]]]), go.JITTER)
    assert bad["status"][0] == 1 and bad["loglike"][0] == -np.inf and np.isnan(bad["mean"][0])


def test_fold_oracle():
    cube = np.array([[1.0, 5.0, 5.0], [-np.inf, -np.inf, -np.inf], [9.0, -np.inf, 9.0], [np.nan, 2.0, np.inf]])
    profile, cell, marginal, best = go.fold(cube)
    assert cell.tolist() == [1, -1, 0, 1] and cell.dtype == np.int32
    assert profile[0] == 5.0 and np.isnan(profile[1]) and profile[2] == 9.0 and profile[3] == 2.0
    assert marginal[1] == -np.inf and marginal[3] == 2.0 - np.log(3.0)
    assert marginal[0] == pytest.approx(np.log((np.e + 2 * np.e ** 5) / 3), rel=1e-15)
    assert best == (9.0, 2, 0)
    assert go.fold(np.full((2, 2), -np.inf))[3][1:] == (-1, -1)


# ---- the term builders ------------------------------------------------------------------------------------------------
def test_rotation_terms():
    sigma, period = np.array([0.7, 1.3, 2.0]), np.array([3.1, 4.0, 0.5])
    terms = gp.rotation_terms(sigma, period, [0.3, 2.0, 300.0], [0.0, 1.0, 5.0], [0.0, 0.5, 1.0])
    assert terms.shape == (3, 2, 4)
    assert np.allclose(terms[:, :, 0].sum(axis=1), sigma ** 2, rtol=1e-14, atol=0)     # sum a = sigma^2
    for m, args in enumerate(zip(sigma, period, [0.3, 2.0, 300.0], [0.0, 1.0, 5.0], [0.0, 0.5, 1.0])):
        assert np.allclose(terms[m], go.rotation(*args), rtol=1e-14, atol=0)
    # the primary oscillates at the period, the secondary at half of it
    assert np.allclose(2 * np.pi / terms[:, 0, 3], period) and np.allclose(2 * np.pi / terms[:, 1, 3], period / 2)
    assert gp.rotation_terms(1.0, 3.0, 1.0, 1.0, 0.5).shape == (1, 2, 4)
    for bad in ((1.0, -3.0, 1.0, 1.0, 0.5), (1.0, 3.0, 0.0, 1.0, 0.5), (1.0, 3.0, 1.0, -1.0, 0.5), (1.0, 3.0, 1.0, 1.0, -0.5)):
        with pytest.raises(ValueError):
            gp.rotation_terms(*bad)


def test_sho_terms_against_the_closed_form_kernel():
    lags = np.array([0.0, 0.3, 1.0, 2.5, 7.0])
    for S0, w0, Q in ((0.8, 2.0, 0.1), (0.8, 2.0, 0.45), (1.5, 0.7, 0.01), (0.8, 2.0, 3.0), (0.3, 5.0, 0.6)):
        terms = gp.sho_terms(S0, w0, Q)
        assert terms.shape == (1, 2 if Q < 0.5 else 1, 4)
        if Q < 0.5:   # overdamped: two real terms, the faster one with a negative amplitude
            assert np.all(terms[0, :, [1, 3]] == 0) and terms[0, 1, 0] < 0 < terms[0, 0, 0] and terms[0, 1, 2] > terms[0, 0, 2]
        got = go.kernel_value(go.to_device(terms)[0], lags).astype(float)
        want = go.sho_kernel(S0, w0, Q, lags)
        # (the closed form multiplies cosh(245) by exp(-245) at Q = 0.01: its argument's rounding, 245 x 2^-53, is the error)
        assert np.max(np.abs(got - want)) <= 1e-12 * want[0]
        assert np.allclose(terms[0], go.sho(S0, w0, Q), rtol=1e-15, atol=0)
    by_sigma = gp.sho_terms(sigma=[1.2, 0.5], tau=[4.0, 9.0], rho=[3.0, 2.0])
    w0, Q = 2 * np.pi / np.array([3.0, 2.0]), np.pi * np.array([4.0, 9.0]) / np.array([3.0, 2.0])
    assert np.allclose(by_sigma, gp.sho_terms(np.array([1.2, 0.5]) ** 2 / (w0 * Q), w0, Q), rtol=1e-15, atol=0)
    assert np.allclose(by_sigma[:, 0, 0], [1.44, 0.25], rtol=1e-14)
    for bad in (dict(S0=1.0, w0=1.0, Q=0.5), dict(S0=1.0, w0=1.0, Q=[0.2, 3.0]), dict(S0=1.0, w0=-1.0, Q=1.0),
                dict(S0=1.0, w0=1.0, Q=0.0), dict(S0=1.0, w0=1.0), dict(S0=1.0, w0=1.0, Q=1.0, sigma=1.0),
                dict(sigma=1.0, tau=1.0), dict(S0=np.nan, w0=1.0, Q=1.0), dict(S0=np.ones((2, 2)), w0=1.0, Q=1.0)):
        with pytest.raises(ValueError):
            gp.sho_terms(**bad)


def test_brownian_terms():
    """The reference's BrownianTerm: k(0) = sigma^2 (1 - (1 - mix)(1 - f) / (1 + f)) with f = sqrt(1 - 4 * 0.01^2) - the slow
    mode carries (1 - mix) sigma^2 exactly, the fast one takes a^- = -(1 - mix) sigma^2 (1 - f) / (1 + f) off: sigma^2 to
    within 1.0003e-4 (1 - mix) of itself, and exactly sigma^2 at mix = 1."""
    sigma, tau, period, mix = np.array([0.9, 1.4, 2.0]), np.array([5.0, 3.0, 40.0]), np.array([3.0, 3.0, 7.0]), np.array([0.3, 0.0, 1.0])
    terms = gp.brownian_terms(sigma, tau, period, mix)
    assert terms.shape == (3, 3, 4)
    f = np.sqrt(1 - 4 * 0.01 ** 2)
    k0 = terms[:, :, 0].sum(axis=1)
    assert np.allclose(k0, sigma ** 2 * (1 - (1 - mix) * (1 - f) / (1 + f)), rtol=1e-13, atol=0)
    assert np.all(np.abs(k0 / sigma ** 2 - 1) <= (1 - mix) * (1 - f) / (1 + f) * (1 + 1e-9) + 1e-14) and (1 - f) / (1 + f) < 1.0003e-4
    assert k0[2] == pytest.approx(sigma[2] ** 2, rel=1e-14)
    assert np.allclose(terms[:, 1, 0], (1 - mix) * sigma ** 2, rtol=1e-13, atol=0)     # the slow mode's amplitude
    assert np.allclose(terms[:, 1, 2], 1 / tau, rtol=1e-9)                             # ... decays on tau
    assert np.allclose(terms[:, 0], gp.sho_terms(sigma=sigma * np.sqrt(mix), tau=tau, rho=period)[:, 0], rtol=1e-15, atol=0)
    for bad in ((1.0, 0.4, 3.0, 0.3), (1.0, -1.0, 3.0, 0.3), (1.0, 5.0, 3.0, 1.5), (1.0, 5.0, 0.0, 0.3)):
        with pytest.raises(ValueError):
            gp.brownian_terms(*bad)


def test_device_coefficients():
    terms = gp.rotation_terms([1.0, 2.0], 3.0, 1.0, 1.0, 0.5)
    coeff = gp.device_coefficients(terms)
    assert coeff.flags.c_contiguous and coeff.dtype == np.float64 and np.array_equal(coeff, go.to_device(terms))
    assert np.array_equal(coeff[:, :, :3], terms[:, :, :3]) and np.array_equal(coeff[:, :, 3], terms[:, :, 3] / (2 * np.pi))
    assert gp.device_coefficients(terms[0]).shape == (1, 2, 4)
    for bad in (np.zeros(4), np.zeros((2, 2, 3)), np.zeros((0, 2, 4)), np.zeros((2, 0, 4))):
        with pytest.raises(ValueError):
            gp.device_coefficients(bad)


# ---- the profiled mean ------------------------------------------------------------------------------------------------
def test_profiled_mean_is_the_maximum_and_matches_a_direct_evaluation():
    tau, y, var = go.curve(33)
    y = y + 0.37
    for J in (1, 2, 3, 4):
        coeff = go.kernels(J, 6)
        prof = go.recursion(tau, y, var, coeff, go.JITTER, fit_mean=True)
        at = go.recursion(tau, y, var, coeff, go.JITTER, mean=prof["mean"])
        # (both in long double: 2^-64 times the kappa of a few hundred)
        assert np.max(np.abs(at["loglike"] - prof["loglike"])) <= 1e-13 * np.max(np.abs(prof["loglike"]))
        for step in (-1e-3, 1e-3):
            beside = go.recursion(tau, y, var, coeff, go.JITTER, mean=prof["mean"] + step)
            assert np.all(beside["loglike"] < prof["loglike"])
        for m in range(6):
            ll, mean = go.dense_loglike(tau, y, var, coeff[m], go.JITTER, fit_mean=True)
            assert abs(prof["mean"][m] - mean) <= 1e-14 and abs(prof["loglike"][m] - ll) <= 1e-13 * abs(ll)


# ---- the C entries without a device ------------------------------------------------------------------------------------
def _good():
    tau, y, var = go.curve(17)
    return dict(t_rel=tau, y=y, var=var, coeff=go.kernels(2, 6), jitter=go.JITTER)


def _refusals():
    g = _good()
    tau, y, var, coeff = g["t_rel"], g["y"], g["var"], g["coeff"]

    def poke(a, index, value):
        b = np.array(a, dtype=float)
        b[index] = value
        return b

    return [
        (dict(t_rel=tau[:0], y=y[:0], var=var[:0]), "1 <= n"),
        (dict(coeff=np.zeros((6, 5, 4))), "1 <= J"),
        (dict(coeff=np.zeros((0, 2, 4))), "1 <= M"),
        (dict(mean=np.zeros(6), fit_mean=True), "fit_mean"),
        (dict(t_rel=tau + 1.0), "start at 0"),
        (dict(t_rel=poke(tau, 5, np.nan)), "not finite"),
        (dict(t_rel=poke(tau, 5, tau[3])), "never decrease"),
        (dict(y=poke(y, 2, np.inf)), "y[2] is not finite"),
        (dict(var=poke(var, 4, -1e-9)), "var[4]"),
        (dict(var=poke(var, 4, np.nan)), "var[4]"),
        (dict(coeff=poke(coeff, (3, 1, 0), np.nan)), "coefficient of candidate 3"),
        (dict(coeff=poke(coeff, (2, 0, 2), -0.1)), "c of term 0 of candidate 2"),
        (dict(jitter=-1.0), "jitter[0]"),
        (dict(jitter=poke(np.zeros(6), 4, np.inf)), "jitter[4]"),
        (dict(mean=poke(np.zeros(6), 1, np.nan)), "mean[1]"),
    ]


def test_every_refusal_of_both_entries_raises_with_the_librarys_message(monkeypatch):
    for kw, text in _refusals():
        with pytest.raises(ValueError, match=text.replace("[", r"\[").replace("]", r"\]")):
            _cabi.gp_loglike(**{**_good(), **kw})
        if "coeff" in kw and kw["coeff"].shape[0] != 6:
            continue   # (the scan's own M = np nq check comes first there)
        with pytest.raises(ValueError, match=text.replace("[", r"\[").replace("]", r"\]")):
            _cabi.gp_scan(n_periods=3, **{**_good(), **kw})
    with pytest.raises(ValueError, match="np x nq must be M"):
        _cabi.gp_scan(n_periods=4, **_good())                    # 6 candidates are not 4 periods of whole cells
    with pytest.raises(ValueError, match="np x nq must be M"):
        _cabi.gp_scan(n_periods=0, **_good())
    g = _good()
    many = np.tile(g["coeff"][:1], (65536, 1, 1))
    with pytest.raises(ValueError, match="nq <= 65535"):
        _cabi.gp_scan(n_periods=1, **{**g, "coeff": many})
    # shapes the binding refuses before the library is asked
    with pytest.raises(ValueError):
        _cabi.gp_loglike(**{**g, "y": g["y"][:-1]})
    with pytest.raises(ValueError):
        _cabi.gp_loglike(**{**g, "coeff": np.zeros((6, 2, 3))})
    # every output NULL, through the raw entries (host arrays stand in for the `_dev` form's pointers: it checks first)
    lib, p = _cabi.lib(), _cabi._ptr
    jit = np.full(6, go.JITTER)
    head = (p(g["t_rel"]), p(g["y"]), p(g["var"]), 17, p(g["coeff"]), 2, p(jit), None, 6, 0)
    for call in (lambda: lib.pdc_gp_loglike(*head, None, None, None, 0),
                 lambda: lib.pdc_gp_loglike_dev(0, None, *head, None, None, None),
                 lambda: lib.pdc_gp_scan(*head, 3, 2, None, None, None, None, None, None, None, 0),
                 lambda: lib.pdc_gp_scan_dev(0, None, *head, 3, 2, None, None, None, None, None, None, None)):
        with pytest.raises(ValueError, match="every output is NULL"):
            _cabi.check(call())
    out = np.empty(6)
    for J in (0, 5):
        with pytest.raises(ValueError, match="1 <= J"):
            _cabi.check(lib.pdc_gp_loglike_dev(0, None, *head[:5], J, *head[6:], p(out), None, None))
    with pytest.raises(ValueError, match="np x nq must be M"):
        _cabi.check(lib.pdc_gp_scan_dev(0, None, *head, 4, 2, p(out), None, None, None, None, None, None))


def test_size_functions(monkeypatch):
    for name in ("pdc_gp_loglike", "pdc_gp_loglike_dev", "pdc_gp_scan", "pdc_gp_scan_dev", "pdc_gp_work_bytes",
                 "pdc_gp_max_terms", "pdc_gp_chunk_samples", "pdc_gp_last_dispatch"):
        assert name in _cabi.PROTOTYPES and hasattr(_cabi.lib(), name)
    assert _cabi.gp_max_terms() in (3, 4)
    assert 16 <= _cabi.gp_chunk_samples() <= 4096
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    small = _cabi.gp_work_bytes(1000, 4096, 2)
    assert small >= 1000 * 32 + 4096 * (2 * 32 + 16)                   # records, coefficients, likelihoods and means
    assert _cabi.gp_work_bytes(1000, 4096, 2, want_cube=True) == small - 4096 * 8
    assert _cabi.gp_work_bytes(2000, 4096, 2) >= small + 1000 * 32
    assert _cabi.gp_work_bytes(1000, 4096, 3) == small + 4096 * 32     # a term more: four coefficients a candidate
    for bad in ((0, 10, 1), (-1, 10, 1), (1 << 31, 10, 1), (10, 0, 1), (10, (1 << 40) + 1, 1), (10, 10, 0),
                (10, 10, _cabi.gp_max_terms() + 1)):
        assert _cabi.gp_work_bytes(*bad) == -1
    # a budget cuts the candidates into slabs: only the repacked coefficients shrink, never under one workgroup's
    big = (2000, 1 << 22, 4)
    free = _cabi.gp_work_bytes(*big)
    fixed = free - (1 << 22) * 128
    assert free > 1 << 29
    sizes = {}
    for gb in ("0.4", "0.2", "0.00001"):
        monkeypatch.setenv("PDC_WORK_BUDGET_GB", gb)
        sizes[gb] = _cabi.gp_work_bytes(*big)
    assert sizes["0.00001"] < sizes["0.2"] < sizes["0.4"] < free
    assert sizes["0.4"] <= 0.4 * (1 << 30) and sizes["0.2"] <= 0.2 * (1 << 30)
    assert sizes["0.00001"] == fixed + 64 * 128
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "1")
    assert _cabi.gp_work_bytes(1000, 4096, 2) == small                 # a call that fits is not touched
    monkeypatch.delenv("PDC_WORK_BUDGET_GB")
    assert _cabi.gp_work_bytes(*big) == free
    assert _cabi.gp_last_dispatch()[2] == 0 or _cabi.device_count() > 0   # zeros before the first call


# ---- the classes ---------------------------------------------------------------------------------------------------------
def _capture(monkeypatch):
    calls = []

    def loglike(t_rel, y, var, coeff, jitter=0.0, mean=None, fit_mean=False, device=None):
        calls.append(dict(t_rel=t_rel, y=y, var=var, coeff=coeff, jitter=jitter, mean=mean, fit_mean=fit_mean, device=device))
        M = coeff.shape[0]
        return np.arange(M, dtype=float), np.full(M, 0.25) if mean is None else np.asarray(mean, dtype=float), np.zeros(M, dtype=np.int32)

    def scan(t_rel, y, var, coeff, n_periods, jitter=0.0, mean=None, fit_mean=False, want_cube=False, device=None):
        calls.append(dict(t_rel=t_rel, y=y, var=var, coeff=coeff, n_periods=n_periods, jitter=jitter, mean=mean,
                          fit_mean=fit_mean, want_cube=want_cube, device=device))
        nq = coeff.shape[0] // n_periods
        cell = np.full(n_periods, nq - 1, dtype=np.int32)
        cell[0] = -1
        profile = np.linspace(1.0, 2.0, n_periods)
        profile[0] = np.nan
        return dict(profile=profile, cell=cell, marginal=profile - 1.0, mean=np.full(n_periods, 0.5),
                    cube=np.zeros((n_periods, nq)) if want_cube else None, best=(2.0, n_periods - 1, nq - 1))

    monkeypatch.setattr(_cabi, "gp_loglike", loglike)
    monkeypatch.setattr(_cabi, "gp_scan", scan)
    return calls


def test_unsorted_input_is_sorted_and_the_first_time_taken_off(monkeypatch):
    calls = _capture(monkeypatch)
    t = np.array([2450003.5, 2450001.0, 2450002.25, 2450001.0])
    y = np.array([30.0, 10.0, 20.0, 11.0])
    err = np.array([0.3, 0.1, 0.2, 0.11])
    like = gp.CeleriteLikelihood((t, y), err, device=3)
    assert like.t.tolist() == [2450001.0, 2450001.0, 2450002.25, 2450003.5] and like.y.tolist() == [10.0, 11.0, 20.0, 30.0]
    assert like.err.tolist() == [0.1, 0.11, 0.2, 0.3] and like.tau.tolist() == [0.0, 0.0, 1.25, 2.5]   # stable: 10 before 11
    assert np.array_equal(like.var, like.err ** 2) and isinstance(like.signal, TSeries)
    again = gp.CeleriteLikelihood(TSeries(t, y), np.sort(err))       # a TSeries is sorted already; err follows its order
    assert np.array_equal(again.tau, like.tau) and np.array_equal(again.y, like.y)
    terms = gp.rotation_terms(1.0, [3.0, 4.0], 1.0, 1.0, 0.5)
    res = like(terms, jitter=1e-3)                                   # mean None: profiled, on the centred curve
    c = calls[-1]
    assert c["fit_mean"] is True and c["mean"] is None and c["device"] == 3 and c["jitter"] == 1e-3
    assert np.array_equal(c["t_rel"], like.tau) and np.array_equal(c["y"], like.y - like.y.mean())
    assert np.array_equal(c["coeff"], go.to_device(terms))
    assert np.array_equal(res.mean, 0.25 + np.full(2, like.y.mean())) and res.status.dtype == np.int32
    res = like(terms, mean=12.5)                                     # one mean: taken off on the host
    assert calls[-1]["mean"] is None and calls[-1]["fit_mean"] is False and np.array_equal(calls[-1]["y"], like.y - 12.5)
    assert res.mean.tolist() == [12.5, 12.5]
    like(terms, mean=[1.0, 2.0])                                     # a mean per candidate: the kernel's
    assert calls[-1]["mean"].tolist() == [1.0, 2.0] and np.array_equal(calls[-1]["y"], like.y)
    with pytest.raises(ValueError):
        like(terms, mean=[1.0, 2.0, 3.0])
    for bad in (((t, y[:-1]), err), ((t, y), err[:-1]), ((t, np.where(y == 20.0, np.nan, y)), err), (TSeries(t, y), err[:2])):
        with pytest.raises(ValueError):
            gp.CeleriteLikelihood(*bad)
    assert np.array_equal(gp.CeleriteLikelihood(y).tau, np.arange(4.0))   # raw values: arange times, as everywhere


def test_scan_classes_build_the_grid_the_reference_names(monkeypatch):
    calls = _capture(monkeypatch)
    t, y, err = go.spot_curve(40)
    h = gp.HarmonicGP(TSeries(t, y), err)
    assert h.sigma == np.std(y) and h.jitter == np.min(err) ** 2 and h.names == ("Q0", "dQ", "f")   # the reference's defaults
    periods = np.array([2.0, 3.0, 4.5])
    s = h.scan(periods, Q0=[1.0, 5.0], dQ=[0.5], f=[0.2, 1.0], want_cube=True)
    c = calls[-1]
    assert c["n_periods"] == 3 and c["coeff"].shape == (12, 2, 4) and c["fit_mean"] is True and c["want_cube"] is True
    assert c["jitter"] == h.jitter and np.array_equal(c["y"], h.y - np.mean(h.y))
    cells = list(itertools.product([1.0, 5.0], [0.5], [0.2, 1.0]))
    want = go.to_device(np.array([go.rotation(h.sigma, p, *cell) for p in periods for cell in cells]))
    assert np.allclose(c["coeff"], want, rtol=1e-14, atol=0)
    assert np.array_equal(s.period, periods) and s.cube.shape == (3, 4) and np.isnan(s.log_likelihood[0])
    assert s.params(2) == dict(Q0=5.0, dQ=0.5, f=1.0) and all(np.isnan(v) for v in s.params(0).values())
    assert s.best["period"] == 4.5 and s.best["log_likelihood"] == 2.0 and s.best["Q0"] == 5.0 and s.best["f"] == 1.0
    assert s.best["sigma"] == h.sigma and s.best["jitter"] == h.jitter and s.best["mean"] == 0.5 + np.mean(h.y)
    assert np.array_equal(s.periodogram.frequency, 1 / periods[::-1]) and s.periodogram.values[0] == 2.0
    h.scan(periods, 1.0, 0.5, 0.2, sigma=0.3, jitter=0.0, fit_mean=False)
    assert calls[-1]["fit_mean"] is False and calls[-1]["coeff"].shape == (3, 2, 4)
    assert np.allclose(calls[-1]["coeff"][:, :, 0].sum(axis=1), 0.09)
    for bad in (dict(periods=[]), dict(periods=[-1.0]), dict(periods=[[2.0]]), dict(Q0=[]), dict(f=[np.nan]), dict(sigma=0.0),
                dict(jitter=-1.0), dict(Q0=np.ones(256), dQ=np.ones(256))):
        with pytest.raises(ValueError):
            h.scan(**{**dict(periods=periods, Q0=[1.0], dQ=[0.5], f=[0.2]), **bad})
    b = gp.BrownianGP(TSeries(t, y), err)
    assert b.names == ("tau", "mix")
    s = b.scan(periods, tau=[1.0, 3.0], mix=[0.1, 0.4], tau_in_periods=True)
    assert calls[-1]["coeff"].shape == (12, 3, 4)
    want = go.to_device(gp.brownian_terms(b.sigma, np.repeat(periods, 4) * np.tile([1.0, 1.0, 3.0, 3.0], 3),
                                          np.repeat(periods, 4), np.tile([0.1, 0.4], 6)))
    assert np.array_equal(calls[-1]["coeff"], want) and s.params(1) == dict(tau=3.0, mix=0.4)
    b.scan(periods, tau=[5.0], mix=[0.1])
    assert np.allclose(calls[-1]["coeff"][:, 1, 2], 1 / 5.0, rtol=1e-9)      # absolute tau
    with pytest.raises(ValueError):
        b.scan(periods, tau=[0.1], mix=[0.1])                               # overdamped at every period


def test_without_a_gpu_the_classes_raise_and_never_answer():
    t, y, err = go.spot_curve(40)
    terms = gp.rotation_terms(1.0, [3.0, 4.0], 1.0, 1.0, 0.5)
    calls = [lambda: gp.CeleriteLikelihood(TSeries(t, y), err)(terms),
             lambda: gp.HarmonicGP(TSeries(t, y), err).scan([3.0, 4.0], [1.0], [0.5], [0.2]),
             lambda: gp.BrownianGP(TSeries(t, y), err).scan([3.0, 4.0], [5.0], [0.2]),
             lambda: _cabi.gp_loglike(**_good())]
    if _cabi.device_count() == 0:
        for call in calls:
            with pytest.raises(RuntimeError):
                call()
    else:   # (with a GPU the same calls answer: tests/test_gp_gpu.py holds them to the oracle)
        assert all(np.all(np.isfinite(r.log_likelihood if hasattr(r, "log_likelihood") else r[0])) for r in (c() for c in calls))
