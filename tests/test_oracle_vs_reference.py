"""Pinning of the oracle against the reference's own outputs, bit for bit.  The expected arrays are
tests/golden/g10_reference_pins.npz, written by ``tests/golden/make_golden.py`` from the reference's
source executed verbatim (``oracle/refstub.py``); the inputs are regenerated here from the same seeds."""
import os

import numpy as np
import pytest

from oracle import scan_oracle as so
from periodicity_amd.core import FSeries


@pytest.fixture(scope="module")
def pins(golden_dir):
    with np.load(os.path.join(golden_dir, "g10_reference_pins.npz")) as z:
        return {k: z[k] for k in z.files}


def curve(n, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, n, n))
    dy = rng.uniform(0.05, 0.2, n)
    return t, 1 + 0.5 * np.sin(2 * np.pi * t / 17.0) + dy * rng.standard_normal(n), dy


def test_reference_tests_pass_through_the_stub(pins):
    # the reference's two known-answer tests, on what its own code returned through the stub - and the
    # oracle reproduces both of those outputs
    t0, ts = 2.5, 0.1
    freq = pins["known_grid_frequency"]
    assert freq[0] == (1 / t0) / 2 and np.round(freq[-1], 6) == (1 / ts) / 2
    assert float(pins["known_sine_period"]) == 10.0
    assert np.array_equal(so.gls_grid(np.arange(0, t0 + ts, ts), n=1)[0], freq)
    got_f, got_p = so.gls(np.arange(100), np.sin((np.arange(100) / 100) * 20 * np.pi))
    assert np.array_equal(got_f, pins["known_sine_frequency"]) and np.array_equal(got_p, pins["known_sine_power"])
    assert FSeries(got_f, got_p).period_at_highest_peak == 10.0


@pytest.mark.parametrize("kw", [dict(), dict(n=3.5), dict(fmin=0.01, fmax=0.4), dict(psd=True)])
@pytest.mark.parametrize("fit_mean", [True, False])
def test_gls_fft_path_matches_reference_bitwise(pins, kw, fit_mean):
    i = [dict(), dict(n=3.5), dict(fmin=0.01, fmax=0.4), dict(psd=True)].index(kw)
    t, y, dy = curve(700, 3)
    freq, power = so.gls(t, y, dy, fit_mean=fit_mean, **kw)
    assert np.array_equal(freq, pins[f"gls_frequency_{i}_fm{int(fit_mean)}"])
    assert np.array_equal(power, pins[f"gls_power_{i}_fm{int(fit_mean)}"])


def test_trig_sum_seam_matches_reference_bitwise(pins):
    t, y, dy = curve(500, 4)
    for tag, tt in (("t", t), ("shifted", t + 1234.5)):
        S2, C2 = so.trig_sum_fft(tt, dy, 0.001, 300, 0.0005)
        assert np.array_equal(pins["trig_S_" + tag], S2) and np.array_equal(pins["trig_C_" + tag], C2)


def test_phase_seams_match_reference_bitwise(pins):
    t, y, _ = curve(600, 5)
    freq, theta = so.pdm(t, y, nb=4, nc=3, n_periods=40)
    assert np.array_equal(freq, pins["pdm_frequency"]) and np.array_equal(theta, pins["pdm_theta"])
    m = so.stringlength_scale(y)
    for p, want in zip(pins["sl_periods"], pins["sl_ell"]):
        assert want == so.stringlength_one(t, m, float(p))
