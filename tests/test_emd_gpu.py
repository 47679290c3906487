"""EMD on the device against tests/emd_oracle.py: the scan alone, one sift, whole trajectories and modes, both storage
routes, placement in a batch.  PARITY UNPINNED BY THE REFERENCE (its TSeries needs xarray): what is pinned is parity with
the reference's own scipy / numpy calls (``literal``) and with the long-double evaluation of the same steps (``exact``).

The gate of every envelope, mode and residue: max|device - exact| <= 8 max(max|literal - exact|, 2^-53 max|x|) - the
reference's float64 recipe measured against long double in the same test is the yardstick; the 8 allows for another order
of elimination and is not a measured number.  Measured on one MI355X (profiles/r32_emd_parity.txt): the worst ratio
device/yardstick is 0.57 for an envelope and 1.27 for a mode (tones(256) cut at max_iter = 5), of the 8 allowed.

Precondition: the oracle's decisions are far from a tie on every parity input (every margin >= 1e-9), so that equal
trajectories can be asked for.  One exception is written down where it is made: on ``tones`` sample 0 is sin(0) = 0, after
the first update it holds rounding noise of either sign, and the sign-change margin is 1e-15 there whatever the evaluation;
literal, exact and the device agree on those trajectories all the same, and the other two margins are asserted.
"""
import functools

import numpy as np
import pytest

import emd_oracle as eo
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.decomposition import EMD, envelopes

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
TABLE = {   # the literal oracle's trajectories (tests/test_emd_host.py checks them without a GPU)
    "tones1000": [3, 280, 233, 28, 9, 16, 8],
    "tones256": [7, 298, 6, 4],
    "noise64": [7, 28, 63, 8],
    "noise257": [7, 15, 6, 8, 13, 4],
    "noise1000": [9, 19, 9, 14, 13, 9, 7, 3],
    "mix": [33, 16, 75, 3, 1],
}


@functools.lru_cache(maxsize=None)
def curve(name):
    if name == "mix":
        return eo.mix()
    if name.startswith("tones"):
        return eo.tones(int(name[5:]))
    n, _, seed = name[5:].partition("_")
    return eo.noise(int(n), {"64": 1, "257": 2, "1000": 3}.get(n, 0) if not seed else int(seed))


@functools.lru_cache(maxsize=None)
def oracle(name, how, max_iter=2000, max_modes=None):
    t, x = curve(name)
    margins = eo.Margins()
    out = eo.emd(t, x, max_iter=max_iter, max_modes=max_modes, how=how, margins=margins)
    return out + (margins,)


def assert_far_from_ties(name):
    m = oracle(name, "literal")[4]
    assert m.sigma >= 1e-9 and m.extremum >= 1e-9, (name, m.sigma, m.extremum)
    if not name.startswith("tones"):   # (the module docstring has the reason)
        assert m.sign >= 1e-9, (name, m.sign)


def ratio(device, literal, exact, top):
    yard = max(float(np.max(np.abs(literal - exact))), EPS * top)
    return float(np.max(np.abs(device - exact))) / yard


def check_decomposition(name, out, b, max_iter=2000, max_modes=None):
    """Row b of a device batch against the two oracles: trajectory equal, every mode and the residue inside the gate, the
    parts summing to the input."""
    t, x = curve(name)
    lit, ex = oracle(name, "literal", max_iter, max_modes), oracle(name, "exact", max_iter, max_modes)
    n_modes = int(out["n_modes"][b])
    assert n_modes == len(lit[0]) == len(ex[0]), name
    assert list(out["sifts"][b, :n_modes]) == lit[2] == ex[2], name
    assert int(out["flags"][b]) == lit[3], name
    top = float(np.max(np.abs(x)))
    parts = [out["modes"][b, k] for k in range(n_modes)] + [out["residue"][b]]
    worst = 0.0
    for k, part in enumerate(parts):
        r = ratio(part, (lit[0] + [lit[1]])[k], (ex[0] + [ex[1]])[k], top)
        print(f"PARITY {name} max_iter={max_iter} max_modes={max_modes} part {k}: {r:.3f} of the yardstick (8 allowed)")
        worst = max(worst, r)
    assert worst <= 8.0, (name, worst)
    defect = np.max(np.abs(np.sum(parts, axis=0) - x))
    assert defect <= (n_modes + 1) * EPS * top, (name, defect)


# ---- 1. the scan alone -----------------------------------------------------------------------------------------------------
def check_scan(t, x):
    got = _cabi.emd_sift(t, x, pad_width=2)
    M, D = eo.extrema(x)
    assert np.array_equal(got["maxima"], M) and np.array_equal(got["minima"], D)
    assert got["n_zero"] == eo.n_zero(x)
    assert got["monotonic"] == eo.is_monotonic(M, D, 2)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_scan_at_the_wave_and_workgroup_seams(n):
    check_scan(*eo.noise(n, n))


def test_scan_flat_tops_edge_plateaus_and_signed_zeros():
    t = np.arange(400, dtype=np.float64)
    x = np.round(np.sin(2 * np.pi * t / 37.0) + 0.3 * np.sin(2 * np.pi * t / 5.3), 1)
    x[:4] = x[4]          # plateaus that touch either edge are no extrema
    x[-5:] = x[-6]
    assert np.any(np.diff(eo.extrema(x)[0]) > 0) and np.any(x[1:] == x[:-1])
    check_scan(t, x)
    z = np.array([1.0, 0.0, -0.0, 0.0, -1.0, -0.0, 2.0, 0.0, 0.0, -0.0, 3.0, -3.0, 0.0, 1.0, -0.0, -0.0, 0.5])
    check_scan(np.arange(z.size, dtype=np.float64), z)


# ---- 2. one sift -------------------------------------------------------------------------------------------------------------
def two_and_two():
    t = np.arange(9, dtype=np.float64)
    return t, np.array([0.0, 1.0, -1.0, 2.0, -2.0, 0.5, 0.6, 0.7, 0.8])


@pytest.mark.parametrize("name", ["noise64", "noise257", "mix", "two_and_two"])
def test_one_sift_meets_the_envelope_gate(name):
    """Worst measured ratio: 0.57 of the yardstick (8 allowed)."""
    t, x = two_and_two() if name == "two_and_two" else curve(name)
    if name == "two_and_two":
        assert len(eo.extrema(x)[0]) == 2 and len(eo.extrema(x)[1]) == 2
    lit, ex = eo.sift(t, x, 2, "literal"), eo.sift(t, x, 2, "exact")
    got = _cabi.emd_sift(t, x, pad_width=2)
    assert not got["monotonic"]
    top = float(np.max(np.abs(x)))
    for env in ("upper", "lower"):
        r = ratio(got[env], lit[env], ex[env], top)
        print(f"PARITY sift {name} {env}: {r:.3f} of the yardstick (8 allowed)")
        assert r <= 8.0, (name, env, r)
    up, lo = envelopes(TSeries(t, x), pad_width=2)
    assert np.array_equal(up.values, got["upper"]) and np.array_equal(lo.values, got["lower"])


def test_one_maximum_is_monotonic():
    t = np.arange(9, dtype=np.float64)
    x = np.array([0.0, 1.0, -1.0, -1.5, -2.0, -1.0, 0.0, 1.0, 2.0])
    assert len(eo.extrema(x)[0]) == 1
    got = _cabi.emd_sift(t, x, pad_width=2)
    assert got["monotonic"] and got["upper"] is None
    with pytest.raises(ValueError):
        envelopes(TSeries(t, x), pad_width=2)


# ---- 3. trajectories and modes -------------------------------------------------------------------------------------------
def run(name, **kw):
    t, x = curve(name)
    return _cabi.emd_batch(t, x[None, :], **kw)


@pytest.mark.parametrize("name", list(TABLE))
def test_trajectories_and_modes(name):
    """Worst measured ratio of a mode or residue on the six inputs: 0.93 of the yardstick (8 allowed)."""
    assert_far_from_ties(name)
    assert oracle(name, "literal")[2] == TABLE[name]
    out = run(name)
    check_decomposition(name, out, 0)
    route, threads, rows, evals = _cabi.emd_last_dispatch()
    assert route == "lds" and rows == 1 and evals >= sum(TABLE[name]) + len(TABLE[name])


def test_max_iter_reached_sets_the_flag():
    out = run("tones256", max_iter=5)
    assert int(out["flags"][0]) & 1
    check_decomposition("tones256", out, 0, max_iter=5)


def test_max_modes_reached_sets_the_flag():
    out = run("tones256", max_modes=2)
    assert int(out["n_modes"][0]) == 2 and int(out["flags"][0]) & 2
    check_decomposition("tones256", out, 0, max_modes=2)


def test_the_class_returns_the_same_modes():
    t, x = curve("mix")
    emd = EMD()
    modes = emd(TSeries(t, x))
    out = run("mix")
    assert emd.n_modes == len(modes) == int(out["n_modes"][0]) and emd.sifts == TABLE["mix"]
    assert all(np.array_equal(m.values, out["modes"][0, k]) for k, m in enumerate(modes))
    assert np.array_equal(emd.residue.values, out["residue"][0])
    rows = EMD().batch(np.stack([curve("noise257")[1], curve("noise257")[1][::-1]]))
    assert len(rows) == 2 and len(rows[0]) == len(TABLE["noise257"])


# ---- 4. routes -----------------------------------------------------------------------------------------------------------
CAP = _cabi.emd_lds_samples()


@pytest.mark.parametrize("n", [CAP - 1, CAP, CAP + 1])
def test_either_side_of_the_lds_cap(n):
    name = f"noise{n}_{n}"
    assert_far_from_ties(name)
    out = run(name)
    assert _cabi.emd_last_dispatch()[0] == ("lds" if n <= CAP else "global")
    check_decomposition(name, out, 0)


def test_forced_global_route_gives_the_lds_bytes(monkeypatch):
    name = f"noise{CAP}_{CAP}"
    first = run(name)
    assert _cabi.emd_last_dispatch()[0] == "lds"
    monkeypatch.setenv("PDC_EMD_FORCE_GLOBAL", "1")
    second = run(name)
    assert _cabi.emd_last_dispatch()[0] == "global"
    for key in ("modes", "residue", "n_modes", "sifts", "flags"):
        assert first[key].tobytes() == second[key].tobytes(), key


# ---- 5. placement ----------------------------------------------------------------------------------------------------------
def test_a_rows_bytes_do_not_depend_on_its_place_or_the_call():
    t, x = curve("noise257")
    alone = _cabi.emd_batch(t, x[None, :])
    rows = np.random.default_rng(99).standard_normal((70, 257))
    for b in (0, 37, 69):
        rows[b] = x
    many = _cabi.emd_batch(t, rows)
    again = _cabi.emd_batch(t, rows)
    for key in ("modes", "residue", "n_modes", "sifts", "flags"):
        assert many[key].tobytes() == again[key].tobytes(), key
        for b in (0, 37, 69):
            assert many[key][b].tobytes() == alone[key][0].tobytes(), (key, b)
    assert int(many["n_modes"][5]) >= 1 and not np.array_equal(many["modes"][5, 0], many["modes"][0, 0])
