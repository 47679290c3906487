"""EMD and CEEMDAN without a GPU: the oracle against the trajectories its literal evaluation was measured to give, its two
evaluations against each other, the knot rule against np.pad / np.delete, the classes' own logic with the ``_cabi`` entries
replaced by the oracle, and the C entries' refusals before any device is looked for.
PARITY UNPINNED BY THE REFERENCE (tests/emd_oracle.py)."""
import warnings

import numpy as np
import pytest

import emd_oracle as eo
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.decomposition import CEEMDAN, EMD, envelopes

TABLE = {
    "tones1000": (eo.tones(1000), [3, 280, 233, 28, 9, 16, 8]),
    "tones256": (eo.tones(256), [7, 298, 6, 4]),
    "noise64": (eo.noise(64, 1), [7, 28, 63, 8]),
    "noise257": (eo.noise(257, 2), [7, 15, 6, 8, 13, 4]),
    "noise1000": (eo.noise(1000, 3), [9, 19, 9, 14, 13, 9, 7, 3]),
    "mix": (eo.mix(), [33, 16, 75, 3, 1]),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_both_evaluations_follow_the_measured_trajectories(name):
    (t, x), sifts = TABLE[name]
    lit, ex = eo.emd(t, x, how="literal"), eo.emd(t, x, how="exact")
    assert lit[2] == sifts and ex[2] == sifts and lit[3] == ex[3] == 0
    # float64 against long double after up to 298 consecutive sifts: 5.6e-14 measured on amplitudes of 1 - 3
    for a, b in zip(lit[0] + [lit[1]], ex[0] + [ex[1]]):
        assert np.max(np.abs(a - b)) <= 1e-12
    assert np.max(np.abs(np.sum(lit[0], axis=0) + lit[1] - x)) <= (len(sifts) + 1) * 2.0 ** -53 * np.max(np.abs(x))


def test_the_long_row_of_the_table():
    t, x = eo.noise(4097, 5)
    modes, _, sifts, _ = eo.emd(t, x)
    assert len(modes) == 9 and sum(sifts) + len(sifts) == 169


@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_knot_rule_is_np_pad_and_np_delete(p):
    t, x = eo.mix()
    for idx in eo.extrema(x):
        kt, kv = eo.knots_reference(t, x, idx, p)
        rt, rv = eo.knots_rule(t, x, idx, p)
        assert kt.tobytes() == rt.tobytes() and kv.tobytes() == rv.tobytes()
        assert kt.size == idx.size + 2 * p and np.all(np.diff(kt) > 0)


# ---- the classes on the oracle ---------------------------------------------------------------------------------------------
def fake_emd_batch(t, x, max_iter=2000, pad_width=2, theta_1=0.05, theta_2=0.50, alpha=0.05, max_modes=64, device=None):
    B, n = x.shape
    out = {"modes": np.zeros((B, max_modes, n)), "residue": np.empty((B, n)), "n_modes": np.zeros(B, dtype=np.int64),
           "sifts": np.zeros((B, max_modes), dtype=np.int64), "flags": np.zeros(B, dtype=np.int64)}
    for b in range(B):
        modes, residue, sifts, flags = eo.emd(t, x[b], max_iter, pad_width, theta_1, theta_2, alpha, max_modes)
        out["n_modes"][b], out["flags"][b], out["residue"][b] = len(modes), flags, residue
        for k, m in enumerate(modes):
            out["modes"][b, k], out["sifts"][b, k] = m, sifts[k]
    return out


def fake_emd_sift(t, x, pad_width=2, device=None):
    s = eo.sift(t, x, pad_width)
    return {"upper": s.get("upper"), "lower": s.get("lower"), "maxima": s["M"], "minima": s["D"], "n_zero": s["n_zero"],
            "monotonic": s["monotonic"]}


class FakePlan:
    def __init__(self, t, noise, max_modes=64, device=None, **params):
        self.t, self.params = t, params
        self.out = fake_emd_batch(t, noise, max_modes=max_modes, **params)
        self.n_modes, self.sifts, self.flags = self.out["n_modes"], self.out["sifts"], self.out["flags"]
        self.closed = False

    def noise_mode(self, k):
        return self.out["modes"][:, k, :].copy()

    def stage(self, residue, k, beta):
        E = self.n_modes.size
        noisy = np.stack([residue + beta[e] * self.out["modes"][e, k] if self.n_modes[e] > k else residue.copy()
                          for e in range(E)])
        first = fake_emd_batch(self.t, noisy, max_modes=1, **self.params)
        mu = np.zeros(residue.size)
        for e in range(E):
            mu = mu + ((noisy[e] - first["modes"][e, 0]) if first["n_modes"][e] else noisy[e] - noisy[e]) / E
        return mu, first["n_modes"], first["sifts"][:, 0], first["flags"]

    def close(self):
        self.closed = True


@pytest.fixture
def on_the_oracle(monkeypatch):
    monkeypatch.setattr(_cabi, "emd_batch", fake_emd_batch)
    monkeypatch.setattr(_cabi, "emd_sift", fake_emd_sift)
    monkeypatch.setattr(_cabi, "CeemdanPlan", FakePlan)


def test_emd_class(on_the_oracle):
    (t, x), sifts = TABLE["mix"]
    emd = EMD()
    modes = emd(TSeries(t, x))
    want = eo.emd(t, x)
    assert emd.n_modes == len(modes) == 5 and emd.sifts == sifts and emd.signal.size == 300
    assert all(isinstance(m, TSeries) and np.array_equal(m.values, w) for m, w in zip(modes, want[0]))
    assert np.array_equal(emd.residue.values, want[1]) and np.array_equal(emd.residue.time, t)
    # an array gets time = arange(N)
    plain = EMD()(x)
    assert np.array_equal(plain[0].time, np.arange(300)) and len(plain) == len(eo.emd(np.arange(300.0), x)[0])
    rows = EMD().batch([TSeries(t, x), TSeries(t, -x)])
    assert len(rows) == 2 and np.array_equal(rows[0][0].values, want[0][0])
    with pytest.raises(ValueError):
        EMD().batch([TSeries(t, x), TSeries(t + 1.0, x)])
    with pytest.raises(ValueError):
        EMD()(x, max_modes=65)


def test_monotonic_input_and_short_input(on_the_oracle):
    x = np.exp(np.linspace(0, 1, 50))
    emd = EMD()
    assert emd(x) == [] and emd.n_modes == 0 and emd.residue.values.tobytes() == x.tobytes()
    calls = []
    _cabi.emd_batch = lambda *a, **k: calls.append(1)
    short = np.array([1.0, -1.0, 1.0])
    assert emd(short) == [] and emd.residue.values.tobytes() == short.tobytes() and not calls


def test_max_modes_warning(on_the_oracle, monkeypatch):
    (t, x), _ = TABLE["noise257"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert len(EMD()(TSeries(t, x), max_modes=2)) == 2   # a bound the caller set: no warning
    monkeypatch.setattr(_cabi, "EMD_MAX_MODES", 3)
    with pytest.warns(RuntimeWarning, match="3 modes"):
        assert len(EMD()(TSeries(t, x))) == 3


def test_envelopes(on_the_oracle):
    (t, x), _ = TABLE["noise64"]
    up, lo = envelopes(TSeries(t, x))
    M, D = eo.extrema(x)   # (pad_width = 0: beyond the outermost extrema the end polynomials go on)
    assert np.max(np.abs(up.values[M] - x[M])) <= 1e-14 and np.max(np.abs(lo.values[D] - x[D])) <= 1e-14
    inner = slice(max(M[0], D[0]), min(M[-1], D[-1]) + 1)
    assert np.all(up.values[inner] >= lo.values[inner])
    with pytest.raises(ValueError, match="padding"):
        envelopes(np.array([0.0, 1.0, 0.0, -1.0, 0.0]), pad_width=2)
    with pytest.raises(ValueError, match="interpolation"):
        envelopes(np.array([0.0, 1.0, 0.0, -1.0, 0.0]), pad_width=1)


def test_ceemdan_flow_postprocessing_and_orthogonality(on_the_oracle):
    t, x = eo.tones(256)
    ce = CEEMDAN(ensemble_size=4, random_seed=7, cores=3)
    imfs = ce(TSeries(t, x), progress=True)
    want, noise_traj, stages = eo.ceemdan(t, x, ensemble_size=4, random_seed=7)
    assert ce.n_modes == len(imfs) == len(want) >= 2
    assert all(np.array_equal(m.values, w) for m, w in zip(imfs, want))
    assert [int(v) for v in ce.noise_trajectories[0]] == [n for n, _ in noise_traj]
    assert len(ce.trajectories) == len(stages)
    for (n_first, sifts), stage in zip(ce.trajectories, stages):
        assert [(int(a), int(b)) for a, b in zip(n_first, sifts)] == stage
    assert np.array_equal(ce.residue.values, x - sum(want))
    ce.postprocessing()
    assert 1 <= len(ce.c_modes) <= ce.n_modes
    total = sum(m.values for m in ce.c_modes) + ce.c_residue.values
    assert np.max(np.abs(total - x)) <= 1e-12
    for orth in (ce.orthogonality_matrix, ce.c_orthogonality_matrix):
        assert np.array_equal(orth, orth.T) and np.array_equal(np.diag(orth), np.ones(len(orth)))
        assert np.all(np.abs(orth) <= 1 + 1e-12)
    assert len(CEEMDAN(ensemble_size=4, random_seed=7)(x, max_modes=1)) == 1


# ---- the C entries' refusals, before any device is looked for --------------------------------------------------------------
def good():
    t, x = eo.noise(32, 1)
    return dict(t=t, x=x[None, :])


@pytest.mark.parametrize("change, text", [
    (dict(x=np.array([[1.0, np.nan] + [0.0] * 30])), "not finite"),
    (dict(x=np.array([[1.0, np.inf] + [0.0] * 30])), "not finite"),
    (dict(t=np.r_[0.0, 0.0, np.arange(2.0, 32.0)]), "strictly increasing"),
    (dict(t=np.arange(32.0)[::-1].copy()), "strictly increasing"),
    (dict(pad_width=-1), "pad_width"),
    (dict(max_modes=0), "max_modes"),
    (dict(max_modes=65), "max_modes"),
    (dict(max_iter=0), "max_iter"),
    (dict(max_iter=1000001), "max_iter"),
    (dict(theta_1=np.nan), "finite"),
])
def test_refusals_come_before_any_device(change, text):
    kw = {**good(), **change}
    with pytest.raises(ValueError, match=text):
        _cabi.emd_batch(**kw, device=10 ** 6)


def test_sift_refusals_and_sizes():
    t, x = eo.noise(32, 1)
    with pytest.raises(ValueError, match="not finite"):
        _cabi.emd_sift(t, np.r_[np.nan, x[1:]], device=10 ** 6)
    with pytest.raises(ValueError, match="strictly increasing"):
        _cabi.emd_sift(np.zeros(32), x, device=10 ** 6)
    with pytest.raises(ValueError, match="pad_width"):
        _cabi.emd_sift(t, x, pad_width=-2, device=10 ** 6)
    cap = _cabi.emd_lds_samples()
    assert cap >= 4096
    # the LDS route needs no slab: eight bytes per row; the workspace route one slab per resident workgroup
    assert _cabi.emd_work_bytes(cap, 10) == 256 and _cabi.emd_work_bytes(cap + 1, 10) > 10 * 36 * cap
    assert _cabi.emd_work_bytes(0, 1) == -1 and _cabi.emd_work_bytes(100, 1, pad_width=-1) == -1
    if _cabi.device_count() == 0:
        with pytest.raises(RuntimeError):
            _cabi.emd_batch(t, x[None, :])
