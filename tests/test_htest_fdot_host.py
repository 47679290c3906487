"""HTest.search / ZTest.search without a GPU: the test-local oracle of the plane (tests/htest_fdot_oracle.py) against
itself in 80-bit arithmetic, the class interface, the C ABI's argument checks and the workspace rule.  PARITY UNPINNED BY
THE REFERENCE."""
import inspect

import numpy as np
import pytest

import htest_fdot_oracle as fo
import htest_oracle as ho
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.spectral import GLS, HTest, SpinSearch, ZTest


def default_grid(t):
    return GLS()._grid(TSeries(t, np.ones_like(t)))


def cases(n):
    """``(epoch name, epoch, cycles, fdot)`` of every (epoch, row) of the list of size ``n``."""
    t, _ = ho.events(n, ho.SEEDS[n])
    for which in fo.EPOCHS:
        epoch = fo.epoch_of(t, which)
        for c, fdot in zip(fo.CYCLES, fo.rows_of(t, epoch)):
            yield which, epoch, c, fdot


@pytest.mark.parametrize("n", list(ho.SEEDS))
def test_float64_and_longdouble_oracles_agree(n):
    """The float64 oracle is within 5 % of the Tier E gate of its 80-bit evaluation, first 300 bins, all 20 harmonics.
    The rows are defined by their drift in cycles: the error of the float64 phase is that of tau**2 at the farthest
    event times the drift, so it does not grow with the list's span."""
    t, w = ho.events(n, ho.SEEDS[n])
    freq = default_grid(t)[:300]
    worst = 0.0
    for which, epoch, c, fdot in cases(n):
        z64 = fo.z2_fdot(t, w, freq, fdot, epoch, 20, np.float64)
        z80 = fo.z2_fdot(t, w, freq, fdot, epoch, 20, np.longdouble)
        ratio = float(np.max(np.abs(z64 - z80) / ho.gate(z80)))
        worst = max(worst, ratio)
        assert ratio <= 0.05, (n, which, c, ratio)
    print(f"N={n}: float64 oracle within {100 * worst:.2f} % of the gate of the 80-bit one")


def test_the_row_without_drift_is_the_plain_oracle():
    t, w = ho.events(65, ho.SEEDS[65])
    freq = default_grid(t)
    np.testing.assert_allclose(fo.z2_fdot(t, w, freq, 0.0, t[0], 20), ho.z2(t, w, freq, 20), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n", list(ho.SEEDS))
def test_the_values_decide_the_harmonics_of_the_test_inputs(n):
    t, w = ho.events(n, ho.SEEDS[n])
    freq = default_grid(t)
    worst = 0.0
    for which, epoch, c, fdot in cases(n):
        for weights in (w, None):
            Z = fo.z2_fdot(t, weights, freq, fdot, epoch, 20)
            for M in (2, 3, 20):
                left_out = float(np.mean(~ho.decided(Z[:M])))
                worst = max(worst, left_out)
                assert left_out <= 0.01, (n, which, c, M, left_out)
    print(f"N={n}: at most {100 * worst:.2f} % of the bins left out")


def test_the_test_pulsar_is_found_by_the_oracle_only_with_its_spin_down():
    t, w = fo.pulsar(400, 7)
    df = 1.0 / (t[-1] - t[0]) / 5
    freq = np.arange(0.12, 0.155 + df, df)
    assert freq.size == 211
    rows = np.linspace(-1.6e-5, 0, 9)
    Z = np.stack([fo.z2_fdot(t, w, freq, fd, t[0] + 600, 20) for fd in rows])
    H = np.stack([ho.h_and_m(z)[0] for z in Z])
    row, j = np.unravel_index(np.argmax(H), H.shape)
    print(f"pulsar: H {H[row, j]:.1f} at row {row} bin {j} against {H[8].max():.1f} without spin-down; "
          f"Z2_2 {Z[:, 1].max():.1f} against {Z[8, 1].max():.1f}")
    assert (row, j) == (4, 102) and abs(freq[j] - 0.137) <= df and H[row, j] >= 2 * H[8].max()
    assert np.unravel_index(np.argmax(Z[:, 1]), H.shape) == (4, 102) and Z[4, 1].max() >= 2 * Z[8, 1].max()


def test_class_signature_and_validation(monkeypatch):
    for cls in (HTest, ZTest):
        sig = inspect.signature(cls.search)
        assert list(sig.parameters) == ["self", "signal", "weights", "fdot", "epoch", "want_plane"]
        assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("fdot", "epoch", "want_plane"))
        assert sig.parameters["fdot"].default is inspect.Parameter.empty
        assert sig.parameters["epoch"].default is None and sig.parameters["want_plane"].default is True
        assert sig.parameters["weights"].default is None
        assert list(inspect.signature(cls.__call__).parameters) == ["self", "signal", "weights"]   # untouched

    def no_library_call(*args, **kwargs):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_cabi, "htest_fdot_scan", no_library_call)
    t, w = ho.events(64, 3)
    ok = np.array([0.0, -1e-6])
    for cls in (HTest, ZTest):
        for call in (lambda: cls().search(t, w, fdot=[]), lambda: cls().search(t, w, fdot=[[0.0, 1e-6]]),
                     lambda: cls().search(t, w, fdot=[0.0, np.nan]), lambda: cls().search(t, w, fdot=[np.inf]),
                     lambda: cls().search(t, w, fdot=ok, epoch=np.nan), lambda: cls().search(t, w, fdot=ok, epoch=np.inf),
                     lambda: cls().search(t, w[:-1], fdot=ok), lambda: cls().search(t, w.reshape(8, 8), fdot=ok),
                     lambda: cls().search(t.reshape(8, 8), fdot=ok), lambda: cls().search(t[:1], fdot=ok)):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(TypeError):
            cls().search(t, w)                                   # fdot is required
        with pytest.raises(AssertionError, match="the library was called"):
            cls().search(t, w, fdot=ok)


def test_search_sorts_the_events_builds_the_grid_and_wraps_the_outputs(monkeypatch):
    seen = {}

    def record(t, w, f0, delta, nf, fdot, epoch, **kw):
        seen.update(t=t, w=w, f0=f0, delta=delta, nf=nf, fdot=fdot, epoch=epoch, **kw)
        nfd = len(fdot)
        out = dict.fromkeys(_cabi.FDOT_OUTPUTS)
        plane = np.arange(nfd * nf, dtype=float).reshape(nfd, nf)
        plane[:, 3] = np.nan
        for name in kw["want"]:
            out[name] = {"plane": plane, "m_plane": np.full((nfd, nf), 2, dtype=np.int32),
                         "ridge": np.where(np.arange(nf) == 3, np.nan, plane[-1]),
                         "ridge_row": np.where(np.arange(nf) == 3, -1, nfd - 1).astype(np.int32),
                         "ridge_m": np.where(np.arange(nf) == 3, -1, 2).astype(np.int32),
                         "best": (float(plane[-1, -1]), nf - 1, nfd - 1, 2)}[name]
        return out

    monkeypatch.setattr(_cabi, "htest_fdot_scan", record)
    t, w = ho.events(65, 4)
    order = np.random.default_rng(0).permutation(65)
    rows = np.array([1e-6, 0.0, -2e-6])
    h = HTest(n=3, max_harmonics=9)
    s = h.search(t[order], w[order], fdot=rows)
    assert isinstance(s, SpinSearch)
    assert np.array_equal(s.frequency, GLS(n=3)._grid(TSeries(t, np.ones(65)))) and np.array_equal(h.frequency, s.frequency)
    assert np.array_equal(seen["t"], t) and np.array_equal(seen["w"], w) and seen["epoch"] == t[0] and s.epoch == t[0]
    assert np.array_equal(seen["fdot"], rows) and np.array_equal(s.fdot, rows)            # any order, kept
    assert seen["nharm"] == 9 and seen["stat"] == "h" and set(seen["want"]) == set(_cabi.FDOT_OUTPUTS)
    assert (seen["f0"], seen["delta"], seen["nf"]) == _cabi.grid_params(s.frequency)
    assert s.plane.shape == (3, s.frequency.size) and s.harmonics.dtype == np.int32
    assert np.array_equal(s.ridge.frequency, s.frequency) and np.isnan(s.ridge.values[3])
    assert np.isnan(s.ridge_fdot[3]) and np.all(np.delete(s.ridge_fdot, 3) == rows[2]) and s.ridge_harmonics[0] == 2
    nf = s.frequency.size
    assert s.best == (s.frequency[-1], rows[2], float(3 * nf - 1), 2, nf - 1, 2)
    assert s.best.fdot_index == 2 and s.best.index == nf - 1 and s.best.harmonics == 2
    assert not hasattr(h, "periodogram")                       # a search is not a call
    z = ZTest(0.02, 0.3, nharm=3)
    s = z.search(TSeries(t, np.arange(65.0)), fdot=rows, epoch=t[0] + 7, want_plane=False)
    assert seen["w"] is None and seen["stat"] == "z2" and seen["nharm"] == 3 and seen["epoch"] == t[0] + 7
    assert set(seen["want"]) == {"ridge", "ridge_row", "best"}
    assert s.plane is None and s.harmonics is None and s.ridge_harmonics is None and s.best.harmonics == 3


def raw_scan(**kw):
    """``pdc_htest_fdot_scan`` itself, every argument by name."""
    t, w = ho.events(31, 7)
    a = dict(t=t, w=w, n=31, f0=0.01, delta=0.01, j_begin=0, nf=50, fdot=np.array([0.0, 1e-7]), nfd=2, epoch=t[0],
             nharm=20, stat=0, parts=0, plane=np.empty((2, 64)), m_plane=np.empty((2, 64), dtype=np.int32),
             ridge=np.empty(64), ridge_row=np.empty(64, dtype=np.int32), ridge_m=np.empty(64, dtype=np.int32),
             best=np.empty(1), best_at=np.empty(3, dtype=np.int64), device=0)
    a.update(kw)
    P = _cabi._ptr
    _cabi.check(_cabi.lib().pdc_htest_fdot_scan(
        P(a["t"]), P(a["w"]), a["n"], a["f0"], a["delta"], a["j_begin"], a["nf"], P(a["fdot"]), a["nfd"], a["epoch"],
        a["nharm"], a["stat"], a["parts"], P(a["plane"]), P(a["m_plane"]), P(a["ridge"]), P(a["ridge_row"]), P(a["ridge_m"]),
        P(a["best"]), P(a["best_at"]), a["device"]))


NO_OUTPUT = dict(plane=None, m_plane=None, ridge=None, ridge_row=None, ridge_m=None, best=None, best_at=None)
BAD = [dict(n=0), dict(n=-1), dict(nf=-1), dict(j_begin=-1), dict(nharm=0), dict(nharm=21), dict(parts=-1), dict(delta=0.0),
       dict(delta=-0.1), dict(delta=float("nan")), dict(delta=float("inf")), NO_OUTPUT, dict(nf=(1 << 31) * 1024),
       dict(t=None), dict(fdot=None), dict(nfd=0), dict(nfd=-3), dict(fdot=np.array([0.0, np.nan])),
       dict(fdot=np.array([-np.inf, 0.0])), dict(epoch=float("nan")), dict(epoch=float("inf")), dict(stat=2), dict(stat=-1),
       dict(stat=1), dict(stat=1, m_plane=None), dict(stat=1, ridge_m=None)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(b) if len(b) < 7 else "no_output" for b in BAD])
def test_the_library_rejects_bad_arguments_before_it_looks_for_a_device(bad):
    with pytest.raises(ValueError, match="htest"):
        raw_scan(device=10 ** 6, **bad)


def test_cabi_symbols_and_loud_failure_without_a_device():
    names = ("pdc_htest_fdot_scan", "pdc_htest_fdot_scan_dev", "pdc_htest_fdot_last_dispatch", "pdc_htest_fdot_work_bytes")
    assert all(s in _cabi.PROTOTYPES and hasattr(_cabi.lib(), s) for s in names)
    t, w = ho.events(31, 7)
    with pytest.raises(ValueError):
        _cabi.htest_fdot_scan(t, w[:-1], 0.01, 0.01, 50, [0.0], t[0])
    with pytest.raises(ValueError):
        _cabi.htest_fdot_scan(t, w, 0.01, 0.01, 50, [0.0], t[0], want=("plane", "power"))
    with pytest.raises(ValueError):
        _cabi.htest_fdot_scan(t, w, 0.01, 0.01, 50, [0.0], t[0], stat="h2")
    raw_scan(nf=0, device=10 ** 6)                             # nothing to do: OK without touching any device
    raw_scan(nf=0, device=10 ** 6, stat=1, m_plane=None, ridge_m=None)
    if _cabi.device_count() == 0:
        for call in (lambda: _cabi.htest_fdot_scan(t, w, 0.01, 0.01, 50, [0.0], t[0]),
                     lambda: HTest().search(t, w, fdot=[0.0]), lambda: ZTest().search(t, fdot=[0.0, 1e-7])):
            with pytest.raises(RuntimeError):                  # no GPU: loud, never a CPU answer
                call()


def test_work_bytes_follow_the_budget(monkeypatch):
    """Records 9 984 B + ridge state 16 640 + 2 x 8 448 B = 43 520 B; 2 049 bins at HT = 20 and two parts are 1 311 488 B of
    partial sums per row; without planes and with one part a row is its slabs, 16 640 + 8 448 B."""
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    wb = _cabi.htest_fdot_work_bytes
    fixed, row2, slabs = 43520, 1311488, 16640 + 8448
    assert wb(200, 2049, 7, 20, 2, True) == wb(200, 2049, 7, 20, 2, False) == fixed + 7 * row2
    assert wb(200, 2049, 7, 20, 1, True) == fixed and wb(200, 2049, 7, 20, 1, False) == fixed + 7 * slabs
    assert wb(200, 2049, 7, 2, 2, True) == fixed + 7 * 131328              # the instance of nharm = 2 holds 2 harmonics
    for parts in (0, 1, 2):                                                # an empty grid: the records alone, no planning
        for want_plane in (True, False):
            assert wb(200, 0, 7, 20, parts, want_plane) == 9984
    assert wb(200, 1, 7, 20, 0, True) > 9984 and wb(200, -1, 7, 20, 0, True) == -1
    assert wb(0, 2049, 7, 20, 2, True) == wb(200, 2049, 0, 20, 2, True) == wb(200, 2049, 7, 21, 2, True) == -1
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "1")                          # a budget it fits in changes nothing
    assert wb(200, 2049, 7, 20, 2, True) == fixed + 7 * row2
    for rows in (3, 1):                                                    # fewer rows per launch first
        monkeypatch.setenv("PDC_WORK_BUDGET_GB", repr((fixed + (rows + 0.5) * row2) / 2 ** 30))
        assert wb(200, 2049, 7, 20, 2, True) == fixed + rows * row2
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", repr((fixed + 0.5 * row2) / 2 ** 30))   # then fewer parts: one, with its slabs
    assert wb(200, 2049, 7, 20, 2, True) == fixed and wb(200, 2049, 7, 20, 2, False) == fixed + 7 * slabs
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", repr((fixed + 2.5 * slabs) / 2 ** 30))
    assert wb(200, 2049, 7, 20, 1, False) == fixed + 2 * slabs
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", "0.000001")                   # never an error, never below one row
    assert wb(200, 2049, 7, 20, 7, False) == fixed + slabs
