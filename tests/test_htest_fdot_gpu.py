"""HTest.search / ZTest.search on the GPU (csrc/htest_fdot.hip through the classes and the C ABI) against the test-local
oracle of the plane (tests/htest_fdot_oracle.py: direct cos / sin of the whole phase per pair in float64, itself held to
5 % of the gate by its 80-bit evaluation in tests/test_htest_fdot_host.py).  PARITY UNPINNED BY THE REFERENCE.

Gates, as tests/test_htest_gpu.py.  Values: |got - exact| <= 1e-6 Z2 + 1e-9 (Tier E) with the bin's largest Z2_m.
``harmonics`` equals the oracle's wherever the oracle's best and second-best candidate are more than twice that gate apart;
at most 1 % of a case's bins may be left out.  Everything that should be the same computation is compared bit for bit."""
import functools

import numpy as np
import pytest

import htest_fdot_oracle as fo
import htest_oracle as ho
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.spectral import GLS, HTest, SpinSearch, ZTest

pytestmark = pytest.mark.gpu

TOPS = (2, 4, 8, 12, 16, 20)       # the kernel instances
ALL = _cabi.FDOT_OUTPUTS


@functools.lru_cache(maxsize=None)
def events(n):
    return ho.events(n, ho.SEEDS[n])


def with_bins(n, nf, cls, **kw):
    """An explicit ``fmax`` that gives ``nf`` bins on the events of size ``n``."""
    t, _ = events(n)
    df = 1.0 / (t[-1] - t[0]) / 5
    return cls(fmax=0.5 * df + (nf - 1.5) * df, **kw)


@functools.lru_cache(maxsize=None)
def grid(n, nf=None):
    t, _ = events(n)
    freq = (GLS() if nf is None else with_bins(n, nf, GLS))._grid(TSeries(t, np.ones_like(t)))
    assert nf is None or freq.size == nf
    return freq


@functools.lru_cache(maxsize=None)
def rows(n, which, cycles=fo.CYCLES):
    t, _ = events(n)
    return fo.rows_of(t, fo.epoch_of(t, which), cycles)


@functools.lru_cache(maxsize=None)
def exact(n, weighted, which, nf=None, cycles=fo.CYCLES):
    """The oracle's cumulative Z2_m, m = 1 .. 20, ``[rows][20][nf]``, evaluated once: fewer harmonics are leading rows."""
    t, w = events(n)
    epoch = fo.epoch_of(t, which)
    Z = np.stack([fo.z2_fdot(t, w if weighted else None, grid(n, nf), fd, epoch, 20) for fd in rows(n, which, cycles)])
    Z.setflags(write=False)
    return Z


def assert_meets_oracle(label, Z, h=None, m=None, z2=None):
    """One row of the plane; ``Z``: the oracle's rows 1 .. nharm.  Returns the worst error over its gate."""
    gate = ho.gate(Z)
    h_exact, m_exact = ho.h_and_m(Z)
    worst = 0.0
    for name, got, want in (("H", h, h_exact), ("Z2", z2, Z[-1])):
        if got is not None:
            err = np.abs(got - want)
            worst = max(worst, float(np.max(err / gate)))
            assert np.all(err <= gate), (label, name, float(np.max(err / gate)))
    if m is not None:
        keep = ho.decided(Z)
        assert 1 - keep.mean() <= 0.01, (label, f"{100 * (1 - keep.mean()):.1f} % of the bins left out")
        assert m.dtype == np.int32 and np.array_equal(m[keep], m_exact[keep]), label
        assert np.all((m >= 1) & (m <= Z.shape[0])), label
    return worst


def scan(n, which, fdot, nharm, *, weighted=True, nf=None, stat="h", parts=0, want=ALL):
    t, w = events(n)
    f0, delta, nbins = _cabi.grid_params(grid(n, nf))
    return _cabi.htest_fdot_scan(t, w if weighted else None, f0, delta, nbins, fdot, fo.epoch_of(t, which), nharm=nharm,
                                 stat=stat, parts=parts, want=want)


def same(a, b):
    """Bit for bit (NaN equals NaN); an output that was not asked for is None on both sides."""
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", list(ho.SEEDS))
def test_parity_with_the_oracle(n, weighted):
    t, w = events(n)
    w = w if weighted else None
    for which in fo.EPOCHS:
        epoch, fdot, Z = fo.epoch_of(t, which), rows(n, which), exact(n, weighted, which)
        worst = 0.0
        for nharm in (1, 2, 3, 20):
            s = HTest(max_harmonics=nharm).search(TSeries(t, np.ones_like(t)), w, fdot=fdot, epoch=epoch)
            assert isinstance(s, SpinSearch) and np.array_equal(s.frequency, grid(n)) and isinstance(s.ridge, FSeries)
            assert _cabi.htest_fdot_last_dispatch()[0] == min(top for top in TOPS if top >= nharm)
            z = scan(n, which, fdot, nharm, weighted=weighted, stat="z2", want=("plane",))["plane"]
            for r, c in enumerate(fo.CYCLES):
                worst = max(worst, assert_meets_oracle(f"parity N={n} {which} c={c} nharm={nharm} weights={int(weighted)}",
                                                       Z[r, :nharm], s.plane[r], s.harmonics[r], z[r]))
            if nharm <= 2:
                sz = ZTest(nharm=nharm).search(t, w, fdot=fdot, epoch=epoch)
                assert same(sz.plane, z) and sz.harmonics is None and sz.ridge_harmonics is None
                assert sz.best.harmonics == nharm and sz.best.value == np.nanmax(z)
        print(f"parity N={n} weights={int(weighted)} epoch={which}: worst err/gate {worst:.3e}")


@pytest.mark.parametrize("nharm", TOPS)
def test_tile_seams(nharm):
    """Grids one bin short of a tile, exactly a tile, and one bin over: every bin of both rows."""
    tile = _cabi.htest_tile_bins(nharm)
    assert tile == 1024
    cycles = (0.0, 2.0)
    Z = exact(65, True, "middle", tile + 1, cycles)
    worst = 0.0
    for nf in (tile - 1, tile, tile + 1):
        assert np.array_equal(grid(65, nf), grid(65, tile + 1)[:nf])
        out = scan(65, "middle", rows(65, "middle", cycles), nharm, nf=nf)
        zz = scan(65, "middle", rows(65, "middle", cycles), nharm, nf=nf, stat="z2", want=("plane",))["plane"]
        ht, k, parts, per_launch, launches = _cabi.htest_fdot_last_dispatch()
        assert (ht, k * (256 if ht <= 12 else 512), per_launch, launches) == (nharm, tile, 2, 1)
        for r in range(2):
            worst = max(worst, assert_meets_oracle(f"seam nf={nf} nharm={nharm} row={r}", Z[r, :nharm, :nf], out["plane"][r],
                                                   out["m_plane"][r], zz[r]))
    print(f"seams nharm={nharm}: worst err/gate {worst:.3e}")


@pytest.mark.parametrize("nharm", [2, 20])
def test_sample_parts(nharm):
    """200 events are four chunks: three parts split them unevenly, seven leave parts empty.  The row without drift is
    the plain scan with the same parts, bit for bit, whatever the epoch."""
    cycles = (2.0, 0.0, -4.5)
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    worst = 0.0
    for which in fo.EPOCHS:
        Z = exact(200, True, which, None, cycles)
        fdot = rows(200, which, cycles)
        for parts in (1, 2, 3, 7):
            out = scan(200, which, fdot, nharm, parts=parts)
            assert _cabi.htest_fdot_last_dispatch()[2:] == (parts, 3, 1)
            zz = scan(200, which, fdot, nharm, parts=parts, stat="z2", want=("plane",))["plane"]
            for r in range(3):
                worst = max(worst, assert_meets_oracle(f"parts={parts} nharm={nharm} {which} row={r}", Z[r, :nharm],
                                                       out["plane"][r], out["m_plane"][r], zz[r]))
            h, m, z2 = _cabi.htest_scan(t, w, f0, delta, nf, nharm, parts=parts)
            assert np.array_equal(out["plane"][1], h) and np.array_equal(out["m_plane"][1], m) and np.array_equal(zz[1], z2)
            again = scan(200, which, fdot, nharm, parts=parts)
            assert all(same(out[name], again[name]) for name in ALL if name != "best") and out["best"] == again["best"]
    print(f"parts nharm={nharm}: worst err/gate {worst:.3e}")


def reduce_like_numpy(plane, m_plane):
    """``(ridge, ridge_row, ridge_m, best)`` of a plane with at least one finite value per bin."""
    row = np.nanargmax(plane, axis=0)
    ridge = np.take_along_axis(plane, row[None], 0)[0]
    ridge_m = None if m_plane is None else np.take_along_axis(m_plane, row[None], 0)[0]
    j = int(np.nanargmax(ridge))
    return ridge, row, ridge_m, (float(ridge[j]), j, int(row[j]), None if ridge_m is None else int(ridge_m[j]))


@pytest.mark.parametrize("parts", [1, 3])
def test_ridge_and_best_cell(parts):
    """Five rows, two of them given twice: equal maxima, of which the lowest row must win."""
    cycles = (2.0, 0.0, 2.0, -4.5, 0.0)
    fdot = rows(200, "middle", cycles)
    for stat, nharm in (("h", 20), ("z2", 2)):
        out = scan(200, "middle", fdot, nharm, nf=1025, parts=parts, stat=stat)
        assert _cabi.htest_fdot_last_dispatch()[2:] == (parts, 5, 1)
        assert same(out["plane"][0], out["plane"][2]) and same(out["plane"][1], out["plane"][4])
        ridge, row, ridge_m, best = reduce_like_numpy(out["plane"], out["m_plane"])
        assert set(np.unique(row)) <= {0, 1, 3} and len(np.unique(row)) > 1
        assert np.array_equal(out["ridge"], ridge) and np.array_equal(out["ridge_row"], row) and out["ridge_row"].dtype == np.int32
        if stat == "h":
            assert np.array_equal(out["ridge_m"], ridge_m) and out["best"] == best
        else:
            assert out["ridge_m"] is None and out["m_plane"] is None and out["best"] == best[:3] + (nharm,)
        lean = scan(200, "middle", fdot, nharm, nf=1025, parts=parts, stat=stat, want=("ridge", "ridge_row", "ridge_m", "best"))
        assert lean["plane"] is None and lean["m_plane"] is None
        assert all(same(lean[name], out[name]) for name in ("ridge", "ridge_row", "ridge_m")) and lean["best"] == out["best"]
        only_best = scan(200, "middle", fdot, nharm, nf=1025, parts=parts, stat=stat, want=("best",))
        assert only_best["best"] == out["best"] and only_best["ridge"] is None
    t, w = events(200)
    s = with_bins(200, 1025, HTest).search(t, w, fdot=fdot, epoch=fo.epoch_of(t, "middle"), want_plane=False)
    assert s.plane is None and s.harmonics is None and np.array_equal(s.ridge_fdot, fdot[s.ridge_index])
    assert s.best.value == s.ridge.values[s.best.index] == np.max(s.ridge.values) and s.best.fdot == fdot[s.best.fdot_index]
    assert s.best.frequency == s.frequency[s.best.index] and s.best.harmonics == s.ridge_harmonics[s.best.index]


# What a row of a launch costs in workspace, each as a function of the library's own size query (200 events x 2049 bins,
# 7 rows, HT = 20): "partials" with two parts; with one part the slabs of what the caller does not take, "slabs" without
# any plane, "m_slab" with the plane of H taken and m left to the slab (the one size the query does not give: int32 per
# bin, rounded up to 256 B like every part of the workspace).  With one part and BOTH planes taken a row costs no
# workspace and no budget can cut the launch, which is why "one part, with a plane" takes the plane of H alone.
LEAN = ("ridge", "ridge_row", "ridge_m", "best")
SLAB_CASES = [(2, ALL, "partials", 3), (2, LEAN, "partials", 3), (1, ("plane",) + LEAN, "m_slab", 2), (1, LEAN, "slabs", 2)]


def budget_for(rows_per_launch, cost):
    """``PDC_WORK_BUDGET_GB`` with room for ``rows_per_launch`` and a half rows of ``cost``; call it without a budget set."""
    wb = _cabi.htest_fdot_work_bytes
    fixed = wb(200, 2049, 7, 20, 1, True)
    per_row = {"partials": (wb(200, 2049, 7, 20, 2, True) - fixed) // 7, "slabs": (wb(200, 2049, 7, 20, 1, False) - fixed) // 7,
               "m_slab": -(-2049 * 4 // 256) * 256}[cost]
    assert per_row > 0
    return repr((fixed + (rows_per_launch + 0.5) * per_row) / 2 ** 30)


@pytest.mark.parametrize("parts,want,cost,per_launch", SLAB_CASES, ids=["2-plane", "2-lean", "1-plane", "1-lean"])
def test_row_slabs_under_a_budget(monkeypatch, parts, want, cost, per_launch):
    """PDC_WORK_BUDGET_GB cuts the seven rows into launches; the ridge carries across them: no bit changes."""
    fdot = rows(200, "before", (2.0, 0.0, -4.5, 1.0, 2.0, -1.0, 0.5))
    monkeypatch.delenv("PDC_WORK_BUDGET_GB", raising=False)
    free = scan(200, "before", fdot, 20, nf=2049, parts=parts, want=want)
    assert _cabi.htest_fdot_last_dispatch()[2:] == (parts, 7, 1)
    monkeypatch.setenv("PDC_WORK_BUDGET_GB", budget_for(per_launch, cost))
    held = scan(200, "before", fdot, 20, nf=2049, parts=parts, want=want)
    assert _cabi.htest_fdot_last_dispatch()[2:] == (parts, per_launch, -(-7 // per_launch)) and per_launch < 7
    assert all(same(free[name], held[name]) for name in ALL if name != "best") and free["best"] == held["best"]
    if "plane" in want:
        ridge, row, _, best = reduce_like_numpy(held["plane"], None)
        assert np.array_equal(held["ridge"], ridge) and np.array_equal(held["ridge_row"], row) and held["best"][:3] == best[:3]


def test_nan_weights_and_nan_rows():
    t, w = events(65)
    f0, delta, nf = _cabi.grid_params(grid(65))
    bad = w.copy()
    bad[17] = np.nan
    fdot = rows(65, "first")
    for parts in (1, 2):
        out = _cabi.htest_fdot_scan(t, bad, f0, delta, nf, fdot, t[0], nharm=5, parts=parts)
        assert np.all(np.isnan(out["plane"])) and np.all(np.isnan(out["ridge"]))
        assert np.all(out["ridge_row"] == -1) and np.all(out["ridge_m"] == -1)
        assert np.isnan(out["best"][0]) and out["best"][1:] == (-1, -1, -1)
    s = HTest(max_harmonics=5).search(t, bad, fdot=fdot)
    assert np.all(np.isnan(s.ridge_fdot)) and np.isnan(s.best.frequency) and np.isnan(s.best.fdot) and np.isnan(s.best.value)
    assert (s.best.harmonics, s.best.index, s.best.fdot_index) == (-1, -1, -1)
    for poison in (np.nan, np.inf):
        rows_bad = fdot.copy()
        rows_bad[2] = poison
        with pytest.raises(ValueError, match="fdot"):
            _cabi.htest_fdot_scan(t, w, f0, delta, nf, rows_bad, t[0], nharm=5)


@pytest.mark.parametrize("cls,kw", [(HTest, dict(max_harmonics=20)), (ZTest, dict(nharm=2))], ids=["HTest", "ZTest"])
def test_recovers_a_spinning_down_pulsar(cls, kw):
    """Half of 400 events in a pulse of 5 % of a cycle at f = 0.137, fdot = -8e-6 over a span of 1200: the drift at the
    ends is 1.44 cycles and the scan of the frequency alone loses the pulse.  The numpy oracle gives H = 333.8 against
    66.2 in the row without spin-down, Z2_2 = 269.5 against 56.7, at bin 102 (tests/test_htest_fdot_host.py)."""
    t, w = fo.pulsar(400, 7)
    df = 1.0 / (t[-1] - t[0]) / 5
    frequency = np.arange(0.12, 0.155 + df, df)
    assert frequency.size == 211
    fdot = np.linspace(-1.6e-5, 0, 9)
    s = cls(fmin=0.12, fmax=0.155, **kw).search(t, w, fdot=fdot, epoch=t[0] + 600)
    assert np.array_equal(s.frequency, frequency) and s.plane.shape == (9, 211)
    print(f"pulsar {cls.__name__}: {s.best}, without spin-down {np.max(s.plane[8]):.1f}")
    assert s.best.fdot_index == 4 and s.best.fdot == fdot[4]
    assert abs(s.best.frequency - 0.137) <= df
    assert s.best.value >= 2 * np.max(s.plane[8])


@pytest.mark.parametrize("parts", [1, 3])
def test_host_entry_and_dev_twin_are_bit_identical(parts):
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    fdot = rows(200, "middle")
    epoch = fo.epoch_of(t, "middle")
    host = _cabi.htest_fdot_scan(t, w, f0, delta, nf, fdot, epoch, nharm=12, parts=parts)
    DB = _cabi.DeviceBuffer
    dev = _cabi.default_device()
    cells = fdot.size * nf
    bt, bw, bf = DB.from_array(t, dev), DB.from_array(w, dev), DB.from_array(fdot, dev)
    outs = [DB(cells * 8, dev), DB(cells * 4, dev), DB(nf * 8, dev), DB(nf * 4, dev), DB(nf * 4, dev), DB(8, dev), DB(24, dev)]
    try:
        _cabi.check(_cabi.lib().pdc_htest_fdot_scan_dev(dev, None, bt.ptr, bw.ptr, t.size, f0, delta, 0, nf, bf.ptr, fdot.size,
                                                       epoch, 12, 0, parts, *[b.ptr for b in outs]))
        _cabi.check(_cabi.lib().pdc_device_sync(dev))
        twin = [b.to_array(dtype, count) for b, dtype, count in zip(
            outs, (np.float64, np.int32, np.float64, np.int32, np.int32, np.float64, np.int64), (cells, cells, nf, nf, nf, 1, 3))]
    finally:
        for b in [bt, bw, bf] + outs:
            b.free()
    assert same(host["plane"].ravel(), twin[0]) and same(host["m_plane"].ravel(), twin[1])
    assert same(host["ridge"], twin[2]) and same(host["ridge_row"], twin[3]) and same(host["ridge_m"], twin[4])
    assert host["best"] == (float(twin[5][0]),) + tuple(int(v) for v in twin[6])


def test_hygiene_no_allocation_on_a_repeated_or_rejected_call():
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    fdot = rows(200, "middle")
    first = _cabi.htest_fdot_scan(t, w, f0, delta, nf, fdot, t[0], nharm=20, parts=3)
    counts = _cabi.alloc_counts()
    again = _cabi.htest_fdot_scan(t, w, f0, delta, nf, fdot, t[0], nharm=20, parts=3)
    assert _cabi.alloc_counts() == counts and all(same(first[name], again[name]) for name in ALL if name != "best")
    for bad in (dict(nharm=21), dict(fdot=np.array([0.0, np.nan])), dict(epoch=np.nan)):
        args = dict(fdot=fdot, epoch=t[0], nharm=20)
        args.update(bad)
        with pytest.raises(ValueError):
            _cabi.htest_fdot_scan(t, w, f0, delta, nf, **args)
    assert _cabi.alloc_counts() == counts
