"""HTest and ZTest on the GPU (csrc/htest.hip through the classes and the C ABI) against the test-local oracle
(tests/htest_oracle.py: direct cos / sin per pair in float64, itself held to the 80-bit evaluation at 1e-11 by
tests/test_htest_host.py).  The reference has no such class - PARITY UNPINNED BY THE REFERENCE.

Gates.  Values: |got - exact| <= 1e-6 Z2 + 1e-9 (Tier E), for H with the bin's largest Z2_m, because H itself cancels to
about 0.  ``harmonics`` equals the oracle's wherever the oracle's best and second-best candidate are more than twice
that gate apart; at most 1 % of a case's bins may be left out (test_htest_host.py: none are, on these inputs).  Two
device paths that should agree to rounding: rtol 1e-9 (another tile phase), atol 1e-9 (Tier E's floor)."""
import ctypes as C
import functools

import numpy as np
import pytest

import htest_oracle as ho
from periodicity_amd import _cabi
from periodicity_amd.core import FSeries, TSeries
from periodicity_amd.spectral import GLS, HTest, ZTest

pytestmark = pytest.mark.gpu

SEEDS = ho.SEEDS                   # 64 / 65 straddle the 64-event chunk of the rotation tables
TOPS = (2, 4, 8, 12, 16, 20)       # the kernel instances: a call with nharm runs the smallest one that holds it
NHARMS = sorted({1} | set(TOPS) | {top + 1 for top in TOPS if top < 20})


@functools.lru_cache(maxsize=None)
def events(n):
    return ho.events(n, SEEDS[n])


def with_bins(n, nf, cls, **kw):
    """An explicit ``fmax`` that gives ``nf`` bins on the events of size ``n``."""
    t, _ = events(n)
    df = 1.0 / (t[-1] - t[0]) / 5
    return cls(fmax=0.5 * df + (nf - 1.5) * df, **kw)


@functools.lru_cache(maxsize=None)
def grid(n, nf=None):
    t, _ = events(n)
    if nf is None:
        return GLS()._grid(TSeries(t, np.ones_like(t)))
    freq = with_bins(n, nf, GLS)._grid(TSeries(t, np.ones_like(t)))
    assert freq.size == nf
    return freq


@functools.lru_cache(maxsize=None)
def exact(n, weighted, nf=None):
    """The oracle's cumulative Z2_m, m = 1 .. 20, of one list on one grid, evaluated once: fewer harmonics are its
    leading rows."""
    t, w = events(n)
    Z = ho.z2(t, w if weighted else None, grid(n, nf), 20)
    Z.setflags(write=False)
    return Z


def assert_meets_oracle(label, Z, h=None, m=None, z2=None):
    """``Z``: the oracle's rows 1 .. nharm."""
    gate = ho.gate(Z)
    h_exact, m_exact = ho.h_and_m(Z)
    for name, got, want in (("H", h, h_exact), ("Z2", z2, Z[-1])):
        if got is not None:
            err = np.abs(got - want)
            print(f"{label} {name}: bins {got.size} max |err| {err.max():.3e} max err/gate {np.max(err / gate):.3e}")
            assert np.all(err <= gate), (label, name, float(np.max(err / gate)))
    if m is not None:
        keep = ho.decided(Z)
        assert 1 - keep.mean() <= 0.01, (label, f"{100 * (1 - keep.mean()):.1f} % of the bins left out")
        assert m.dtype == np.int32 and np.array_equal(m[keep], m_exact[keep]), label
        assert np.all((m >= 1) & (m <= Z.shape[0])), label


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", list(SEEDS))
def test_parity_with_the_oracle(n, weighted):
    t, w = events(n)
    w = w if weighted else None
    for nharm in NHARMS:
        ht = HTest(max_harmonics=nharm)
        p = ht(TSeries(t, np.ones_like(t)), w)
        assert isinstance(p, FSeries) and np.array_equal(p.frequency, grid(n)) and ht.periodogram is p
        assert _cabi.htest_last_dispatch()[0] == min(top for top in TOPS if top >= nharm)
        assert ht.signal.size == n and (ht.weights is None if w is None else np.array_equal(ht.weights, w))
        assert_meets_oracle(f"parity N={n} nharm={nharm} weights={int(weighted)}", exact(n, weighted)[:nharm],
                            p.values, ht.harmonics, ht.z2.values)
        z = ZTest(nharm=nharm)(t, w)
        assert np.array_equal(z.values, ht.z2.values) and np.array_equal(z.frequency, grid(n))


@pytest.mark.parametrize("nharm", TOPS)
def test_tile_seams(nharm):
    """Grids one bin short of a tile, exactly a tile, and one bin over: every bin."""
    tile = _cabi.htest_tile_bins(nharm)
    t, w = events(200)
    for nf in (tile - 1, tile, tile + 1):
        ht = with_bins(200, nf, HTest, max_harmonics=nharm)
        p = ht(t, w)
        assert p.size == nf
        assert_meets_oracle(f"seam nf={nf} nharm={nharm}", exact(200, True, nf)[:nharm], p.values, ht.harmonics, ht.z2.values)


@pytest.mark.parametrize("nharm", [2, 20])
def test_sample_parts(nharm):
    """200 events are four chunks: three parts split them unevenly, seven leave parts empty."""
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    Z = exact(200, True)[:nharm]
    one = _cabi.htest_scan(t, w, f0, delta, nf, nharm, parts=1)
    for parts in (1, 2, 3, 7):
        h, m, z2 = _cabi.htest_scan(t, w, f0, delta, nf, nharm, parts=parts)
        assert _cabi.htest_last_dispatch()[2] == parts
        assert_meets_oracle(f"parts={parts} nharm={nharm}", Z, h, m, z2)
        np.testing.assert_allclose(h, one[0], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(z2, one[2], rtol=1e-9, atol=1e-9)
        again = _cabi.htest_scan(t, w, f0, delta, nf, nharm, parts=parts)
        assert all(np.array_equal(a, b) for a, b in zip((h, m, z2), again))


def test_parts_respect_the_workspace_budget(monkeypatch):
    """PDC_WORK_BUDGET_GB holds the records plus the partial sums: fewer parts, never an error.  658 bins at HT = 20 are
    210 560 B of partial sums per part beside 9 984 B of records: 0.0005 GB (536 870 B) has room for two parts."""
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    assert nf == 658
    two = _cabi.htest_scan(t, w, f0, delta, nf, 20, parts=2)
    one = _cabi.htest_scan(t, w, f0, delta, nf, 20, parts=1)
    for budget, ran, same in (("0.0005", 2, two), ("0.000001", 1, one)):
        monkeypatch.setenv("PDC_WORK_BUDGET_GB", budget)
        got = _cabi.htest_scan(t, w, f0, delta, nf, 20, parts=7)
        assert _cabi.htest_last_dispatch()[2] == ran
        assert all(np.array_equal(a, b) for a, b in zip(got, same))
    monkeypatch.delenv("PDC_WORK_BUDGET_GB")
    _cabi.htest_scan(t, w, f0, delta, nf, 20, parts=7)
    assert _cabi.htest_last_dispatch()[2] == 7


def test_automatic_parts():
    """The documented rule, parts = min(ceil(2 CUs / tiles), max(1, chunks / 8)), at 20 000 events (313 chunks) on one
    tile of bins: 39 parts on any device of 10 CUs or more."""
    n, nharm = 20_000, 4
    t, w = ho.events(n, 12)
    nf = _cabi.htest_tile_bins(nharm)
    f0, delta = 0.02, 0.3 / nf
    cus = _cabi.device_info(_cabi.default_device())["cu_count"]
    want = min(-(-2 * cus // 1), max(1, -(-n // 64) // 8))
    assert want > 1
    auto = _cabi.htest_scan(t, w, f0, delta, nf, nharm, parts=0)
    ht, k, ran = _cabi.htest_last_dispatch()
    assert (ht, ran) == (4, want) and k >= 1
    one = _cabi.htest_scan(t, w, f0, delta, nf, nharm, parts=1)
    assert _cabi.htest_last_dispatch()[2] == 1
    np.testing.assert_allclose(auto[0], one[0], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(auto[2], one[2], rtol=1e-9, atol=1e-9)
    assert np.mean(auto[1] != one[1]) <= 0.01                # (near-ties between candidates may fall either way)


@pytest.mark.parametrize("nharm", [1, 20])
def test_slab_of_the_grid_reproduces_the_full_call(nharm):
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    assert nf // 3 + 257 <= nf
    full = _cabi.htest_scan(t, w, f0, delta, nf, nharm)
    part = _cabi.htest_scan(t, w, f0, delta, 257, nharm, j_begin=nf // 3)
    for a, b in ((part[0], full[0]), (part[2], full[2])):
        np.testing.assert_allclose(a, b[nf // 3:nf // 3 + 257], rtol=1e-9, atol=1e-9)   # another tile phase: to rounding
    keep = ho.decided(exact(200, True)[:nharm])[nf // 3:nf // 3 + 257]
    assert np.array_equal(part[1][keep], full[1][nf // 3:nf // 3 + 257][keep])


def test_finds_a_pulsation():
    """35 % of 300 events in a pulse of 6 % of the period 7.3: the oracle's highest bin is at 7.3028 with m = 4,
    H about 109."""
    t, _ = ho.events(300, 11)
    ht = HTest(fmin=0.02, fmax=0.5)
    p = ht(t)
    peak = int(np.argmax(p.values))
    print(f"pulsation: HTest peak at period {1 / p.frequency[peak]:.4f}, H = {p.values[peak]:.2f}, m = {ht.harmonics[peak]}")
    assert abs(1 / p.frequency[peak] - 7.3) <= 0.01 * 7.3 and ht.harmonics[peak] >= 2
    assert HTest.fap(p.values[peak]) < 1e-15
    rayleigh = ZTest(fmin=0.02, fmax=0.5, nharm=1)(t)
    one = HTest(fmin=0.02, fmax=0.5, max_harmonics=1)
    one(t)
    assert np.array_equal(rayleigh.values, one.z2.values)
    assert np.array_equal(one.periodogram.values, one.z2.values) and np.all(one.harmonics == 1)


def test_against_the_exact_trig_sums():
    """Z2_m for m <= 4 rebuilt from the pinned exact-sum kernel (``pdc_trig_sums`` on the grids (k f0, k delta)).  Its own
    gate is 1e-9 sum |w| per sum; with |C|, |S| <= sum |w| that moves C**2 + S**2 by at most 4e-9 (sum |w|)**2 per
    harmonic, and twice that is allowed because both sides carry it."""
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    scale = 2 / np.sum(w * w)
    cum = np.zeros(nf)
    for m in (1, 2, 3, 4):
        S, Cc = _cabi.trig_sums(t, w, m * f0, m * delta, nf)
        cum = cum + (Cc * Cc + S * S)
        _, _, z2 = _cabi.htest_scan(t, w, f0, delta, nf, m, want=("z2",))
        bound = 8e-9 * m * scale * np.sum(np.abs(w)) ** 2
        err = np.max(np.abs(z2 - scale * cum))
        print(f"trig_sums m={m}: max |err| {err:.3e} bound {bound:.3e}")
        assert err <= bound


def test_class_conveniences():
    t, w = events(65)
    ht = HTest(max_harmonics=5)
    sorted_run = ht(t, w)
    harmonics = ht.harmonics
    order = np.random.default_rng(3).permutation(t.size)
    shuffled = HTest(max_harmonics=5)
    p = shuffled(t[order], w[order])                        # a raw array is the list of arrival times, in any order
    assert np.array_equal(p.values, sorted_run.values) and np.array_equal(shuffled.harmonics, harmonics)
    assert np.array_equal(shuffled.signal.time, t) and np.array_equal(shuffled.weights, w)
    assert np.array_equal(HTest(max_harmonics=5)(TSeries(t, np.arange(65.0)), w).values, sorted_run.values)   # values unused
    with pytest.raises(ValueError):
        ht(t, w[:-1])
    f0, delta, nf = _cabi.grid_params(grid(65))
    bad = t.copy()
    bad[-1] = np.nan                                        # a NaN event propagates, it is not an error
    h, m, z2 = _cabi.htest_scan(bad, w, f0, delta, nf, 5)
    assert np.all(np.isnan(h)) and np.all(np.isnan(z2)) and np.all(m == 1)
    assert _cabi.htest_scan(t, w, f0, delta, nf, 5, want=("m",))[0] is None


@pytest.mark.parametrize("parts", [1, 3])
def test_host_entry_and_dev_twin_are_bit_identical(parts):
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    host = _cabi.htest_scan(t, w, f0, delta, nf, 12, parts=parts)
    DB = _cabi.DeviceBuffer
    dev = _cabi.default_device()
    bt, bw, bh, bm, bz = DB.from_array(t, dev), DB.from_array(w, dev), DB(nf * 8, dev), DB(nf * 4, dev), DB(nf * 8, dev)
    try:
        _cabi.check(_cabi.lib().pdc_htest_scan_dev(dev, None, bt.ptr, bw.ptr, t.size, f0, delta, 0, nf, 12, parts, bh.ptr, bm.ptr,
                                                  bz.ptr))
        _cabi.check(_cabi.lib().pdc_device_sync(dev))
        twin = bh.to_array(np.float64, nf), bm.to_array(np.int32, nf), bz.to_array(np.float64, nf)
    finally:
        for b in (bt, bw, bh, bm, bz):
            b.free()
    assert all(np.array_equal(a, b) for a, b in zip(host, twin))


def test_hygiene_no_allocation_on_a_repeated_or_rejected_call():
    t, w = events(200)
    f0, delta, nf = _cabi.grid_params(grid(200))
    first = _cabi.htest_scan(t, w, f0, delta, nf, 20, parts=3)
    counts = _cabi.alloc_counts()
    again = _cabi.htest_scan(t, w, f0, delta, nf, 20, parts=3)
    assert _cabi.alloc_counts() == counts and all(np.array_equal(a, b) for a, b in zip(first, again))
    with pytest.raises(ValueError):
        _cabi.htest_scan(t, w, f0, delta, nf, 21)
    assert _cabi.alloc_counts() == counts
