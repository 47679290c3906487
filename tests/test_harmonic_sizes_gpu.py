"""The four harmonic-sum scans on the GPU - csrc/mhgls.hip, mbgls.hip, htest.hip and htest_fdot.hip through the C ABI with
explicit (f0, delta, nf) - against their test-local numpy oracles at the sizes the other test files do not reach
(tests/harmonic_sizes.py holds the inputs, grids, oracle values and rules; tests/test_harmonic_sizes_host.py pins those
oracles to 80 bits and counts the bins each shape leaves out).  PARITY UNPINNED BY THE REFERENCE.

What the shapes are for:
  prologue trips   the 1024-thread prologues of mhgls and htest walk ``i = tid; i < n + 2; i += 1024``: at 1022 samples the
                   two read-ahead records are written in the first trip, at 1023 one in each, at 1024 both in the second;
                   2049 and 4097 take three and five trips and feed ``block_sum`` more than one term per thread.
  segment walk     the prologue of mbgls places every record: 16 waves, a segment of roundup64(ceil(n / 16)) samples each,
                   walked four 64-sample groups per trip.  1024, 1025, 4096, 4097 and 8193 samples give segments of 64,
                   128, 256, 320 and 576: live second to fourth groups, a second and a third trip, the running place carried
                   across trips, and last trips with dead groups; hand-made label layouts; 32 bands; an empty band.
  wide grid        9217 bins: more than eight tiles, where the XCD tile order of mhgls and mbgls stops being the identity.
  one size up      20 000 samples (313 chunks, automatic sample parts for htest) on 128 picked bins.
  1e6 cycles       300 samples over 3000 d searched at a period of 0.0031 d, 300 events over 1e5 s at 10.0123 Hz: the exact
                   phase reduction of put_record and the rotation tables.
  stale workspace  the `_dev` forms read nothing a previous call left in the per-stream scratch block.

Gates: those of the four families' own GPU tests - |got - exact| <= 1e-6 |exact| + 1e-9 on bins with cond(M) <= 1e6 plus
the argmax over them; ``htest_oracle.gate`` for H and Z2, ``harmonics`` where the oracle's candidates decide it; at most
5 % / 1 % of a case's bins left out.  Grids are 1025 bins (257 for the 200-sample curve) centred on the signal: they
straddle the seams of the 512- and the 1024-frequency tiles."""
import ctypes as C

import numpy as np
import pytest

import harmonic_sizes as hs
from periodicity_amd import _cabi

pytestmark = pytest.mark.gpu

DB = _cabi.DeviceBuffer


def same(a, b):
    """Bit for bit (NaN equals NaN)."""
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def group(name, worst):
    print(f"GROUP {name}: worst err/gate {worst:.3e}")


# ---- prologue trips -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_err", [True, False])
@pytest.mark.parametrize("fit_mean", [True, False])
@pytest.mark.parametrize("nterms", [1, 4])
@pytest.mark.parametrize("n", hs.TRIPS)
def test_prologue_trips_mhgls(n, nterms, fit_mean, with_err):
    t, y, err = hs.mh_curve(n)
    got = _cabi.mhgls_scan(t, y, err if with_err else None, *hs.mh_grid(n), nterms, fit_mean)
    exact, keep = hs.mh_oracle(n, nterms, with_err, fit_mean)
    group("trips mhgls", hs.assert_gls(f"mhgls N={n} nterms={nterms} fit_mean={int(fit_mean)} err={int(with_err)}", got, exact, keep))


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("nharm", [2, 20])      # 256 and 512 threads
@pytest.mark.parametrize("n", hs.TRIPS)
def test_prologue_trips_htest(n, nharm, weighted, parts):
    t, w = hs.ht_events(n)
    h, m, z2 = _cabi.htest_scan(t, w if weighted else None, *hs.ht_grid(n), nharm, parts=parts)
    assert _cabi.htest_last_dispatch() == (nharm, 4 if nharm == 2 else 2, parts)
    Z = hs.ht_exact(n, weighted)[:nharm]
    group("trips htest", hs.assert_htest(f"htest N={n} nharm={nharm} weights={int(weighted)} parts={parts}", Z, h, m, z2))


def plane_against_the_oracle(n, cycles, nharm, parts):
    """H, its m and Z2 of every row against the oracle, and the row without drift against the plain scan, bit for bit."""
    t, w = hs.ht_events(n)
    f0, delta, nf = hs.ht_grid(n)
    fdot, epoch = hs.fd_rows(n, cycles), hs.fd_epoch(n)
    out = _cabi.htest_fdot_scan(t, w, f0, delta, nf, fdot, epoch, nharm=nharm, parts=parts)
    assert _cabi.htest_fdot_last_dispatch()[2:] == (parts, len(cycles), 1)
    zz = _cabi.htest_fdot_scan(t, w, f0, delta, nf, fdot, epoch, nharm=nharm, stat="z2", parts=parts, want=("plane",))["plane"]
    Z = hs.fd_exact(n, cycles)
    worst = 0.0
    for r, c in enumerate(cycles):
        worst = max(worst, hs.assert_htest(f"fdot N={n} drift={c} nharm={nharm} parts={parts}", Z[r, :nharm], out["plane"][r],
                                           out["m_plane"][r], zz[r]))
    h, m, z2 = _cabi.htest_scan(t, w, f0, delta, nf, nharm, parts=parts)
    r0 = cycles.index(0.0)
    assert fdot[r0] == 0.0 and same(out["plane"][r0], h) and same(out["m_plane"][r0], m) and same(zz[r0], z2)
    return worst, out, Z


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("nharm", [2, 20])
@pytest.mark.parametrize("n", [1025, 4097])
def test_prologue_trips_htest_fdot(n, nharm, parts):
    group("trips fdot", plane_against_the_oracle(n, (0.0, 2.0), nharm, parts)[0])


# ---- the segment walk of the multiband prologue ---------------------------------------------------------------------------
def mb_against_the_oracle(name, nterms, top=3):
    t, y, err, band, B = hs.mb_inputs(name)
    got = _cabi.mbgls_scan(t, y, err, band, B, *hs.mb_grid(name), nterms)
    exact, keep = hs.mb_oracle(name, nterms, top)
    return hs.assert_gls(f"mbgls {name} nterms={nterms}", got, exact, keep)


@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("n", hs.SEGMENTS)
def test_segment_walk_mbgls(n, B):
    group("segments mbgls", max(mb_against_the_oracle(f"random-{n}-{B}", nterms) for nterms in (1, 2, 3)))


@pytest.mark.parametrize("name", list(hs.LAYOUTS))
def test_segment_walk_label_layouts(name):
    """Contiguous runs (a band inside one wave's segment, one across two, one in every segment), ``i % 3``, and a band
    whose one sample is the last of the curve: alone in its wave's second trip at 4097, alone in its segment at 1025."""
    group("layouts mbgls", max(mb_against_the_oracle(name, nterms) for nterms in (1, 2, 3)))


@pytest.mark.parametrize("n,B,nterms", hs.MANY)
def test_thirty_two_bands(n, B, nterms):
    assert B == 32
    group("32 bands mbgls", mb_against_the_oracle(f"many-{n}-{B}", nterms, nterms))


def device_call(entry, inputs, outputs, *args):
    """One `_dev` call on the null stream: ``inputs`` are uploaded (None stays NULL), ``outputs`` are (dtype, count)."""
    dev = _cabi.default_device()
    ins = [None if a is None else DB.from_array(a, dev) for a in inputs]
    outs = [DB(np.dtype(dtype).itemsize * count, dev) for dtype, count in outputs]
    try:
        _cabi.check(entry(dev, None, *[None if b is None else b.ptr for b in ins], *[a(outs) if callable(a) else a for a in args]))
        _cabi.check(_cabi.lib().pdc_device_sync(dev))
        return [b.to_array(dtype, count) for b, (dtype, count) in zip(outs, outputs)]
    finally:
        for b in ins + outs:
            if b is not None:
                b.free()


def out(i):
    """The device pointer of output ``i`` of a ``device_call``."""
    return lambda outs: outs[i].ptr


def mhgls_dev(t, y, err, f0, delta, nf, nterms):
    return device_call(_cabi.lib().pdc_mhgls_scan_dev, (t, y, err), [(np.float64, nf)], t.size, f0, delta, 0, nf, nterms, 1, 0, out(0))[0]


def mbgls_dev(t, y, err, labels, n_bands, f0, delta, nf, nterms):
    return device_call(_cabi.lib().pdc_mbgls_scan_dev, (t, y, err, np.asarray(labels, dtype=np.int32)), [(np.float64, nf)], t.size,
                       n_bands, f0, delta, 0, nf, nterms, 1, 0, out(0))[0]


def htest_dev(t, w, f0, delta, nf, nharm, parts):
    return device_call(_cabi.lib().pdc_htest_scan_dev, (t, w), [(np.float64, nf), (np.int32, nf), (np.float64, nf)], t.size, f0, delta,
                       0, nf, nharm, parts, out(0), out(1), out(2))


def fdot_dev(t, w, f0, delta, nf, fdot, epoch, nharm, parts):
    """(plane, m_plane, ridge, ridge_row, ridge_m, best, best_at), flat."""
    cells = fdot.size * nf
    shapes = [(np.float64, cells), (np.int32, cells), (np.float64, nf), (np.int32, nf), (np.int32, nf), (np.float64, 1), (np.int64, 3)]
    dev = _cabi.default_device()
    bf = DB.from_array(fdot, dev)
    try:
        return device_call(_cabi.lib().pdc_htest_fdot_scan_dev, (t, w), shapes, t.size, f0, delta, 0, nf, bf.ptr, fdot.size, epoch,
                           nharm, 0, parts, *[out(i) for i in range(7)])
    finally:
        bf.free()


@pytest.mark.parametrize("n", hs.GAPS)
def test_dev_entry_skips_a_band_without_samples(n):
    """Labels {0, 2} under ``n_bands = 3`` (the host form refuses them, the `_dev` form cannot look): the value is that of
    the same curve with the labels compacted to two bands - the oracle's, and the host entry's to rounding."""
    name = f"gap-{n}"
    t, y, err, band, B = hs.mb_inputs(name)
    assert B == 2 and set(band.tolist()) == {0, 1}
    f0, delta, nf = hs.mb_grid(name)
    worst = 0.0
    for nterms in (1, 2, 3):
        got = mbgls_dev(t, y, err, 2 * band, 3, f0, delta, nf, nterms)
        exact, keep = hs.mb_oracle(name, nterms)
        worst = max(worst, hs.assert_gls(f"mbgls {name} (labels 0 and 2 of three) nterms={nterms}", got, exact, keep))
        np.testing.assert_allclose(got[keep], _cabi.mbgls_scan(t, y, err, band, 2, f0, delta, nf, nterms)[keep], rtol=1e-9, atol=0)
    group("empty band mbgls", worst)


# ---- more than eight tiles ------------------------------------------------------------------------------------------------
def test_more_than_eight_tiles_of_the_gls_scans():
    """mhgls and mbgls give workgroup p the tile (p % 8) ceil(tiles / 8) + p / 8: the identity up to eight tiles, which
    is as far as the other tests' grids go.  9217 bins are ten tiles of 1024 and nineteen of 512, every bin compared."""
    t, y, err = hs.mh_curve(65)
    grid = hs.wide_grid(t)
    worst = 0.0
    for nterms in (1, 4):
        exact, keep = hs.gls_oracle(hs.mo, hs.mh_wide_equations(), 2 * nterms + 1)
        worst = max(worst, hs.assert_gls(f"mhgls wide nterms={nterms}", _cabi.mhgls_scan(t, y, err, *grid, nterms), exact, keep))
    t, y, err, band, B = hs.mb_inputs("random-65-3")
    grid = hs.wide_grid(t)
    for nterms in (1, 3):
        assert -(-hs.WIDE // _cabi.mbgls_tile_bins(nterms)) > 8
        exact, keep = hs.gls_oracle(hs.mb, hs.mb_wide_equations(), hs.mb.columns(B, nterms, True))
        worst = max(worst, hs.assert_gls(f"mbgls wide nterms={nterms}", _cabi.mbgls_scan(t, y, err, band, B, *grid, nterms), exact, keep))
    group("wide grid mhgls mbgls", worst)


# ---- one size up: 20 000 samples, 128 picked bins -------------------------------------------------------------------------
def test_one_size_up_mhgls():
    t, y, err = hs.mh_curve(hs.BIG)
    got = _cabi.mhgls_scan(t, y, err, *hs.mh_grid(hs.BIG), 4)
    exact, keep = hs.mh_oracle(hs.BIG, 4, picked=True)
    group("20000 mhgls", hs.assert_gls(f"mhgls N={hs.BIG} nterms=4", got[hs.PICK], exact, keep))
    assert same(got, _cabi.mhgls_scan(t, y, err, *hs.mh_grid(hs.BIG), 4))


def test_one_size_up_mbgls():
    t, y, err, band, B = hs.mb_inputs("big")
    assert (t.size, B) == (hs.BIG, 6)
    got = _cabi.mbgls_scan(t, y, err, band, B, *hs.mb_grid("big"), 3)
    exact, keep = hs.mb_oracle("big", 3, picked=True)
    group("20000 mbgls", hs.assert_gls(f"mbgls N={hs.BIG} B=6 nterms=3", got[hs.PICK], exact, keep))
    assert same(got, _cabi.mbgls_scan(t, y, err, band, B, *hs.mb_grid("big"), 3))


def test_one_size_up_htest():
    """One tile plus one bin at 313 chunks: the automatic rule gives every tile several sample parts."""
    t, w = hs.ht_events(hs.BIG)
    got = _cabi.htest_scan(t, w, *hs.ht_grid(hs.BIG), 20, parts=0)
    assert _cabi.htest_last_dispatch()[2] > 1
    Z = hs.ht_exact(hs.BIG, True, True)
    group("20000 htest", hs.assert_htest(f"htest N={hs.BIG} nharm=20", Z, *[a[hs.PICK] for a in got]))
    assert all(same(a, b) for a, b in zip(got, _cabi.htest_scan(t, w, *hs.ht_grid(hs.BIG), 20, parts=0)))


# ---- 1e6 cycles over the baseline -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nterms", [1, 4])
def test_a_million_cycles_mhgls(nterms):
    t, y, err = hs.mh_curve("long")
    got = _cabi.mhgls_scan(t, y, err, *hs.mh_grid("long"), nterms)
    exact, keep = hs.mh_oracle("long", nterms)
    group("1e6 cycles mhgls", hs.assert_gls(f"mhgls 1e6 cycles nterms={nterms}", got, exact, keep))   # (the peak bin too)


@pytest.mark.parametrize("nterms", [1, 3])
def test_a_million_cycles_mbgls(nterms):
    assert hs.mb_inputs("long")[4] == 3
    group("1e6 cycles mbgls", mb_against_the_oracle("long", nterms))


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("nharm", [2, 20])
def test_a_million_cycles_htest(nharm, parts):
    t, w = hs.ht_events("long")
    h, m, z2 = _cabi.htest_scan(t, w, *hs.ht_grid("long"), nharm, parts=parts)
    Z = hs.ht_exact("long")[:nharm]
    group("1e6 cycles htest", hs.assert_htest(f"htest 1e6 cycles nharm={nharm} parts={parts}", Z, h, m, z2))
    hs.assert_peak(f"htest 1e6 cycles nharm={nharm}", Z, h, m)


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("nharm", [2, 20])
def test_a_million_cycles_htest_fdot(nharm, parts):
    cycles = (0.0, 2.0, -4.5)
    worst, got, Z = plane_against_the_oracle("long", cycles, nharm, parts)
    group("1e6 cycles fdot", worst)
    for r in range(len(cycles)):
        hs.assert_peak(f"fdot 1e6 cycles row {r} nharm={nharm}", Z[r, :nharm], got["plane"][r], got["m_plane"][r])
    assert got["best"][2] == 0 and got["best"][1] == int(np.argmax(hs.ho.h_and_m(Z[0, :nharm])[0]))   # the pulsar does not drift


# ---- stale workspace ------------------------------------------------------------------------------------------------------
# What the four calls below need of the block: 1027 records of 48 B and the scalars behind them (50 KB), and for the two
# H-test forms the partial sums of three parts, 3 x 40 x 1025 x 8 B = 984 000 B per row of the plane.
SCRATCH = 8 << 20


def poison_the_scratch_block():
    """Pin the null stream's block, fill it with 0xFF bytes (NaN as doubles, -1 as counts) and unpin it - one holder at a
    time, pinned and unpinned from this thread."""
    lib, dev = _cabi.lib(), _cabi.default_device()
    _cabi.check(lib.pdc_device_sync(dev))
    block = C.c_void_p()
    _cabi.check(lib.pdc_test_scratch_pin(dev, None, SCRATCH, C.byref(block)))
    try:
        _cabi.check(lib.pdc_memset(dev, block, 0xFF, SCRATCH))
        _cabi.check(lib.pdc_device_sync(dev))
    finally:
        _cabi.check(lib.pdc_test_scratch_unpin(dev, None))


@pytest.mark.parametrize("family", ["mhgls", "mbgls", "htest", "htest_fdot"])
def test_dev_entry_reads_nothing_stale_from_its_workspace(family):
    """One `_dev` call at 1025 samples on a block full of 0xFF has the bits of the host entry (which has a workspace of its
    own); the H-test forms with three sample parts, so their partial sums are in the block too."""
    if family == "mhgls":
        t, y, err = hs.mh_curve(1025)
        grid = hs.mh_grid(1025)
        want = [_cabi.mhgls_scan(t, y, err, *grid, 4)]
        poison_the_scratch_block()
        got = [mhgls_dev(t, y, err, *grid, 4)]
    elif family == "mbgls":
        t, y, err, band, B = hs.mb_inputs("random-1025-4")
        grid = hs.mb_grid("random-1025-4")
        want = [_cabi.mbgls_scan(t, y, err, band, B, *grid, 3)]
        poison_the_scratch_block()
        got = [mbgls_dev(t, y, err, band, B, *grid, 3)]
    elif family == "htest":
        t, w = hs.ht_events(1025)
        grid = hs.ht_grid(1025)
        want = list(_cabi.htest_scan(t, w, *grid, 20, parts=3))
        assert _cabi.htest_last_dispatch()[2] == 3
        poison_the_scratch_block()
        got = htest_dev(t, w, *grid, 20, 3)
    else:
        t, w = hs.ht_events(1025)
        f0, delta, nf = hs.ht_grid(1025)
        fdot, epoch = hs.fd_rows(1025, (0.0, 2.0)), hs.fd_epoch(1025)
        assert 0 < _cabi.htest_fdot_work_bytes(1025, nf, 2, 20, 3, True) <= SCRATCH
        host = _cabi.htest_fdot_scan(t, w, f0, delta, nf, fdot, epoch, nharm=20, parts=3)
        assert _cabi.htest_fdot_last_dispatch()[2:] == (3, 2, 1)
        want = [host["plane"].ravel(), host["m_plane"].ravel(), host["ridge"], host["ridge_row"], host["ridge_m"],
                np.array([host["best"][0]]), np.array(host["best"][1:], dtype=np.int64)]
        poison_the_scratch_block()
        got = fdot_dev(t, w, f0, delta, nf, fdot, epoch, 20, 3)
    assert len(got) == len(want) and all(same(a, b) for a, b in zip(got, want))
    assert all(np.all(np.isfinite(a)) for a in got if a.dtype.kind == "f")
