"""WWZ on the GPU (csrc/wwz.hip through the class and the C ABI) against the test-local 80-bit oracle
(tests/wwz_oracle.py: exp, cos and sin evaluated directly per pair, no recurrence, no support cut, no centring; its
float64 evaluation sits below 1e-3 of the gate, tests/test_wwz_host.py).  PARITY UNPINNED BY THE REFERENCE.

Gate and keep rule: WWZ, WWA and Neff are held to Tier E, |got - exact| <= 1e-6 |exact| + 1e-9, on the cells whose
oracle Neff is at least 6; every other cell must be NaN or finite; at most 5 % of a grid may be left out, which every
parity test asserts.  Everything that should be the same computation is compared bit for bit."""
import functools

import numpy as np
import pytest

import wwz_oracle as wo
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.timefrequency import WWZ

pytestmark = pytest.mark.gpu

PLANES = ("wwz", "amp", "neff")


def scan(t, y, err, freq, tau, decay=wo.FOSTER, **kw):
    f0, delta, nf = _cabi.grid_params(freq)
    if nf < 2:
        delta = 1.0
    return _cabi.wwz_scan(t, y, err, f0, delta, nf, tau, decay, **kw)


def assert_meets_oracle(label, got, exact):
    """Prints each family's worst error over its gate and the share left out before it asserts."""
    for name, want in zip(PLANES, exact):
        worst, left_out = wo.compare(got[name], want, exact[2])
        print(f"{label} {name}: error / gate = {worst:.3e}, left out {left_out:.4f} (cap {wo.LEFT_OUT_CAP})")
        assert left_out <= wo.LEFT_OUT_CAP, (label, name, left_out)
        assert worst <= 1.0, (label, name, worst)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_reductions_follow_numpy(out, min_neff=wo.MIN_NEFF):
    """Ridge and best cell are the numpy expressions on the returned planes, bit for bit."""
    bins, rz, ra, best = wo.reductions(out["wwz"], out["amp"], out["neff"], min_neff)
    assert np.array_equal(out["ridge_bin"], bins)
    assert same(out["ridge_wwz"][bins >= 0], rz[bins >= 0]) and np.all(np.isnan(out["ridge_wwz"][bins < 0]))
    assert same(out["ridge_amp"][bins >= 0], ra[bins >= 0]) and np.all(np.isnan(out["ridge_amp"][bins < 0]))
    assert out["best"][1:] == best[1:]
    assert out["best"][0] == best[0] or (np.isnan(out["best"][0]) and np.isnan(best[0]))


@functools.lru_cache(maxsize=None)
def chirp_exact(weighted, decay, offset=0.0):
    t, y, err, freq, tau = wo.chirp_curve(offset)
    return wo.planes(t, y, err if weighted else None, freq, tau, decay)


@pytest.mark.parametrize("decay", [wo.FOSTER, 0.005])
@pytest.mark.parametrize("weighted", [False, True])
def test_parity_chirp(weighted, decay):
    t, y, err, freq, tau = wo.chirp_curve()
    out = scan(t, y, err if weighted else None, freq, tau, decay)
    assert_meets_oracle(f"chirp weighted={weighted} decay={decay:.4g}", out, chirp_exact(weighted, decay))
    assert_reductions_follow_numpy(out)


@pytest.mark.parametrize("weighted", [False, True])
def test_parity_at_a_julian_date_offset(weighted):
    t, y, err, freq, tau = wo.chirp_curve(2450000.0)
    out = scan(t, y, err if weighted else None, freq, tau)
    assert_meets_oracle(f"offset weighted={weighted}", out, chirp_exact(weighted, wo.FOSTER, 2450000.0))


def seam_curve(n):
    """The chirp input at ``n`` samples on a baseline scaled to its density (100 n / 253, no gap): Neff >= 6 on at
    least 95 % of the cells at every size used here, checked on the CPU (the worst, n = 65 weighted, leaves 3.3 % out)."""
    rng = np.random.default_rng(20261020 + n)
    span = 100.0 * n / 253
    t = np.sort(rng.uniform(0, span, n))
    y = np.sin(2 * np.pi * (0.2 + 0.1 * t / span) * t) * (1 + t / 200) + 0.3 * rng.standard_normal(n) + 5
    return t, y, rng.uniform(0.2, 0.5, n), np.linspace(0, span, 5)


@pytest.mark.parametrize("n", [63, 64, 65, 129])   # the chunk seams of scan_stretch
def test_sample_seams(n):
    t, y, err, tau = seam_curve(n)
    freq = wo.chirp_curve()[3]
    for e in (None, err):
        out = scan(t, y, e, freq, tau)
        assert_meets_oracle(f"n={n} weighted={e is not None}", out, wo.planes(t, y, e, freq, tau))
        assert out["visited"] == n * tau.size   # nothing is cut at these baselines


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_tile_seams(extra):
    tile = _cabi.wwz_tile_bins()
    nf = tile + extra
    t, y, err, _, _ = wo.chirp_curve()
    freq = 0.05 + (0.4 / nf) * np.arange(nf)
    tau = np.array([25.0, 75.0])
    out = scan(t, y, err, freq, tau)
    assert out["wwz"].shape == (2, nf)
    assert_meets_oracle(f"nf={nf}", out, wo.planes(t, y, err, freq, tau))
    assert_reductions_follow_numpy(out)
    assert out["visited"] == t.size * tau.size * ((nf + tile - 1) // tile)


def test_one_time_shift():
    t, y, err, freq, _ = wo.chirp_curve()
    tau = np.array([30.0])
    out = scan(t, y, err, freq, tau)
    assert_meets_oracle("ntau=1", out, wo.planes(t, y, err, freq, tau))
    assert_reductions_follow_numpy(out)
    assert out["best"][1] == 0


def test_support_cut_is_proved_to_have_run():
    """4000 samples on [0, 1000), bins from 0.5: the support is +-77 time units around a tau, about 15 % of the samples."""
    t, y, _, freq, tau = wo.dense_curve()
    tiles = (freq.size + _cabi.wwz_tile_bins() - 1) // _cabi.wwz_tile_bins()
    out = scan(t, y, None, freq, tau)
    assert_meets_oracle("support cut", out, wo.planes(t, y, None, freq, tau))
    assert_reductions_follow_numpy(out)
    print(f"visited {out['visited']} of {t.size * tiles * tau.size}")
    assert 0 < out["visited"] < 0.25 * t.size * tiles * tau.size
    wide = scan(t, y, None, freq, tau, decay=1e-12, want_planes=False)
    assert wide["visited"] == t.size * tiles * tau.size


def test_reductions_bit_for_bit():
    t, y, err, freq, tau = wo.chirp_curve()
    tau = np.concatenate([tau, tau[3:4]])   # a duplicated time shift: two identical rows
    out = scan(t, y, None, freq, tau)
    assert_reductions_follow_numpy(out)
    assert np.any(out["neff"] < wo.MIN_NEFF)   # (the rule had something to exclude)
    for name in PLANES:
        assert same(out[name][3], out[name][-1])
    for name in ("ridge_bin", "ridge_wwz", "ridge_amp"):
        assert same(out[name][3:4], out[name][-1:])
    bare = scan(t, y, None, freq, tau, want_planes=False)
    assert all(bare[name] is None for name in PLANES)
    for name in ("ridge_bin", "ridge_wwz", "ridge_amp"):
        assert same(out[name], bare[name])
    assert same(np.array(out["best"]), np.array(bare["best"])) and out["visited"] == bare["visited"]
    # one eligible cell in row 5: min_neff between the row's two largest Neff
    top = np.sort(out["neff"][5])[-2:]
    assert top[0] < top[1]
    one = scan(t, y, None, freq, tau, min_neff=0.5 * (top[0] + top[1]))
    assert one["ridge_bin"][5] == int(np.argmax(out["neff"][5]))
    for name in PLANES:
        assert same(one[name], out[name])   # min_neff never touches the planes
    assert_reductions_follow_numpy(one, 0.5 * (top[0] + top[1]))
    none = scan(t, y, None, freq, tau, min_neff=float(np.max(out["neff"])) + 1.0)
    assert np.all(none["ridge_bin"] == -1) and np.all(np.isnan(none["ridge_wwz"])) and np.all(np.isnan(none["ridge_amp"]))
    assert none["best"][1:] == (-1, -1) and np.isnan(none["best"][0])


@pytest.mark.parametrize("weighted", [False, True])
def test_recovers_the_chirp(weighted):
    """The ridge follows the instantaneous frequency 0.2 + 0.002 tau (bin 30 + 0.4 tau) within 2 bins outside the gap."""
    t, y, err, freq, tau = wo.chirp_curve()
    out = scan(t, y, err if weighted else None, freq, tau)
    away = (tau < 35) | (tau > 60)
    expect = np.rint(30 + 0.4 * tau).astype(np.int64)
    print("ridge", freq[out["ridge_bin"]])
    assert np.all(np.abs(out["ridge_bin"] - expect)[away] <= 2), out["ridge_bin"]


def test_class_returns_what_the_library_computes():
    t, y, err, _, tau = wo.chirp_curve()
    w = WWZ(0.05, 0.445, n=2, decay=0.005, min_neff=8)
    m = w(TSeries(t, y), err, taus=tau)
    out = scan(t, y, err, m.frequency, tau, decay=0.005, min_neff=8)
    assert m.wwz.shape == (tau.size, m.frequency.size)
    assert same(m.wwz, out["wwz"]) and same(m.amplitude, out["amp"]) and same(m.neff, out["neff"])
    assert same(m.ridge_bin, out["ridge_bin"]) and same(m.ridge_wwz, out["ridge_wwz"])
    assert np.array_equal(m.ridge_frequency, m.frequency[m.ridge_bin]) and np.array_equal(m.ridge_period, 1 / m.ridge_frequency)
    row = int(np.nanargmax(m.ridge_wwz))
    assert m.best == (tau[row], m.ridge_frequency[row], m.ridge_wwz[row], m.ridge_amplitude[row])
    bare = w(TSeries(t, y), err, taus=5, want_planes=False)
    assert bare.wwz is None and np.array_equal(bare.tau, np.linspace(t[0], t[-1], 5)) and np.all(bare.ridge_bin >= 0)


def test_more_rows_than_one_launch_takes():
    """65536 + 2 time shifts run as two launches; the rows behind the seam hold the bits of a short call."""
    t, y, err, _ = seam_curve(64)
    freq = 0.2 + 0.01 * np.arange(3)
    tau = np.linspace(t[0], t[-1], 65538)
    out = scan(t, y, err, freq, tau)
    k, rows, launches = _cabi.wwz_last_dispatch()
    assert rows == 65535 and launches == 2 and k * 256 == _cabi.wwz_tile_bins()
    pick = np.array([0, 65534, 65535, 65537])
    short = scan(t, y, err, freq, tau[pick])
    for name in PLANES + ("ridge_bin", "ridge_wwz", "ridge_amp"):
        assert same(out[name][pick], short[name])
    assert_reductions_follow_numpy(out)


def test_host_entry_and_dev_twin_are_bit_identical():
    t, y, err, freq, tau = wo.chirp_curve()
    f0, delta, nf = _cabi.grid_params(freq)
    host = scan(t, y, err, freq, tau)
    DB = _cabi.DeviceBuffer
    dev = _cabi.default_device()
    cells, ntau = tau.size * nf, tau.size
    ins = [DB.from_array(a, dev) for a in (t, y, err, tau)]
    sizes = (cells, cells, cells, ntau, ntau, ntau, 1, 2, 1)
    outs = [DB(count * 8, dev) for count in sizes]
    try:
        _cabi.check(_cabi.lib().pdc_wwz_scan_dev(dev, None, ins[0].ptr, ins[1].ptr, ins[2].ptr, t.size, f0, delta, nf,
                                                 ins[3].ptr, ntau, wo.FOSTER, 6.0, *[b.ptr for b in outs]))
        _cabi.check(_cabi.lib().pdc_device_sync(dev))
        f8, i8 = np.float64, np.int64
        twin = [b.to_array(dtype, count) for b, dtype, count in zip(outs, (f8, f8, f8, i8, f8, f8, f8, i8, i8), sizes)]
    finally:
        for b in ins + outs:
            b.free()
    for name, got in zip(PLANES, twin):
        assert same(host[name].ravel(), got)
    assert same(host["ridge_bin"], twin[3]) and same(host["ridge_wwz"], twin[4]) and same(host["ridge_amp"], twin[5])
    assert host["best"] == (float(twin[6][0]), int(twin[7][0]), int(twin[7][1])) and host["visited"] == int(twin[8][0])


def test_hygiene_no_allocation_on_a_repeated_or_rejected_call():
    t, y, err, freq, tau = wo.chirp_curve()
    first = scan(t, y, err, freq, tau)
    counts = _cabi.alloc_counts()
    again = scan(t, y, err, freq, tau)
    assert _cabi.alloc_counts() == counts
    assert all(same(first[name], again[name]) for name in PLANES + ("ridge_bin", "ridge_wwz", "ridge_amp"))
    assert first["best"] == again["best"] and first["visited"] == again["visited"]
    f0, delta, nf = _cabi.grid_params(freq)
    for bad in (dict(t=t[::-1].copy()), dict(tau=np.array([10.0, np.nan])), dict(decay=0.0), dict(decay=-1.0),
                dict(t=t[:3], y=y[:3], dy=err[:3])):
        args = dict(t=t, y=y, dy=err, f0=f0, delta=delta, nf=nf, tau=tau, decay=wo.FOSTER)
        args.update(bad)
        with pytest.raises(ValueError):
            _cabi.wwz_scan(**args)
    null = [None] * 9
    with pytest.raises(ValueError):   # every output NULL
        _cabi.check(_cabi.lib().pdc_wwz_scan(_cabi._ptr(t), _cabi._ptr(y), _cabi._ptr(err), t.size, f0, delta, nf,
                                             _cabi._ptr(tau), tau.size, wo.FOSTER, 6.0, *null, _cabi.default_device()))
    assert _cabi.alloc_counts() == counts
