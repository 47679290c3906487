"""Inputs, grids and oracle values that tests/test_harmonic_sizes_host.py and tests/test_harmonic_sizes_gpu.py share (plain
numpy; imports nothing from ``periodicity_amd``): the four harmonic-sum scans - MultiHarmonicGLS, MultibandGLS, HTest /
ZTest and their (f, fdot) plane - at the sizes where their prologues take more than one trip, at many bands, at 20 000
samples and at about 1e6 cycles over the baseline.  Every oracle value is evaluated once per process and shared.

Grids.  ``delta = 1 / (5 span)`` as the default grid has it, ``NF`` = 1025 bins - one tile of 1024 plus one bin, two tiles
of 512 plus one - centred on the frequency the generator put into the data, so the peak and its flanks are inside and not
only noise bins whose power the absolute term of the gate covers.  A curve too short for that (200 samples) takes 257.

Left-out bins.  A GLS bin counts in value where cond(M) <= 1e6 on the oracle's full matrix; ``harmonics`` counts where
the oracle's best and second-best candidate are more than twice the value gate apart.  At most 5 % / 1 % of a case's
bins may be left out: ``gls_oracle`` and ``assert_htest`` refuse more (the host tests call both for every shape)."""
import functools

import numpy as np

import htest_fdot_oracle as fo
import htest_oracle as ho
import mbgls_oracle as mb
import mhgls_oracle as mo

NF = 1025
CHUNK = 64                       # [CHUNK][D][N] in float64 at D = 38, N = 4097 is 82 MB
CURVE_FREQUENCY = 1 / 6.3        # mhgls_oracle.curve
EVENT_FREQUENCY = 1 / 7.3        # htest_oracle.events
TRIPS = (1022, 1023, 1024, 1025, 2049, 4097)   # n + 2 records over 1024 threads: the spare two in trip 1, split, in trip 2
BIG = 20_000
# 128 of 1025 bins: both ends, 511 | 512 | 513 and 1023 | 1024 around the seams of both tile sizes, the rest spread evenly
PICK = np.unique(np.r_[np.linspace(0, NF - 1, 125).round().astype(int), 511, 513, 1023])
assert PICK.size == 128 and {0, 511, 512, 1023, 1024} <= set(PICK.tolist())


def centred(f_signal, t, nf=NF):
    """``(f0, delta, nf)`` of the grid of ``nf`` bins around ``f_signal`` at the default spacing of the baseline of ``t``."""
    delta = 1.0 / (5.0 * (t.max() - t.min()))
    f0 = f_signal - (nf // 2) * delta
    assert f0 > 0
    return float(f0), float(delta), nf


def frequencies(f0, delta, nf):
    """The grid as the kernels fill it: ``f0 + j delta``, two roundings."""
    return f0 + delta * np.arange(nf)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the two GLS families ---------------------------------------------------------------------------------------------
def gls_gate(exact):
    return 1e-6 * np.abs(exact) + 1e-9   # Tier E: <= 1e-6 relative in fp64


def gls_oracle(oracle, equations, columns, psd=False):
    """``(exact power, kept bins)`` from the leading ``columns`` of a case's normal equations."""
    M, b, YY, W = equations
    M, b = M[:, :columns, :columns], b[:, :columns]
    keep = oracle.cond_from(M) <= oracle.COND_LIMIT
    assert 1 - keep.mean() <= 0.05, f"{100 * (1 - keep.mean()):.2f} % of the bins left out"
    return np.asarray(oracle.power_from(M, b, YY, W, psd), dtype=np.float64), keep


def assert_gls(label, got, exact, keep):
    """The rule of tests/test_mhgls_gpu.py and tests/test_mbgls_gpu.py; returns the worst error over its gate."""
    err = np.abs(got[keep] - exact[keep])
    gate = gls_gate(exact[keep])
    worst = float(np.max(err / gate))
    print(f"{label}: bins {got.size} kept {int(keep.sum())} max |err| {err.max():.3e} max err/gate {worst:.3e}")
    assert np.all(err <= gate), (label, worst)
    assert int(np.argmax(np.where(keep, got, -np.inf))) == int(np.argmax(np.where(keep, exact, -np.inf))), label
    assert not np.any(np.isinf(got[~keep])), label   # left-out bins: NaN or finite
    return worst


@functools.lru_cache(maxsize=None)
def mh_curve(n):
    """``(t, y, err)``: ``mhgls_oracle.curve`` of size ``n`` (seed 1000 + n), or the long-baseline curve for "long"."""
    return frozen(*(mo.long_curve() if n == "long" else mo.curve(n, 1000 + n)))


def mh_grid(n):
    return centred(1 / mo.LONG_PERIOD if n == "long" else CURVE_FREQUENCY, mh_curve(n)[0])


@functools.lru_cache(maxsize=None)
def mh_equations(n, with_err=True, fit_mean=True, picked=False, dtype=np.float64):
    """The oracle's normal equations at four harmonics (fewer are a leading block); ``picked``: on ``PICK`` only."""
    t, y, err = mh_curve(n)
    freq = frequencies(*mh_grid(n))
    return mo.normal_equations(t, y, err if with_err else None, freq[PICK] if picked else freq, 4, fit_mean, dtype, CHUNK)


def mh_oracle(n, nterms, with_err=True, fit_mean=True, picked=False):
    return gls_oracle(mo, mh_equations(n, with_err, fit_mean, picked), 2 * nterms + (1 if fit_mean else 0))


def runs(*lengths):
    """Labels 0, 1, ... in contiguous runs of the given lengths."""
    return np.repeat(np.arange(len(lengths)), lengths)


def random_labels(n, n_bands, seed):
    return mb.with_labels(np.zeros(n), np.zeros(n), None, n_bands, seed)[3]


# The prologue of mbgls.hip gives each of its 16 waves a segment of roundup64(ceil(n / 16)) samples and walks it 256 at a
# time.  n = 4097: segments of 320 (a trip of 256, then one of 64), the thirteenth holds 3840 .. 4096 and its second trip
# the one sample 4096; n = 1025: segments of 128, the ninth holds the one sample 1024.
LAYOUTS = {
    # band 1 inside the second wave's segment, band 2 across the seam of two segments, band 0 in every segment (three runs)
    "runs-4097": lambda: np.array([0, 1, 0, 2, 0])[runs(400, 100, 1500, 400, 1697)],
    "interleaved-4097": lambda: np.arange(4097) % 3,
    "single-4097": lambda: np.r_[random_labels(4096, 2, 5), 2],
    "single-1025": lambda: np.r_[random_labels(1024, 2, 6), 2],
}
SEGMENTS = (1024, 1025, 4096, 4097, 8193)    # segments of 64, 128, 256, 320 and 576 samples
MANY = ((1025, 32, 3), (4097, 32, 1))        # (n, bands, nterms): kMaxBands
GAPS = (200, 4097)                           # labels {0, 2} under n_bands = 3


@functools.lru_cache(maxsize=None)
def mb_inputs(name):
    """``(t, y, err, band, n_bands)`` of a multiband case, named "random-N-B", "many-N-B", "gap-N" (the compacted labels
    {0, 1}: the device takes them doubled under three bands), a key of ``LAYOUTS``, "big" or "long"."""
    kind, _, rest = name.partition("-")
    if name == "long":
        t, y, err, band = mb.long_curve(3)
        return frozen(t, y, err, band) + (3,)
    if name == "big":
        t, y, err, band = mb.curve(BIG, 6, seed=3000 + BIG)
        return frozen(t, y, err, band) + (6,)
    if kind in ("random", "many"):
        n, B = (int(v) for v in rest.split("-"))
        t, y, err, band = mb.curve(n, B, seed=3000 + n)
        return frozen(t, y, err, band) + (B,)
    n = int(rest)
    t, y, err = mo.curve(n, 3000 + n)
    band = random_labels(n, 2, 7) if kind == "gap" else np.asarray(LAYOUTS[name]())
    assert band.shape == (n,) and set(band.tolist()) == set(range(band.max() + 1))
    return frozen(t, y + 0.5 * band, err, band) + (int(band.max()) + 1,)


def mb_grid(name):
    t = mb_inputs(name)[0]
    return centred(1 / mo.LONG_PERIOD if name == "long" else CURVE_FREQUENCY, t, 257 if name == "gap-200" else NF)


@functools.lru_cache(maxsize=None)
def mb_equations(name, nterms=3, picked=False, dtype=np.float64):
    """The oracle's normal equations with ``nterms`` harmonics (fewer are a leading block); ``picked``: on ``PICK``."""
    t, y, err, band, B = mb_inputs(name)
    freq = frequencies(*mb_grid(name))
    return mb.normal_equations(t, y, err, band, B, freq[PICK] if picked else freq, nterms, True, dtype, CHUNK)


def mb_oracle(name, nterms, top=3, picked=False):
    """``top``: the harmonics of the equations that are evaluated (and cached) for the case."""
    return gls_oracle(mb, mb_equations(name, top, picked), mb.columns(mb_inputs(name)[4], nterms, True))


# The two GLS scans order their tiles by XCD: workgroup p takes tile (p % 8) ceil(tiles / 8) + p / 8.  Up to eight tiles
# that is the identity; WIDE bins are ten tiles of 1024 and nineteen of 512, on the default grid of a 65-sample curve.
WIDE = 9 * 1024 + 1


def wide_grid(t):
    delta = 1.0 / (5.0 * (t.max() - t.min()))
    return float(0.5 * delta), float(delta), WIDE


@functools.lru_cache(maxsize=None)
def mh_wide_equations():
    t, y, err = mh_curve(65)
    return mo.normal_equations(t, y, err, frequencies(*wide_grid(t)), 4, True)


@functools.lru_cache(maxsize=None)
def mb_wide_equations():
    t, y, err, band, B = mb_inputs("random-65-3")
    return mb.normal_equations(t, y, err, band, B, frequencies(*wide_grid(t)), 3, True)


# ---- the H-test family ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ht_events(n):
    """``(t, w)``: ``htest_oracle.events`` of size ``n`` (seed 2000 + n), or the long-baseline list for "long"."""
    return frozen(*(ho.long_events() if n == "long" else ho.events(n, 2000 + n)))


def ht_grid(n):
    return centred(ho.LONG_FREQUENCY if n == "long" else EVENT_FREQUENCY, ht_events(n)[0])


@functools.lru_cache(maxsize=None)
def ht_exact(n, weighted=True, picked=False, dtype=np.float64):
    """The oracle's cumulative Z2_m, m = 1 .. 20, ``[20][bins]``: fewer harmonics are its leading rows."""
    t, w = ht_events(n)
    freq = frequencies(*ht_grid(n))
    return frozen(ho.z2(t, w if weighted else None, freq[PICK] if picked else freq, 20, dtype, CHUNK))[0]


def fd_epoch(n):
    t = ht_events(n)[0]
    return float(fo.epoch_of(t, "middle"))


def fd_rows(n, cycles):
    return fo.rows_of(ht_events(n)[0], fd_epoch(n), cycles)


@functools.lru_cache(maxsize=None)
def fd_row(n, drift, dtype=np.float64):
    """One row of the oracle's plane, ``[20][NF]``: weighted, epoch in the middle of the list, a drift of ``drift``
    cycles at the event farthest from the epoch."""
    t, w = ht_events(n)
    return frozen(fo.z2_fdot(t, w, frequencies(*ht_grid(n)), fd_rows(n, (drift,))[0], fd_epoch(n), 20, dtype, CHUNK))[0]


def fd_exact(n, cycles):
    """The oracle's plane, ``[rows][20][NF]``, one row per drift in ``cycles``."""
    return np.stack([fd_row(n, c) for c in cycles])


def assert_htest(label, Z, h=None, m=None, z2=None):
    """The rule of tests/test_htest_gpu.py and tests/test_htest_fdot_gpu.py on the oracle's rows ``Z`` (1 .. nharm);
    returns the worst error over its gate."""
    gate = ho.gate(Z)
    h_exact, m_exact = ho.h_and_m(Z)
    worst = 0.0
    for name, got, want in (("H", h, h_exact), ("Z2", z2, Z[-1])):
        if got is not None:
            err = np.abs(got - want)
            worst = max(worst, float(np.max(err / gate)))
            print(f"{label} {name}: bins {got.size} max |err| {err.max():.3e} max err/gate {np.max(err / gate):.3e}")
            assert np.all(err <= gate), (label, name, float(np.max(err / gate)))
    keep = ho.decided(Z)
    assert 1 - keep.mean() <= 0.01, (label, f"{100 * (1 - keep.mean()):.2f} % of the bins left out")
    if m is not None:
        assert m.dtype == np.int32 and np.array_equal(m[keep], m_exact[keep]), label
        assert np.all((m >= 1) & (m <= Z.shape[0])), label
    return worst


def assert_peak(label, Z, h, m):
    """The highest bin of H and the harmonics that give it are the oracle's."""
    h_exact, m_exact = ho.h_and_m(Z)
    peak = int(np.argmax(h_exact))
    assert int(np.argmax(h)) == peak and int(m[peak]) == int(m_exact[peak]), (label, peak, int(np.argmax(h)))
