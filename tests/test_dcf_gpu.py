"""The discrete correlation function on the GPU (``pdc_dcf_scan``, csrc/dcf.hip) against the test-local oracle
(tests/dcf_oracle.py): counts equal in every bin, every sum of every bin inside the derived gate
``(pairs + 8) 2^-53 sum |term|``, at the seams of the layout (a lane per bin: 63 / 64 / 65 / 257 bins; a chunk of
consecutive samples: chunk - 1 / chunk / chunk + 1 / 2 chunk + 1 samples), under rounding at every edge, on ties, empty
bins, empty curves and NaN values; then the host class on top.  The reference has no such statistic - PARITY UNPINNED BY
THE REFERENCE; on an evenly sampled curve the DCF is its mask-corrected FFT autocorrelation, which is checked.
Worst error / gate seen on an MI355X: see DESIGN.md (the DCF section)."""
import functools

import numpy as np
import pytest

import dcf_oracle as do
import dcf_raw as raw
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.correlation import DCF

pytestmark = pytest.mark.gpu


def check(label, ta, a, tb, b, edges, skip=False, chunk=0, oracle=None):
    """One scan held to the oracle; returns (pairs, sums, oracle)."""
    oracle = oracle or do.scan(ta, a, tb, b, edges, skip)
    pairs, sums = _cabi.dcf_scan(ta, a, tb, b, edges, skip, chunk)
    ratio = do.worst_ratio(pairs, sums, oracle)
    chunks, size = _cabi.dcf_last_dispatch()
    print(f"{label}: {int(oracle.pairs.sum())} pairs, {chunks} chunks of {size}: worst error / gate {ratio:.3f}")
    return pairs, sums, oracle


@functools.lru_cache(maxsize=None)
def auto_oracle():
    t, x, edges = do.uneven_auto()
    return do.scan(t, x, t, x, edges, True)


def test_uneven_auto_at_a_julian_date_offset():
    t, x, edges = do.uneven_auto()
    check("uneven auto", t, x, t, x, edges, True, oracle=auto_oracle())
    chunks, size = _cabi.dcf_last_dispatch()
    assert size == _cabi.dcf_chunk(500, 500, 64) and chunks == -(-500 // size)


def test_edge_predicate_under_rounding():
    """The lags of 2450000 + 0.1 i scatter by ulps around the edges 0.1 k: a kernel comparing tb >= ta + edge, or
    taking a quotient, counts differently."""
    t, x, edges = do.rounding_case()
    _, _, o = check("rounding", t, x, t, x, edges, True)
    # (the input does tell the forms apart: the sum form puts some of these pairs into another bin)
    moved = np.sum(t[o.j] < t[o.i] + edges[o.k]) + np.sum(t[o.j] >= t[o.i] + edges[o.k + 1])
    print(f"pairs that tb >= ta + edge bins elsewhere: {moved} of {o.k.size}")
    assert moved > 0


@pytest.mark.parametrize("nlag", [1, 63, 64, 65, 257])
def test_cross_correlation_at_the_lane_seams(nlag):
    ta, a, tb, b, edges = do.cross_case(nlag)
    pairs, _, _ = check(f"cross nlag={nlag}", ta, a, tb, b, edges)
    d = tb[None, :] - ta[:, None]
    assert pairs.sum() == np.sum((d >= edges[0]) & (d < edges[-1]))


def _seam_curve(n):
    rng = np.random.default_rng(100 + n)
    return np.sort(rng.uniform(0, 0.2 * n, n)) + 2450000.0, rng.standard_normal(n)      # (the same density at every n)


@pytest.mark.parametrize("offset", [-1, 0, 1, None])
def test_chunk_seams(offset):
    C = _cabi.dcf_chunk(64, 64, 64)
    assert C <= 256                                     # (small enough for a test of seconds)
    na = 2 * C + 1 if offset is None else C + offset
    assert _cabi.dcf_chunk(na, na, 64) == C
    t, x = _seam_curve(na)
    check(f"na={na}", t, x, t, x, 0.25 * np.arange(65), True)
    assert _cabi.dcf_last_dispatch() == (-(-na // C), C)
    # ... and with another curve across
    tb, b = _seam_curve(150)
    check(f"na={na} cross", t, x, tb, b, np.linspace(-9.0, 9.0, 41))


def test_forced_chunks_same_counts_and_every_sum_in_the_gate():
    t, x, edges = do.uneven_auto()
    seen = {}
    for chunk in (1, 7, 64, 500):
        pairs, sums, _ = check(f"chunk={chunk}", t, x, t, x, edges, True, chunk, oracle=auto_oracle())
        seen[chunk] = _cabi.dcf_last_dispatch()
        assert np.array_equal(pairs, auto_oracle().pairs)
    assert seen == {1: (500, 1), 7: (72, 7), 64: (8, 64), 500: (1, 500)}


def test_two_calls_return_the_same_bytes():
    t, x, edges = do.uneven_auto()
    for chunk in (0, 7, 500):
        first, second = (_cabi.dcf_scan(t, x, t, x, edges, True, chunk) for _ in range(2))
        assert _cabi.dcf_last_dispatch()[0] == {0: 8, 7: 72, 500: 1}[chunk]
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    ta, a, tb, b, edges = do.cross_case(65)
    first, second = (_cabi.dcf_scan(ta, a, tb, b, edges) for _ in range(2))
    assert _cabi.dcf_last_dispatch()[0] >= 3
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def test_the_diagonal_is_the_only_difference():
    t, x, _ = do.uneven_auto()
    edges = -0.185 + 0.37 * np.arange(65)
    with_self, s_with = _cabi.dcf_scan(t, x, t, x, edges, False)
    without, s_without = _cabi.dcf_scan(t, x, t, x, edges, True)
    want = np.zeros(64, dtype=np.int64)
    want[0] = 500                                        # the bin that holds lag 0
    assert np.array_equal(with_self - without, want)
    assert np.array_equal(s_with[:, 1:], s_without[:, 1:])
    do.worst_ratio(with_self, s_with, do.scan(t, x, t, x, edges))


def test_degenerate_shapes():
    rng = np.random.default_rng(8)
    # ties: every time three times
    t = np.repeat(np.sort(rng.uniform(0, 30, 100)), 3)
    x = rng.standard_normal(300)
    check("ties", t, x, t, x, -0.15 + 0.3 * np.arange(41), True)
    check("ties, lag 0 on an edge", t, x, t, x, 0.3 * np.arange(41), True)
    # edges wholly beyond the baseline
    for edges in (40.0 + np.arange(9.0), -50.0 + np.arange(9.0)):
        pairs, sums = _cabi.dcf_scan(t, x, t, x, edges)
        assert not pairs.any() and np.all(sums == 0.0) and not np.signbit(sums).any()
    # bins far narrower than the sampling: mostly empty, some with one pair
    t = np.sort(rng.uniform(0, 50, 200))
    x = rng.standard_normal(200)
    dlag = 1e-3 * np.median(np.diff(t))
    pairs, sums, _ = check("narrow bins", t, x, t, x, 3.0 + dlag * np.arange(513), True)
    assert np.mean(pairs == 0) > 0.5 and np.any(pairs == 1) and np.all(sums[:, pairs == 0] == 0.0)
    # one sample a curve, and none
    one_t, one_x = np.array([5.0]), np.array([2.0])
    pairs, sums = _cabi.dcf_scan(one_t, one_x, np.array([5.5]), np.array([-3.0]), np.array([0.0, 0.5, 1.0]))
    assert pairs.tolist() == [0, 1] and sums[:, 1].tolist() == [2.0, -3.0, 4.0, 9.0, -6.0, 36.0] and np.all(sums[:, 0] == 0)
    pairs, sums = _cabi.dcf_scan(one_t, one_x, one_t, one_x, np.array([-1.0, 1.0]), True)
    assert pairs.tolist() == [0] and np.all(sums == 0.0)
    empty = np.array([])
    for args in ((empty, empty, t, x), (t, x, empty, empty), (empty, empty, empty, empty)):
        pairs, sums = _cabi.dcf_scan(*args, np.arange(5.0))
        assert pairs.shape == (4,) and sums.shape == (6, 4) and not pairs.any() and np.all(sums == 0.0)
        assert _cabi.dcf_last_dispatch()[0] == 0


def test_nan_reaches_the_bins_its_pairs_fall_in_and_no_others():
    ta, a, tb, b, edges = do.cross_case(65)
    clean = do.scan(ta, a, tb, b, edges)
    b_nan = b.copy()
    b_nan[0] = np.nan
    hit = np.zeros(65, dtype=bool)
    hit[clean.k[clean.j == 0]] = True
    assert hit.any() and not hit.all()
    for chunk in (0, 257):
        pairs, sums = _cabi.dcf_scan(ta, a, tb, b_nan, edges, chunk=chunk)
        assert np.array_equal(pairs, clean.pairs)
        for q in (1, 3, 4, 5):                           # Sb, Sbb, Sab, Sabab
            assert np.array_equal(np.isnan(sums[q]), hit)
        bound = do.gate(clean)
        err = np.abs(sums.astype(np.longdouble) - clean.sums)
        assert np.all(err[[0, 2]] <= bound[[0, 2]])      # Sa, Saa: untouched
        assert np.all(err[:, ~hit] <= bound[:, ~hit])
    # ... and a NaN in a: Sa, Saa, Sab, Sabab of the bins sample i has a pair in
    a_nan = a.copy()
    a_nan[200] = np.nan
    hit = np.zeros(65, dtype=bool)
    hit[clean.k[clean.i == 200]] = True
    pairs, sums = _cabi.dcf_scan(ta, a_nan, tb, b, edges)
    assert np.array_equal(pairs, clean.pairs) and hit.any() and not hit.all()
    for q in (0, 2, 4, 5):
        assert np.array_equal(np.isnan(sums[q]), hit)
    assert not np.isnan(sums[[1, 3]]).any()


def test_invalid_arguments_launch_nothing():
    t, x, edges = do.uneven_auto()
    _cabi.dcf_scan(t, x, t, x, edges, True, 100)
    assert _cabi.dcf_last_dispatch() == (5, 100)
    good = dict(ta=t, a=x, tb=t, b=x, edges=edges)
    for kw in (dict(edges=edges[:1]), dict(edges=np.arange((1 << 22) + 2.0)), dict(edges=edges[::-1]),
               dict(edges=np.where(np.arange(65) == 9, edges[8], edges)), dict(edges=np.where(np.arange(65) == 64, np.inf, edges)),
               dict(edges=np.where(np.arange(65) == 3, np.nan, edges)), dict(ta=t[::-1]), dict(tb=t[::-1].copy()),
               dict(ta=np.where(np.arange(500) == 7, np.nan, t)), dict(tb=np.where(np.arange(500) == 499, np.inf, t)),
               dict(tb=t[:-1], b=x[:-1], skip_same_index=True), dict(chunk=-1)):
        with pytest.raises(ValueError):
            _cabi.dcf_scan(**{**good, **kw})
        assert _cabi.dcf_last_dispatch() == (5, 100)
    # what the wrapper cannot say - a negative size, a NULL output, a NULL input - through the entry itself, and the
    # same through its `_dev` twin (which checks before it looks at a pointer: the host arrays stand in)
    for refused in raw.refusals(t, x, edges):
        for entry in (raw.raw_scan, raw.raw_scan_dev):
            with pytest.raises(ValueError):
                entry(**refused)
            assert _cabi.dcf_last_dispatch() == (5, 100)
    # a forced chunk that would make 2^24 chunks or more is refused by its count alone (no array is read before)
    with pytest.raises(ValueError, match="chunks"):
        raw.raw_scan(t, x, t, x, edges, na=1 << 24, nb=1 << 24, skip=1, chunk=1)
    assert _cabi.dcf_last_dispatch() == (5, 100)


def test_dev_twin_returns_the_bytes_of_the_host_entry():
    """``pdc_dcf_scan_dev`` on resident inputs (its own workspace per stream) against ``pdc_dcf_scan``: auto with the
    diagonal left out and the same buffers twice, cross in several chunks, and an empty curve."""
    DB = _cabi.DeviceBuffer
    t, x, edges = do.uneven_auto()
    ta, a, tb, b, cross_edges = do.cross_case(65)
    for args, skip, chunk in (((t, x, t, x, edges), True, 0), ((ta, a, tb, b, cross_edges), False, 7),
                              ((ta, a, tb[:0], b[:0], cross_edges), False, 0)):
        host_pairs, host_sums = _cabi.dcf_scan(*args, skip, chunk)
        host_dispatch = _cabi.dcf_last_dispatch()
        nlag = args[4].size - 1
        bufs = [DB.from_array(v, 0) if v.size else DB(8, 0) for v in args] + [DB(nlag * 8, 0), DB(6 * nlag * 8, 0)]
        try:
            raw.raw_scan_dev(*(buf.ptr for buf in bufs[:5]), na=args[0].size, nb=args[2].size, nlag=nlag, skip=int(skip),
                            chunk=chunk, pairs=bufs[5].ptr, sums=bufs[6].ptr)
            _cabi.check(_cabi.lib().pdc_device_sync(0))
            pairs, sums = bufs[5].to_array(np.int64, nlag), bufs[6].to_array(np.float64, 6 * nlag)
        finally:
            for buf in bufs:
                buf.free()
        assert _cabi.dcf_last_dispatch() == host_dispatch
        assert pairs.tobytes() == host_pairs.tobytes() and sums.tobytes() == host_sums.tobytes()


def test_class_values_are_the_numpy_formulas_on_its_own_sums():
    t, y = do.wandering_sinusoid()
    for err in (None, np.full(400, 0.2)):
        d = DCF()
        out = d(TSeries(t, y), err=err)
        assert np.array_equal(d.lags, 0.0 + np.median(np.diff(t)) * np.arange(d.lags.size)) and out is d.correlogram
        n = d.pairs.astype(float)
        norm = np.sqrt((np.var(y) - (0.0 if err is None else np.mean(err ** 2))) ** 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            dcf = d.sums["Sab"] / (n * norm)
            sigma = np.sqrt(np.maximum(d.sums["Sabab"] / norm ** 2 - n * dcf ** 2, 0)) / (n - 1)
        few = d.pairs < 2
        assert np.array_equal(d.dcf, np.where(few, np.nan, dcf), equal_nan=True)
        assert np.array_equal(d.sigma, np.where(few, np.nan, sigma), equal_nan=True)
        assert np.isfinite(d.dcf).sum() > 0.5 * d.dcf.size
    a = y - np.mean(y)
    do.worst_ratio(d.pairs, np.array([d.sums[name] for name in do.SUMS]), do.scan(t, a, t, a, d.edges, True))
    loc = DCF(max_lag=60.0, dlag=1.0, normalization="local")
    loc(TSeries(t, y))
    n, s = loc.pairs.astype(float), loc.sums
    r = (s["Sab"] / n - (s["Sa"] / n) * (s["Sb"] / n)) / np.sqrt((s["Saa"] / n - (s["Sa"] / n) ** 2) * (s["Sbb"] / n - (s["Sb"] / n) ** 2))
    assert np.array_equal(loc.dcf, r, equal_nan=True) and np.array_equal(loc.sigma, (1 - r ** 2) / np.sqrt(n - 1), equal_nan=True)
    assert np.all(np.abs(r) <= 1)


def test_class_finds_the_period_of_a_phase_wandering_sinusoid():
    t, y = do.wandering_sinusoid()
    d = DCF(max_lag=60.0, dlag=1.0)
    d(TSeries(t, y))
    a = y - np.mean(y)
    o = do.scan(t, a, t, a, d.edges, True)
    want = (o.sums[4] / (o.pairs * np.var(y))).astype(np.float64)
    period, res = do.period_rule(d.lags, want)
    top = np.sort(res["prominences"])[::-1]
    print(f"period {d.period} (oracle {period}), prominence {top[0]:.2f} against {top[1]:.2f}")
    assert d.period == period and abs(d.period - 17.3) <= 1.5
    assert d.peak_lag == float(d.lags[np.nanargmax(want)])
    # a delayed copy: the cross-correlation peaks at the delay
    c = DCF(max_lag=30.0, dlag=1.0)
    c(TSeries(t, y), TSeries(t + 5.0, y))
    assert c.peak_lag == 5.0 and c.dcf[np.flatnonzero(c.lags == 5.0)[0]] > 0.9
    with pytest.raises(ValueError):
        c.period


def test_class_on_an_even_curve_is_the_fft_acf_of_the_reference():
    t, x = do.random_walk(600)
    d = DCF(max_lag=299.0, include_self=True)
    d(TSeries(t, x))
    assert np.array_equal(d.lags, np.arange(300.0)) and np.array_equal(d.pairs, 600 - np.arange(300))
    o = do.scan(t, x - x.mean(), t, x - x.mean(), d.edges)
    allowed = 1e-12 + (do.gate(o)[4] / (o.pairs * np.var(x))).astype(np.float64)
    err = np.abs(d.dcf - do.fft_acf(x, 300))
    print(f"DCF(include_self=True) vs FFT ACF: {err.max():.1e}")
    assert np.all(err <= allowed)
