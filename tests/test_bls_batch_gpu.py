"""BLS.batch: many light curves, each on its own period grid, in one set of launches (csrc/bls_ragged.hip) - against
the single-curve call (bit for bit: the sums are 64-bit integers, so a curve's result does not depend on how its
samples are dealt to workgroups), the long-double oracle (tests/bls_oracle.py) and the host FSeries peak methods."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import bls_oracle as bo
from periodicity_amd import _cabi
from periodicity_amd.core import TSeries
from periodicity_amd.phase import BLS, _pdm_periods
from test_bls_gpu import assert_meets_oracle, y_scale

pytestmark = pytest.mark.gpu

LENGTHS = [9, 10, 11, 31, 64, 255, 256, 257, 1000, 1025, 5000]
PLAIN = 32                                   # curves with a periodogram; then:
NAN_CURVE, CONSTANT_CURVE = 32, 33


def catalogue(seed=5):
    """32 curves - every length in LENGTHS, then random ones (20 .. 3000, log-uniform) - with the time origins and spans
    of test_phase_batch_gpu.catalogue, each a box of depth 1 over 5 % of the phase at span / U(3, 40) plus noise
    err * N(0, 1); err is passed for b % 3 != 0.  Then one curve holding a NaN and one constant curve (256 unit weights:
    its mean is exact, so YY is exactly 0)."""
    rng = np.random.default_rng(seed)
    sigs, errs = [], []
    for b in range(PLAIN + 2):
        n = LENGTHS[b] if b < len(LENGTHS) else int(np.exp(rng.uniform(np.log(20), np.log(3000))))
        if b == CONSTANT_CURVE:
            n = 256
        span = rng.uniform(0.5, 3.0) * n * rng.choice([0.1, 1.0, 10.0])
        t = np.sort(rng.uniform(0.0, span, n)) + rng.choice([-1.0, 1.0]) * rng.uniform(0, 1) * rng.choice([10.0, 1e6])
        period = span / rng.uniform(3.0, 40.0)
        err = rng.uniform(0.5, 1.5, n) * 0.1
        y = 10.0 - ((t / period) % 1 < 0.05) + err * rng.standard_normal(n)
        if b == NAN_CURVE:
            y[n // 2] = np.nan
        if b == CONSTANT_CURVE:
            y[:] = 1.5
        sigs.append(TSeries(t, y))
        errs.append(err if b % 3 != 0 else None)
    return sigs, errs


CAT = catalogue()

# the grids of test_phase_batch_gpu.scans() (the default one at 120 periods), the two histogram shapes
DESCENDING = dict(p_min=50.0, p_max=1.0, n_periods=300)
GRIDS = {"default": dict(n_periods=120), "derived-count": dict(n_periods=None),
         "explicit": dict(p_min=0.7, p_max=55.0, n_periods=700), "descending": DESCENDING}
SHAPES = {"50bins": dict(n_bins=50, q_min=0.02, q_max=0.12), "200bins": dict(),
          "8bins": dict(n_bins=8, q_min=0.1, q_max=0.3)}     # (8 bins, boxes of 1 .. 3: the peak-table test)
ROWS = ("power", "depth", "start_bin", "box_bins", "duration", "transit_time")


@functools.lru_cache(maxsize=None)
def singles(grid, shape, dips_only, min_points=5):
    """The single call on every curve of the catalogue: evaluated once per setting, shared, read only."""
    out = []
    for s, e in zip(*CAT):
        scan = BLS(dips_only=dips_only, min_points=min_points, **GRIDS[grid], **SHAPES[shape])
        fs = scan(s, e)
        one = {name: getattr(scan, name) for name in ROWS}
        one.update(periods=scan.periods, fs=fs, best=scan.best)
        out.append(one)
    return out


def assert_rows_equal(res, b, one, label):
    assert np.array_equal(res.periods[b], one["periods"]), label
    for name in ROWS:
        assert np.array_equal(getattr(res, name)[b], one[name], equal_nan=True), (label, name)
    assert np.array_equal(res.periodograms[b].frequency, one["fs"].frequency), label
    assert np.array_equal(res.periodograms[b].values, one["fs"].values, equal_nan=True), label


def assert_best_equal(res, b, one, label):
    power = one["power"]
    j = int(np.nanargmax(power)) if np.any(~np.isnan(power)) else -1
    assert res.best["index"][b] == j, (label, res.best["index"][b], j)
    for name, want in one["best"].items():
        assert np.array_equal(res.best[name][b], want, equal_nan=True), (label, name, res.best[name][b], want)


@pytest.mark.parametrize("dips_only", [False, True])
@pytest.mark.parametrize("shape", ["50bins", "200bins"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_each_curve_is_bit_identical_to_the_single_call(grid, shape, dips_only):
    sigs, errs = CAT
    res = BLS(dips_only=dips_only, **GRIDS[grid], **SHAPES[shape]).batch(sigs, errs)
    assert res.peaks is None and len(res.periodograms) == len(sigs) == len(res)
    ones = singles(grid, shape, dips_only)
    some = 0
    for b, s in enumerate(sigs):
        scan = BLS(**GRIDS[grid])
        assert np.array_equal(res.periods[b], _pdm_periods(s, scan.p_min, scan.p_max, scan.n_periods, 1)[0])
        assert_rows_equal(res, b, ones[b], (grid, shape, dips_only, b, len(s)))
        assert_best_equal(res, b, ones[b], (grid, shape, dips_only, b, len(s)))
        some += bool(np.any(~np.isnan(ones[b]["power"])))
    assert some >= PLAIN - 4, some            # (the comparison is of periodograms, not of NaN rows)
    for b in (0, NAN_CURVE, CONSTANT_CURVE):  # 9 samples: no box has 5 inside and 5 outside; no periodogram
        assert np.all(np.isnan(res.power[b])) and np.all(np.isnan(res.start_bin[b])) and res.best["index"][b] == -1
        assert all(np.isnan(res.best[name][b]) for name in ("period", "power", "depth", "duration", "transit_time"))


def test_the_catalogue_has_rows_with_and_without_nan():
    """At 50 bins, 120 periods, min_points=5: the 9-sample curve has no box at all, the 10- and 11-sample curves at some
    periods only, the long ones at every period - the three kinds of row the argmax and the peak table have to take."""
    ones = singles("default", "50bins", False)
    nan = [np.isnan(o["power"]) for o in ones[:PLAIN]]
    assert nan[0].all() and all(0 < m.sum() < m.size for m in nan[1:3])
    assert sum(not m.any() for m in nan) >= 24
    assert not any(np.isnan(o["power"]).any() for o in singles("default", "50bins", False, 1)[:PLAIN])


def test_split_route_of_the_single_call_gives_the_same_bits():
    """8192 samples on 4 periods: the single call splits the samples over two workgroups per period through the global
    histogram (bls_auto_slices); the batch bins them in one workgroup."""
    t, y, err = bo.curve(8192, 26)
    small = bo.curve(40, 21)
    kw = dict(n_bins=50, q_min=0.02, q_max=0.1, p_min=3.65, p_max=11.0, n_periods=4)
    res = BLS(**kw).batch([TSeries(t, y), TSeries(small[0], small[1])], [err, small[2]])
    for b, (tt, yy, ee) in enumerate(((t, y, err), small)):
        scan = BLS(**kw)
        fs = scan(TSeries(tt, yy), ee)
        one = {name: getattr(scan, name) for name in ROWS}
        one.update(periods=scan.periods, fs=fs, best=scan.best)
        assert_rows_equal(res, b, one, b)
        assert_best_equal(res, b, one, b)
    assert np.all(~np.isnan(res.power[0])) and res.power[0].size == 4


@pytest.mark.parametrize("count,ascending", [(4, True), (193, True), (769, True), (193, False)])
def test_first_of_equal_maxima_wins(count, ascending):
    """Integer times and a dip at t % 3 == 0: at the periods 0.75, 1.5 and 3.0 (exact members of linspace(0.75, 3, count)
    for these counts: the step is a dyadic fraction) every quotient is the quotient at period 3 times 4, 2, 1 - an exact
    scaling - so the phases fall in the same bins, the histograms are equal and so are the bits of the power.  The three
    sit in one thread's stride (769), in three waves (193) and in neighbouring lanes (4) of the argmax."""
    rng = np.random.default_rng(3)
    t = np.arange(240.0)
    y = 10.0 - (t % 3 == 0) + 0.01 * rng.standard_normal(240)
    lo, hi = (0.75, 3.0) if ascending else (3.0, 0.75)
    kw = dict(n_bins=8, q_min=0.1, q_max=0.3, p_min=lo, p_max=hi, n_periods=count, min_points=5)
    filler, errs = CAT[0][5], CAT[1][5]
    res = BLS(**kw).batch([filler, TSeries(t, y), filler], [errs, None, errs])
    scan = BLS(**kw)
    scan(TSeries(t, y))
    ties = [0, (count - 1) // 3 if ascending else 2 * (count - 1) // 3, count - 1]
    assert scan.periods[ties].tolist() == ([0.75, 1.5, 3.0] if ascending else [3.0, 1.5, 0.75])
    top = np.nanmax(scan.power)
    assert np.all(scan.power[ties] == top) and int(np.nanargmax(scan.power)) == 0
    exact = bo.scan(t, y, None, scan.periods[ties], 8, 1, 3, 5).power()   # the oracle confirms the tie
    assert exact[0] == exact[1] == exact[2]
    assert np.array_equal(res.power[1], scan.power, equal_nan=True)
    assert res.best["index"][1] == 0 and res.best["period"][1] == lo and res.best["power"][1] == top
    assert res.best["depth"][1] == scan.depth[0] and res.best["transit_time"][1] == scan.transit_time[0]


def test_oracle_rows():
    """Rows of 31, 257, 1025 and 5000 samples against the longdouble oracle under the single call's derived gate,
    1e-9 |exact| + 1e-11."""
    sigs, errs = CAT
    res = BLS(n_bins=50, q_min=0.02, q_max=0.12, n_periods=120).batch(sigs, errs)
    for b in (3, 7, 9, 10):
        s, e = sigs[b], errs[b]
        assert len(s) in (31, 257, 1025, 5000)
        sc = bo.scan(s.time, s.values, e, res.periods[b], 50, 1, 6, 5)
        ints = [np.where(np.isnan(a), -1, a).astype(np.int32) for a in (res.start_bin[b], res.box_bins[b])]
        assert_meets_oracle(f"batch row {b} N={len(s)}", (res.power[b], res.depth[b], *ints), sc, False,
                            y_scale(s.time, s.values, e))


def half_max_pair(fs, rank, by_prominence):
    try:
        return fs.periods_at_half_max(rank + 1, use_prominence=by_prominence)
    except IndexError:
        return None


TABLE = ("count", "index", "height", "prominence", "period", "period_lo", "period_hi")


@pytest.mark.parametrize("grid", ["default", "descending"])
@pytest.mark.parametrize("by_prominence", [False, True])
@pytest.mark.parametrize("k", [1, 4, 200])
def test_peak_table_matches_the_host_methods(k, by_prominence, grid):
    """min_points=1 leaves no NaN in a row of the default grid: every curve's table against find_peaks, psort_by_* and
    periods_at_half_max of the single call's FSeries; rows whose ranked keys tie are compared as sets.  At 8 bins: with
    min_points=1 and many bins the best box of a sparse curve is one outlying sample alone in its bins, the same power at
    many periods, and nearly every row has tied peaks (50 bins: 28 of 32 rows); 8 bins leave 20 or more rows without a
    tie on either grid (counted with the oracle).  On the descending grid (periods 50 .. 1) three short curves fold into
    one bin at some periods; their rows hold NaN and are left to test_peak_table_with_nan_in_the_rows."""
    sigs, errs = CAT[0][:PLAIN], CAT[1][:PLAIN]
    lean = BLS(min_points=1, **SHAPES["8bins"], **GRIDS[grid]).batch(sigs, errs, peaks=k, by_prominence=by_prominence,
                                                                   want_power=False)
    assert lean.periodograms is None and lean.power is None
    tab = lean.peaks
    assert tab.index.shape == (len(sigs), k)
    ones = singles(grid, "8bins", False, 1)
    ordered = as_sets = with_nan = 0
    for b in range(len(sigs)):
        fs = ones[b]["fs"]
        assert_best_equal(lean, b, ones[b], (grid, b))
        if np.any(np.isnan(fs.values)):
            with_nan += 1
            continue
        found = fs.find_peaks()
        c = len(found)
        assert tab.count[b] == c
        top = min(k, c)
        assert np.all(tab.index[b, top:] == -1) and np.all(np.isnan(tab.height[b, top:]))
        if c == 0:
            continue
        idx = tab.index[b, :top]
        assert np.array_equal(tab.period[b, :top], fs.period[idx])
        assert np.array_equal(tab.height[b, :top], fs.values[idx])
        key = found.attrs["prominences"] if by_prominence else found.values
        ranked = np.sort(key)[::-1]
        if len(np.unique(key)) < len(key):
            got_key = tab.prominence[b, :top] if by_prominence else tab.height[b, :top]
            assert np.array_equal(got_key, ranked[:top])
            pos = np.searchsorted(found.attrs["indices"], idx)
            assert np.array_equal(found.attrs["indices"][pos], idx) and np.array_equal(key[pos], got_key)
            as_sets += 1
            continue
        want = fs.psort_by_prominence() if by_prominence else fs.psort_by_peak()
        assert np.array_equal(tab.period[b, :top], want[:top])
        for r in list(range(min(top, 6))) + ([top - 1] if top > 6 else []):
            pair = half_max_pair(fs, r, by_prominence)
            lo, hi = tab.period_lo[b, r], tab.period_hi[b, r]
            if pair is None:
                assert np.isnan(lo) or np.isnan(hi), (b, r)
            else:
                assert (lo, hi) == pair, (b, r)
        ordered += 1
    assert ordered >= len(sigs) // 2, (ordered, as_sets, with_nan)
    assert with_nan == 0 or grid == "descending"
    print(f"BLS {grid} k={k} by_prominence={by_prominence}: {ordered} curves compared rank by rank, {as_sets} with tied "
          f"extrema as sets, {with_nan} rows with NaN left to the flat-row comparison")


@pytest.mark.parametrize("grid", ["default", "descending"])
@pytest.mark.parametrize("by_prominence", [False, True])
@pytest.mark.parametrize("k", [1, 4, 200])
def test_peak_table_with_nan_in_the_rows(k, by_prominence, grid):
    """min_points=5: rows that are NaN at some periods, or at all of them, and the pad of the pitched copy.  The table is
    pdc_peaks_topk's on the single call's FSeries values - the same kernel on a flat row - so the bits are equal."""
    sigs, errs = CAT
    lean = BLS(n_bins=50, q_min=0.02, q_max=0.12, **GRIDS[grid]).batch(sigs, errs, peaks=k, by_prominence=by_prominence,
                                                                      want_power=False)
    tab = lean.peaks
    ones = singles(grid, "50bins", False)
    with_nan = 0
    for b in range(len(sigs)):
        fs = ones[b]["fs"]
        flat = _cabi.peaks_topk(fs.values, k, by_prominence)
        with_nan += bool(np.isnan(fs.values).any())
        assert tab.count[b] == flat["count"][0], b
        assert np.array_equal(tab.index[b], flat["indices"][0]), b
        assert np.array_equal(tab.height[b], flat["heights"][0], equal_nan=True), b
        assert np.array_equal(tab.prominence[b], flat["prominences"][0], equal_nan=True), b
        for name, col in (("period", "indices"), ("period_lo", "half_lo"), ("period_hi", "half_hi")):
            at = flat[col][0]
            want = np.where(at >= 0, fs.period[np.maximum(at, 0)], np.nan)
            assert np.array_equal(getattr(tab, name)[b], want, equal_nan=True), (b, name)
        assert_best_equal(lean, b, ones[b], (grid, b))
    assert with_nan >= 5


def test_peaks_with_and_without_power():
    sigs, errs = CAT
    full = BLS(n_periods=120).batch(sigs, errs, peaks=5)
    lean = BLS(n_periods=120).batch(sigs, errs, peaks=5, want_power=False)
    for name in TABLE:
        assert np.array_equal(getattr(full.peaks, name), getattr(lean.peaks, name), equal_nan=True), name
    for name in full.best:
        assert np.array_equal(full.best[name], lean.best[name], equal_nan=True), name
    ones = singles("default", "200bins", False)
    for b in range(len(sigs)):
        assert_rows_equal(full, b, ones[b], b)


def same_result(a, b):
    for name in ROWS:
        for ra, rb in zip(getattr(a, name), getattr(b, name)):
            assert np.array_equal(ra, rb, equal_nan=True), name
    for name in a.best:
        assert np.array_equal(a.best[name], b.best[name], equal_nan=True), name
    for name in TABLE:
        assert np.array_equal(getattr(a.peaks, name), getattr(b.peaks, name), equal_nan=True), name


def on_slots(devices, **kw):
    scan = BLS(**kw)
    scan.devices = devices
    return scan


def test_device_slots_are_bit_identical_and_cached():
    sigs, errs = CAT
    kw = dict(n_bins=50, q_min=0.02, q_max=0.12, n_periods=120)
    one = BLS(device=0, **kw).batch(sigs, errs, peaks=3)
    three = on_slots((0, 0, 0), **kw).batch(sigs, errs, peaks=3)
    same_result(one, three)
    before = _cabi.alloc_counts()
    again = on_slots((0, 0, 0), **kw).batch(sigs, errs, peaks=3)
    assert _cabi.alloc_counts() == before
    same_result(one, again)
    same_result(one, on_slots((0,) * 5, **kw).batch(sigs, errs, peaks=3))


BUDGET_CHILD = r"""
import pickle, sys
sys.path.insert(0, sys.argv[1] + "/tests")
from periodicity_amd import _cabi
from test_bls_batch_gpu import budget_catalogue, ROWS, TABLE
from periodicity_amd.phase import BLS
sigs, errs = budget_catalogue()
out = {}
try:
    r = BLS(n_periods=1000).batch(sigs, errs, peaks=4)
    out["groups"] = _cabi.bls_ragged_groups()
    out["rows"] = {k: getattr(r, k) for k in ROWS}
    out["best"] = r.best
    out["table"] = {k: getattr(r.peaks, k) for k in TABLE}
except ValueError as e:
    out["error"] = str(e)
sys.stdout.buffer.write(pickle.dumps(out))
"""


def budget_catalogue():
    """Without the 5000-sample curve: a group is a run of whole curves, and that one alone is a quarter of the bytes."""
    sigs, errs = CAT
    return sigs[:10] + sigs[11:], errs[:10] + errs[11:]


def run_child(budget_gb):
    """One batch in a child process, so that PDC_WORK_BUDGET_GB (read once per process) reaches no other test."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("PDC_WORK_BUDGET_GB", None)
    if budget_gb is not None:
        env["PDC_WORK_BUDGET_GB"] = repr(budget_gb)
    proc = subprocess.run([sys.executable, "-c", BUDGET_CHILD, root], env=env, capture_output=True, timeout=600, cwd=root)
    assert proc.returncode == 0, proc.stderr.decode()[-2000:]
    return pickle.loads(proc.stdout)


def test_budget_groups_are_bit_identical():
    ref = run_child(None)
    sigs, errs = budget_catalogue()
    n, p = sum(len(s) for s in sigs), 1000 * len(sigs)
    # inputs t, y, dy | the workspace with the four rows in it
    whole = 3 * 8 * n + _cabi.lib().pdc_bls_ragged_work_bytes(len(sigs), n, p, 0, 0)
    small = run_child(whole / 6 / 2 ** 30)
    assert ref["groups"] == 1 and small["groups"] >= 3, (ref.get("groups"), small)
    for name in ROWS:
        for a, b in zip(ref["rows"][name], small["rows"][name]):
            assert np.array_equal(a, b, equal_nan=True), name
    for part in ("best", "table"):
        for key, a in ref[part].items():
            assert np.array_equal(a, small[part][key], equal_nan=True), (part, key)
    assert "budget" in run_child(1e-9).get("error", "")


def test_edges():
    sigs, errs = CAT
    # an empty curve between two others: an empty row, -1 / NaN, and the neighbours untouched
    kw = dict(n_bins=50, q_min=0.02, q_max=0.12, n_periods=120)
    res = BLS(**kw).batch([sigs[7], TSeries(np.empty(0), np.empty(0)), sigs[8]], [errs[7], None, errs[8]], peaks=2)
    ones = singles("default", "50bins", False)
    assert_rows_equal(res, 0, ones[7], 0)
    assert_rows_equal(res, 2, ones[8], 2)
    assert res.power[1].size == 0 and res.best["index"].tolist()[1] == -1 and np.isnan(res.best["power"][1])
    assert res.peaks.count[1] == 0 and np.all(res.peaks.index[1] == -1)
    assert res.peaks.count[0] == len(ones[7]["fs"].find_peaks())
    # ... also through the library with a grid of its own: NaN / -1 at every period
    t, y = np.asarray(sigs[7].time), np.asarray(sigs[7].values)
    rows, best, _ = _cabi.bls_scan_ragged(t, y, None, [0, 0, t.size], [1.0, 2.0], [0.5, 0.25], [3.0, 4.0], [0, 5, 14], 50, 1,
                                          6)
    assert np.all(np.isnan(rows["power"][:5])) and np.all(rows["start_bin"][:5] == -1) and best["index"][0] == -1
    assert np.isnan(best["power"][0]) and best["start_bin"][0] == -1 and np.any(~np.isnan(rows["power"][5:]))
    # a one-period grid
    kw1 = dict(n_bins=50, q_min=0.02, q_max=0.12, p_min=7.0, p_max=9.0, n_periods=1)
    res = BLS(**kw1).batch(sigs[8:10], errs[8:10])
    for b in (0, 1):
        scan = BLS(**kw1)
        scan(sigs[8 + b], errs[8 + b])
        assert scan.periods.tolist() == [7.0] and np.array_equal(res.periods[b], scan.periods)
        assert np.array_equal(res.power[b], scan.power) and res.best["index"][b] == 0
        assert res.best["depth"][b] == scan.best["depth"] and res.best["period"][b] == 7.0
    # the largest histogram: 2048 bins, boxes of 20 .. 205
    t, y, err = bo.curve(3000, 25)
    big = BLS(n_bins=2048, n_periods=16)
    assert big.box_lengths() == (20, 205)
    res = big.batch([TSeries(t, y)], [err])
    big(TSeries(t, y), err)
    assert np.array_equal(res.power[0], big.power, equal_nan=True) and np.any(~np.isnan(big.power))
    assert np.array_equal(res.depth[0], big.depth, equal_nan=True)
    assert np.array_equal(res.start_bin[0], big.start_bin, equal_nan=True)
    assert res.best["period"][0] == big.best["period"] and res.best["transit_time"][0] == big.best["transit_time"]


def test_a_rejected_call_allocates_nothing():
    sigs, errs = CAT
    _cabi.lib().pdc_release()
    before = _cabi.alloc_counts()
    t, y = np.asarray(sigs[7].time), np.asarray(sigs[7].values)
    good = dict(offsets=[0, 100, t.size], start=[1.0, 2.0], step=[0.5, 0.25], stop=[3.0, 4.0], p_offsets=[0, 5, 14],
                n_bins=50, len_min=1, len_max=6, min_points=5)
    for bad in (dict(n_bins=1), dict(len_max=50), dict(min_points=0), dict(offsets=[0, 300, t.size]),
                dict(p_offsets=[0, 15, 14])):
        for k in (0, 3):
            with pytest.raises(ValueError):
                _cabi.bls_scan_ragged(t, y, None, k=k, **dict(good, **bad))
    assert _cabi.alloc_counts() == before
    rows, best, _ = _cabi.bls_scan_ragged(t, y, None, **good)
    assert np.any(~np.isnan(rows["power"])) and _cabi.alloc_counts() != before
