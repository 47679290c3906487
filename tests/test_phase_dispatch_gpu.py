"""Every route of the phase-binning dispatcher (``phase_route`` / ``phase_stat_dev`` in csrc/pdm.hip) at the smallest
shape that reaches it, for PDM theta, AoV, conditional entropy and Gregory-Loredo.

The dispatcher picks an unsplit instance of ``pdm_scan_kernel`` by period count and histogram size, or the split mode
with a slice count from one of three rules; the rounds-filled score may decline to split and ``PDC_PDM_SPLIT`` /
``PDC_PDM_NZ`` change the outcome.  So every case first runs the scan through the public binding in a child interpreter
whose environment holds exactly the switches the case names, then asserts that the record of the launch
(``pdc_test_phase_last_dispatch``) equals the plan (``pdc_test_phase_shape``) AND is the route the case is here for, and
only then looks at the numbers:

* every period (case 2: a strided sample) against the C oracle (``oracle/scan_oracle.c``: numpy's exact bin rule),
  rtol 1e-9 for all four statistics, atol 1e-13 for the conditional entropy and 1e-9 for Gregory-Loredo as in
  tests/test_aov_ce_gpu.py;
* equal NaN masks, the same index of the optimum, the same bits on a repeated call;
* split and unsplit results of one input agree to rtol 1e-12.

The hook only observes: no case takes a route that the switches would not give a user.  Each case prints its route and
its largest relative error before it asserts (``-s``; profiles/r29_phase_dispatch_parity.txt holds one run).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import scan_oracle as so

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PDM, AOV, CE, GL = 0, 1, 2, 4
NAME = {PDM: "pdm", AOV: "aov", CE: "ce", GL: "gl"}
RTOL = 1e-9
ATOL = {PDM: 0.0, AOV: 0.0, CE: 1e-13, GL: 1e-9}
JD = 2454900.5
# one small histogram per kind, (nb, nc) as pdc_phase_scan_dev takes them: PDM 5 x 2, AoV 10 bins, conditional entropy
# 10 x 5 cells, Gregory-Loredo m = 6 with 4 offsets
SMALL = {PDM: (5, 2), AOV: (10, 1), CE: (10, 5), GL: (24, 6)}

_CHILD = r"""
import json, sys
import numpy as np
from periodicity_amd import _cabi
spec = json.load(open(sys.argv[1]))
data = np.load(sys.argv[2])
out = {}
def scan(c):
    t, p = data[c["t"]], data[c["periods"]][:c["P"]]
    kind, nb, nc = c["kind"], c["nb"], c["nc"]
    if kind == 0:
        return _cabi.pdm_scan(t, data[c["x"]], p, nb, nc, c["sigma"])
    if kind == 1:
        return _cabi.aov_scan(t, data[c["x"]], p, nb)
    if kind == 2:
        return _cabi.cond_entropy_scan(t, data[c["x"]], p, nb, nc)
    return _cabi.gl_scan(t, p, nc, nb // nc)
for c in spec:
    k = c["name"]
    if "batch" in c:    # PDM / AOV .batch on short curves against the single calls (pdm_ragged.hip::shape_of)
        from periodicity_amd import phase
        from periodicity_amd.core import TSeries
        sigs = [TSeries(data[f"{k}_t{i}"], data[f"{k}_x{i}"]) for i in range(c["batch"])]
        make = lambda: getattr(phase, c["cls"])(*c["args"], p_min=2.0, p_max=40.0, n_periods=c["P"])
        res = make().batch(sigs)
        same, recs = [], []
        for i, s in enumerate(sigs):
            single = make()
            one = single(s)
            recs.append(_cabi.phase_last_dispatch())
            same.append(bool(np.array_equal(res.periodograms[i].values, one.values, equal_nan=True)))
            out[f"{k}_periods{i}"] = single.periods           # ascending; the periodogram is in frequency order
            out[f"{k}_one{i}"] = one.values[::-1]
        out[k + "_same"] = np.array(same)
        out[k + "_rec"] = json.dumps(recs)
        continue
    got = scan(c)
    out[k + "_rec"] = json.dumps(_cabi.phase_last_dispatch())
    out[k + "_plan"] = json.dumps(_cabi.phase_shape(c["kind"], data[c["t"]].size, c["P"], c["nb"], c["nc"]))
    out[k + "_same_bits"] = np.array_equal(got, scan(c), equal_nan=True)
    out[k] = got
np.savez(sys.argv[3], **out)
print("ok")
"""


def run_child(tmp_path, tag, env, cases, arrays):
    """One fresh interpreter with the ``PDC_PDM_*`` switches of ``env`` (and no others): every case's scan, its repeat
    and the hook's record and plan come back in an npz.  Children run one at a time."""
    spec, inp, res = (str(tmp_path / f"{tag}.{ext}") for ext in ("json", "in.npz", "out.npz"))
    with open(spec, "w") as fh:
        json.dump(cases, fh)
    np.savez(inp, **arrays)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PDC_PDM_")}
    clean.update({k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, "-c", _CHILD, spec, inp, res], env=clean, cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stderr[-2000:])
    return np.load(res)


def case(name, kind, t, periods, P, nbc, x=None, sigma=1.0):
    return dict(name=name, kind=kind, t=t, x=x, periods=periods, P=int(P), nb=nbc[0], nc=nbc[1], sigma=float(sigma))


def route_of(rec):
    """The kernel instance a record names: ``<BLOCK,SPLIT>`` unsplit, ``<256,4,ZS>xN`` in split mode with N slices."""
    if rec["split"]:
        return f"<{rec['block']},{rec['waves']},ZS>x{rec['n_z']}"
    return f"<{rec['block']},{rec['waves']}>"


def check_route(res, c, route, **want):
    """The launch's record equals the plan asked of the same process and is the route this case is here for."""
    rec, plan = json.loads(str(res[c["name"] + "_rec"])), json.loads(str(res[c["name"] + "_plan"]))
    assert rec == plan, (c["name"], rec, plan)
    assert rec["kind"] == c["kind"] and route_of(rec) == route, (c["name"], route, rec)
    assert rec["periods_per_wg"] * rec["waves"] == rec["block"] and rec["workgroups"] == -(-c["P"] // rec["periods_per_wg"])
    assert {k: rec[k] for k in want} == want, (c["name"], want, rec)
    assert bool(res[c["name"] + "_same_bits"]), c["name"]
    return rec


def oracle(kind, t, x, periods, nbc, sigma=1.0):
    nb, nc = nbc
    if kind == PDM:
        return co.pdm_scan(t, x, periods, nb, nc, sigma)
    if kind == AOV:
        return co.aov_scan(t, x, periods, nb)
    if kind == CE:
        return co.cond_entropy_scan(t, x, periods, nb, nc)
    return co.gl_scan(t, periods, nc, nb // nc)


def check_values(kind, got, want, label, route):
    """Equal NaN masks, every value within the statistic's tolerance, the optimum at the same index."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, label
    nan = np.isnan(want)
    big = ~nan & (np.abs(want) > 10 * ATOL[kind])
    rel = np.max(np.abs(got[big] - want[big]) / np.abs(want[big])) if big.any() else 0.0
    err = np.max(np.abs(got[~nan] - want[~nan])) if (~nan).any() else 0.0
    print(f"PHASE-DISPATCH {NAME[kind]} {label} route {route} periods {want.size} NaN {int(nan.sum())} "
          f"max rel err {rel:.3e} max abs err {err:.3e}")
    assert np.array_equal(np.isnan(got), nan), (label, int(np.isnan(got).sum()), int(nan.sum()))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL[kind], err_msg=label)
    if not nan.all():
        arg = np.nanargmax if kind in (AOV, GL) else np.nanargmin
        assert int(arg(got)) == int(arg(want)), label


def curve(n, seed, period=13.7, t_shift=0.0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, float(n), n)) + t_shift
    dy = rng.uniform(0.05, 0.2, n)
    return t, 1.0 + 0.5 * np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)


def values_of(kind, x):
    """What the scan takes beside the times: the curve, its magnitude bins (conditional entropy), nothing."""
    if kind == CE:
        return so.magnitude_bins(x, SMALL[CE][1])
    return None if kind == GL else x


def sigma_of(kind, x):
    return float(np.var(x, ddof=1)) if kind == PDM else 1.0


# ---- 1. <256, 2> and <256, 1>: the unsplit instances of long period grids ------------------------------------------
# 131 009 periods are 2048 groups of 64: <256, 2>, 1024 workgroups of 128, the last one with 65 periods (its second
# wave pair holds one).  262 080 = 4095 groups: still <256, 2>, the last of 2048 workgroups holds 64 periods (its
# second wave pair none).  262 081 = 4096 groups: <256, 1>, 1024 workgroups of 256, the last one with 193.
# One grid of 262 081 periods; the shorter grids are its prefixes, so one oracle call serves the three launches.
LADDER = ((131_009, "<256,2>"), (262_080, "<256,2>"), (262_081, "<256,1>"))
# commensurate periods of the evenly sampled curve at both ends of workgroups of every instance and at the grids' ends
COMMENSURATE = {0: 1.0, 63: 2.0, 64: 2.5, 127: 4.0, 128: 5.0, 255: 12.5, 256: 25.0, 131_007: 50.0,
                131_008: 3.0000000000000004, 262_079: 10.0, 262_080: 6.25}


def long_grid():
    periods = np.linspace(1.0, 60.0, 262_081)
    for i, p in COMMENSURATE.items():
        periods[i] = p
    return periods


def ladder_curve(which):
    """n = 387: two chunks, the second with 131 samples - part 0 of SPLIT = 2 takes a full half (128), part 1 three.
    n = 300: the second chunk has 44 samples, part 1 none."""
    if which == "jd":         # Julian dates; a NaN time stamp in part 1 of the first chunk: q_nan through the part fold
        t, x = curve(387, 1)
        t = t + JD
        t[200] = np.nan
    elif which == "neg":      # a negative origin
        t, x = curve(300, 2, t_shift=-12345.5)
    elif which == "even":     # evenly sampled: phases on bin edges; the two tiny negatives fold to phi == 1.0 exactly
        t = np.concatenate([[-1e-300, -1e-18], np.arange(385.0)])
        x = np.sin(2 * np.pi * t / 12.5) + 0.1 * np.cos(t)
    else:                     # "nanx": a NaN value as well - the mean is NaN, and so is every theta (PDM, AoV)
        t, x = curve(387, 3)
        t = t + JD
        t[200] = np.nan
        x[130] = np.nan
    return t, x


LADDER_CASES = [(kind, which) for kind in SMALL for which in ("jd", "neg", "even")] + [(PDM, "nanx"), (AOV, "nanx")]


@pytest.mark.parametrize("kind,which", LADDER_CASES, ids=[f"{NAME[k]}-{w}" for k, w in LADDER_CASES])
def test_two_and_one_wave_per_period_group(tmp_path, kind, which):
    t, x = ladder_curve(which)
    periods = long_grid()
    v, sigma = values_of(kind, x), sigma_of(kind, x)
    arrays = {"t": t, "periods": periods}
    if v is not None:
        arrays["x"] = v
    cases = [case(f"p{P}", kind, "t", "periods", P, SMALL[kind], "x", sigma) for P, _ in LADDER]
    res = run_child(tmp_path, "ladder", {}, cases, arrays)
    want = oracle(kind, t, v, periods, SMALL[kind], sigma)
    if which == "nanx":
        assert np.isnan(want).all()
    for c, (P, route) in zip(cases, LADDER):
        check_route(res, c, route, split=0, n_z=1, finish_lds=0)
        check_values(kind, res[c["name"]], want[:P], f"n={t.size} P={P} {which}", route)


# ---- 2. the same instances with many chunks ------------------------------------------------------------------------
def strided(P, per_wg):
    """At most 4096 periods: a stride over the grid, its first and last index, and both ends of four workgroups."""
    wgs = -(-P // per_wg)
    ends = [i for w in (0, 1, wgs // 2, wgs - 1) for i in (w * per_wg, min((w + 1) * per_wg, P) - 1)]
    pick = np.unique(np.concatenate([np.arange(0, P, -(-P // 4000)), ends, [0, P - 1]]))
    assert pick.size <= 4096 and pick[0] == 0 and pick[-1] == P - 1 and len(set(ends)) >= 6
    return pick


@pytest.mark.parametrize("kind", list(SMALL), ids=[NAME[k] for k in SMALL])
def test_many_chunks_where_the_score_declines_to_split(tmp_path, kind):
    """n = 8192 opens the split mode, 2048 (4096) period groups go to the rounds-filled score, and the score keeps the
    unsplit <256, 2> (<256, 1>) launch, which fills exactly one round: 32 full chunks per workgroup.  Gregory-Loredo's
    small histogram (8 workgroups per CU) makes the same score take ONE slice in split mode there - asserted as such -
    and reaches the two instances with 31 chunks and 255 samples at n = 8191."""
    t, x = curve(8192, 4, t_shift=JD)
    periods = long_grid()
    v, sigma = values_of(kind, x), sigma_of(kind, x)
    shapes = [(8192, 131_009, "<256,2>"), (8192, 262_081, "<256,1>")]
    if kind == GL:
        shapes = [(8191, 131_009, "<256,2>"), (8191, 262_081, "<256,1>"), (8192, 131_009, "<256,4,ZS>x1")]
    arrays, cases = {"periods": periods}, []
    for n, P, _ in shapes:
        arrays[f"t{n}"] = t[:n]
        if v is not None:
            arrays[f"x{n}"] = v[:n]
        cases.append(case(f"n{n}_p{P}", kind, f"t{n}", "periods", P, SMALL[kind], f"x{n}", sigma))
    res = run_child(tmp_path, "chunks", {}, cases, arrays)
    for c, (n, P, route) in zip(cases, shapes):
        rec = check_route(res, c, route)
        pick = strided(P, rec["periods_per_wg"])
        want = oracle(kind, t[:n], None if v is None else v[:n], periods[pick], SMALL[kind], sigma)
        check_values(kind, res[c["name"]][pick], want, f"n={n} P={P} ({pick.size} of the periods)", route)


# ---- 3. AoV beyond 47 bins: <64, 1, false, 1> ----------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [48, 100])
def test_aov_with_one_wave_per_workgroup(tmp_path, n_bins):
    t, x = curve(2000, 5, t_shift=JD)
    periods = np.linspace(1.0, 60.0, 300)
    cases = [case(f"p{P}", AOV, "t", "periods", P, (n_bins, 1), "x") for P in (1, 64, 65, 300)]
    res = run_child(tmp_path, "aov64", {}, cases, {"t": t, "x": x, "periods": periods})
    want = co.aov_scan(t, x, periods, n_bins)
    for c in cases:
        check_route(res, c, "<64,1>", split=0, workgroups=-(-c["P"] // 64))
        check_values(AOV, res[c["name"]], want[:c["P"]], f"n=2000 P={c['P']} {n_bins} bins", "<64,1>")


# ---- 4. the largest histogram of 256 threads (47 fine bins, 152 008 B) against the first of 64 (48) ------------------
BOUNDARY = [(PDM, (47, 1)), (PDM, (48, 1)), (AOV, (47, 1)), (AOV, (48, 1))]


@pytest.mark.parametrize("kind,nbc", BOUNDARY, ids=[f"{NAME[k]}{b[0]}" for k, b in BOUNDARY])
def test_histogram_boundary_unsplit_and_split(tmp_path, kind, nbc):
    """n = 3000 x 130 periods: unsplit on either side.  n = 9000 x 64 periods: 47 bins go through split mode with the
    152 008-byte scan kernel (4 slices of 2304), 48 bins stay unsplit on <64, 1>."""
    t, x = curve(9000, 6, t_shift=JD)
    periods = np.linspace(1.0, 60.0, 130)
    sigma = sigma_of(kind, x)
    fits = nbc[0] == 47
    shapes = [(3000, 130, "<256,4>" if fits else "<64,1>"), (9000, 64, "<256,4,ZS>x4" if fits else "<64,1>")]
    arrays, cases = {"periods": periods}, []
    for n, P, _ in shapes:
        arrays.update({f"t{n}": t[:n], f"x{n}": x[:n]})
        cases.append(case(f"n{n}", kind, f"t{n}", "periods", P, nbc, f"x{n}", sigma))
    res = run_child(tmp_path, "boundary", {}, cases, arrays)
    for c, (n, P, route) in zip(cases, shapes):
        rec = check_route(res, c, route, scan_lds=152_008 if fits else 42_192)
        assert not (fits and n == 9000) or (rec["z_len"], rec["finish_lds"]) == (2304, 49_152)
        check_values(kind, res[c["name"]], oracle(kind, t[:n], x[:n], periods[:P], nbc, sigma),
                     f"n={n} P={P} {nbc[0]} bins", route)


@pytest.mark.parametrize("cls,args", [("PDM", (47, 1)), ("PDM", (48, 1)), ("AOV", (47,)), ("AOV", (48,))],
                         ids=["pdm47", "pdm48", "aov47", "aov48"])
def test_histogram_boundary_in_a_batch(tmp_path, cls, args):
    """The ragged batch switches its kernel at the same boundary (pdm_ragged.hip::shape_of): three short curves in one
    batch give the bits of three single calls, whose own routes are asserted, and the oracle's values."""
    kind = PDM if cls == "PDM" else AOV
    arrays = {}
    for i, n in enumerate((600, 1500, 2500)):
        arrays[f"b_t{i}"], arrays[f"b_x{i}"] = curve(n, 60 + i, t_shift=-300.0)
    res = run_child(tmp_path, "batch", {}, [dict(name="b", batch=3, cls=cls, args=list(args), P=130)], arrays)
    assert res["b_same"].all(), res["b_same"]
    route = "<256,4>" if args[0] == 47 else "<64,1>"
    for i, rec in enumerate(json.loads(str(res["b_rec"]))):
        assert rec["kind"] == kind and route_of(rec) == route, rec
        t, x = arrays[f"b_t{i}"], arrays[f"b_x{i}"]
        want = oracle(kind, t, x, res[f"b_periods{i}"], (args[0], 1), sigma_of(kind, x))
        check_values(kind, res[f"b_one{i}"], want, f"batch curve {i} (n={t.size}) {args[0]} bins", route)


# ---- 5. the counts-only kinds in split mode with many cells ----------------------------------------------------------
# pdm_finish_kernel unpacks two 16-bit cells per word; an odd cell count leaves the high half of the last word unused.
# Conditional entropy at (18, 10): 190 cells; at (190, 1): 191 - but with ONE magnitude bin the entropy is 0 at every
# period, so that case checks the launch and its zeros only; (62, 3) has an odd count (189) and real values.
# Gregory-Loredo with m = 10 and 19 offsets bins 190 fine bins + the overflow bin: 191 cells, the limit, with real values.
MANY_CELLS = [(CE, (18, 10)), (CE, (190, 1)), (CE, (62, 3)), (GL, (190, 10))]


@pytest.mark.parametrize("kind,nbc", MANY_CELLS, ids=[f"{NAME[k]}{b[0]}x{b[1]}" for k, b in MANY_CELLS])
def test_counts_only_split_mode_with_many_cells(tmp_path, kind, nbc):
    """n = 9000 x 64 periods: 4 slices of 2304.  n = 66 000 x 33 periods: more than one workgroup's 65 280 samples; one
    period group asks for 1024 slices and gets 66 000 // 2048 = 32 of 2304 samples, which makes 29."""
    t, x = curve(66_000, 7, period=9.1, t_shift=JD)
    mag = so.magnitude_bins(x, nbc[1]) if kind == CE else None
    periods = np.linspace(2.0, 30.0, 64)
    shapes = [(9000, 64, "<256,4,ZS>x4"), (66_000, 33, "<256,4,ZS>x29")]
    arrays, cases = {"periods": periods}, []
    for n, P, _ in shapes:
        arrays[f"t{n}"] = t[:n]
        if mag is not None:
            arrays[f"x{n}"] = so.magnitude_bins(x[:n], nbc[1])
        cases.append(case(f"n{n}", kind, f"t{n}", "periods", P, nbc, f"x{n}"))
    res = run_child(tmp_path, "cells", {}, cases, arrays)
    cells = (nbc[0] + 1) * nbc[1] if kind == CE else nbc[0] + 1
    for c, (n, P, route) in zip(cases, shapes):
        check_route(res, c, route, z_len=2304, finish_lds=cells * 64 * 8)
        want = oracle(kind, t[:n], None if mag is None else arrays[f"x{n}"], periods[:P], nbc)
        check_values(kind, res[c["name"]], want, f"n={n} P={P} {nbc[0]}x{nbc[1]} ({cells} cells)", route)
        if nbc == (190, 1):
            assert np.all(res[c["name"]] == 0.0)


# ---- 6. split mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8191, 8192])
@pytest.mark.parametrize("kind", list(SMALL), ids=[NAME[k] for k in SMALL])
def test_split_threshold_few_groups_rule_and_score_rule(tmp_path, kind, n):
    """8191 samples: unsplit.  8192: 49 088 periods (767 groups) take the few-groups rule, 2 slices of 4096; 49 089 (768
    groups) the score, 4 slices of 2048 (Gregory-Loredo, 2048 resident workgroups: 2 of 4096).  Back to back in one
    process; the shorter grid is a prefix of the longer."""
    t, x = curve(8192, 8, t_shift=JD)
    t, x = t[:n], x[:n]
    periods = np.linspace(1.0, 60.0, 49_089)
    v, sigma = values_of(kind, x), sigma_of(kind, x)
    arrays = {"t": t, "periods": periods}
    if v is not None:
        arrays["x"] = v
    cases = [case(f"p{P}", kind, "t", "periods", P, SMALL[kind], "x", sigma) for P in (49_088, 49_089)]
    res = run_child(tmp_path, "threshold", {}, cases, arrays)
    want = oracle(kind, t, v, periods, SMALL[kind], sigma)
    if n == 8191:
        routes = [("<256,4>", 0), ("<256,4>", 0)]
    else:
        routes = [("<256,4,ZS>x2", 4096), ("<256,4,ZS>x2", 4096) if kind == GL else ("<256,4,ZS>x4", 2048)]
    for c, (route, z_len) in zip(cases, routes):
        check_route(res, c, route, z_len=z_len)
        check_values(kind, res[c["name"]], want[:c["P"]], f"n={n} P={c['P']}", route)


@pytest.mark.parametrize("kind", list(SMALL), ids=[NAME[k] for k in SMALL])
def test_seventeen_slices_and_a_last_slice_of_one_sample(tmp_path, kind):
    """34 816 samples x 64 periods: 17 slices of 2048, one more than pdm_finish_kernel has waves.  18 433 samples: 8
    slices are allowed and asked for, of ceil(2305 / 256) x 256 = 2304 samples, which makes 9 - the last with ONE
    sample."""
    t, x = curve(34_816, 9, t_shift=JD)
    periods = np.linspace(1.0, 60.0, 64)
    sigma = sigma_of(kind, x)
    shapes = [(34_816, "<256,4,ZS>x17", 2048), (18_433, "<256,4,ZS>x9", 2304)]
    arrays, cases = {"periods": periods}, []
    for n, _, _ in shapes:
        arrays[f"t{n}"] = t[:n]
        if kind != GL:
            arrays[f"x{n}"] = values_of(kind, x[:n])
        cases.append(case(f"n{n}", kind, f"t{n}", "periods", 64, SMALL[kind], f"x{n}", sigma))
    res = run_child(tmp_path, "slices", {}, cases, arrays)
    for c, (n, route, z_len) in zip(cases, shapes):
        rec = check_route(res, c, route, z_len=z_len, workgroups=1)
        assert n - (rec["n_z"] - 1) * rec["z_len"] == (2048 if n == 34_816 else 1)
        check_values(kind, res[c["name"]], oracle(kind, t[:n], arrays.get(f"x{n}"), periods, SMALL[kind], sigma),
                     f"n={n} P=64", route)


@pytest.mark.parametrize("kind", list(SMALL), ids=[NAME[k] for k in SMALL])
def test_the_switches_in_children_of_their_own(tmp_path, kind):
    """One input, three processes, one at a time: no switch (the few-groups rule: 2 slices; the score: 4, Gregory-Loredo
    2), PDC_PDM_SPLIT=0 (unsplit <256, 4>) and PDC_PDM_NZ=3, which replaces the score's answer only (3 slices of 2816
    at 49 089 periods, still 2 of 4096 at 49 088).  Split and unsplit results agree to 1e-12.  With PDC_PDM_SPLIT=0 the
    counts-only kinds still cut 66 000 samples in the two slices their 16-bit cells force."""
    t, x = curve(8192, 8, t_shift=JD)
    periods = np.linspace(1.0, 60.0, 49_089)
    v, sigma = values_of(kind, x), sigma_of(kind, x)
    arrays = {"t": t, "periods": periods}
    if v is not None:
        arrays["x"] = v
    cases = [case(f"p{P}", kind, "t", "periods", P, SMALL[kind], "x", sigma) for P in (49_088, 49_089)]
    long_t, long_x = curve(66_000, 7, period=9.1, t_shift=JD)
    forced = []
    if kind in (CE, GL):
        arrays["long_t"], arrays["long_periods"] = long_t, np.linspace(2.0, 30.0, 33)
        if kind == CE:
            arrays["long_x"] = values_of(kind, long_x)
        forced = [case("long", kind, "long_t", "long_periods", 33, SMALL[kind], "long_x")]
    default = run_child(tmp_path, "default", {}, cases, arrays)
    off = run_child(tmp_path, "off", {"PDC_PDM_SPLIT": 0}, cases + forced, arrays)
    nz3 = run_child(tmp_path, "nz3", {"PDC_PDM_NZ": 3}, cases, arrays)
    want = oracle(kind, t, v, periods, SMALL[kind], sigma)
    score = ("<256,4,ZS>x2", 4096) if kind == GL else ("<256,4,ZS>x4", 2048)
    for c, by_default, by_nz3 in zip(cases, (("<256,4,ZS>x2", 4096), score), (("<256,4,ZS>x2", 4096), ("<256,4,ZS>x3", 2816))):
        check_route(default, c, by_default[0], z_len=by_default[1])
        check_route(off, c, "<256,4>", split=0)
        check_route(nz3, c, by_nz3[0], z_len=by_nz3[1])
        k, P = c["name"], c["P"]
        check_values(kind, off[k], want[:P], f"n=8192 P={P} PDC_PDM_SPLIT=0", "<256,4>")
        check_values(kind, nz3[k], want[:P], f"n=8192 P={P} PDC_PDM_NZ=3", by_nz3[0])
        for other in (default[k], nz3[k]):
            np.testing.assert_allclose(other, off[k], rtol=1e-12, atol=0.0)
    for c in forced:
        check_route(off, c, "<256,4,ZS>x2", z_len=33_024)          # ceil(33 000 / 256) x 256
        check_values(kind, off["long"], oracle(kind, long_t, arrays.get("long_x"), arrays["long_periods"], SMALL[kind]),
                     "n=66000 P=33 PDC_PDM_SPLIT=0", "<256,4,ZS>x2")
