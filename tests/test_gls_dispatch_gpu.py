"""Every route of the GLS dispatcher (``scan_dev`` in csrc/gls.hip) at the smallest shape that reaches it.

The dispatcher chooses between the general scan, the general scan with the samples cut into parts (on ``grid.y`` or
dealt to the XCDs), the balanced-pieces launch and the two shared-time-axis kernels from a cost model, a handful of
thresholds and the ``PDC_GLS_*`` switches.  A switch does not guarantee its route (a weight table that does not fit
falls through to the general kernel, a forced balanced launch still needs enough tiles), so every case here first
asserts, through the ``pdc_test_gls_last_dispatch`` hook, which route, tile shape and part count actually ran, and only
then checks the numbers:

* Tier E against the long-double sums (1e-6 relative, floor 1e-13 of the maximum; the inputs are chosen so that NO bin
  of the exact spectrum is under the floor, which is asserted); where the pair count forbids it, against the
  double-precision direct sums on every bin, re-proved first against the long-double sums on a stratified subset;
* agreement with the same call on the plain route to rtol 1e-9 / atol 1e-14 max (only the summation order differs);
* the same bits on a repeated call;
* device-side peaks equal to nanmax / nanargmax of the returned power, with and without the spectrum written.

The switches are read once per process: every group of cases runs in a child interpreter, one at a time.  Inputs are
noisy sinusoids on a Julian-date-sized time axis.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-6            # Tier E (BASELINE.json north_star)
FLOOR = 1e-13
JD = 2454900.5

_CHILD = r"""
import json, sys
import numpy as np
from periodicity_amd import _cabi
spec = json.load(open(sys.argv[1]))
data = np.load(sys.argv[2])
out = {}
for c in spec:
    k = c["name"]
    t, y = data[k + "_t"], data[k + "_y"]
    dy = data[k + "_dy"] if k + "_dy" in data.files else None
    if "boot" in c:
        picks = data[k + "_picks"]
        amax, arg = _cabi.gls_bootstrap(t, y, dy, picks, c["f0"], c["delta"], c["nf"], c["fit_mean"], c["psd"])
        out[k + "_rec"] = json.dumps(_cabi.gls_last_dispatch())
        out[k + "_amax"], out[k + "_arg"] = amax, arg
        B, n = picks.shape
        y, dy = y[picks].ravel(), (None if dy is None else dy[picks].ravel())
        c = dict(c, B=B, n=n, shared_t=True, j_begin=0)
    B, n = c["B"], c["n"]
    offsets = np.arange(B + 1, dtype=np.int64) * n
    args = (t, y, dy, offsets, c["f0"], c["delta"], c["nf"], c["fit_mean"], c["psd"], c["shared_t"])
    power, amax, arg = _cabi.gls_scan_batch(*args, want_power=True, want_peaks=True, j_begin=c["j_begin"])
    out[k + "_rec_scan"] = json.dumps(_cabi.gls_last_dispatch())
    again, _, _ = _cabi.gls_scan_batch(*args, want_power=True, want_peaks=False, j_begin=c["j_begin"])
    _, amax2, arg2 = _cabi.gls_scan_batch(*args, want_power=False, want_peaks=True, j_begin=c["j_begin"])
    out[k + "_rec_peaks"] = json.dumps(_cabi.gls_last_dispatch())
    out[k + "_power"] = power
    out[k + "_same_bits"] = np.array_equal(power, again, equal_nan=True)
    out[k + "_peaks"] = np.stack([amax, amax2])
    out[k + "_args"] = np.stack([arg, arg2])
    if c.get("twin"):   # the plain route: a two-curve batch is never cut into parts or balanced pieces
        two, _, _ = _cabi.gls_scan_batch(np.tile(t, 2), np.tile(y, 2), None if dy is None else np.tile(dy, 2),
                                         np.array([0, n, 2 * n]), c["f0"], c["delta"], c["nf"], c["fit_mean"],
                                         c["psd"], j_begin=c["j_begin"])
        out[k + "_twin"] = two[0]
        out[k + "_rec_twin"] = json.dumps(_cabi.gls_last_dispatch())
np.savez(sys.argv[3], **out)
print("ok")
"""


def run_child(tmp_path, tag, env, cases, arrays):
    """One fresh interpreter with the ``PDC_GLS_*`` switches of ``env`` (and no others): every case's scan, its
    repeat, its peaks-only call and the hook's records come back in an npz."""
    spec, inp, res = (str(tmp_path / f"{tag}.{ext}") for ext in ("json", "in.npz", "out.npz"))
    with open(spec, "w") as fh:
        json.dump(cases, fh)
    np.savez(inp, **arrays)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PDC_GLS_")}
    clean.update({k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, "-c", _CHILD, spec, inp, res], env=clean, cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stderr[-2000:])
    return np.load(res)


def record(res, key):
    return json.loads(str(res[key]))


def check_record(rec, **want):
    got = {k: rec[k] for k in want}
    assert got == want, (got, want, rec)


def tier_e(power, exact, label):
    """``assert_tier_e`` of tests/test_gls_gpu.py with the stronger input condition of this file: no bin of the exact
    spectrum may be under the floor."""
    exact = np.asarray(exact)
    assert power.shape == exact.shape
    ok = np.abs(exact) > FLOOR * np.nanmax(np.abs(exact))
    assert ok.all(), (label, int((~ok).sum()))
    rel = np.abs(power - exact) / np.abs(exact)
    print(f"DISPATCH-REL {label} max rel err {np.nanmax(rel):.3e}")
    assert np.all(np.isfinite(power)) and rel.max() <= RTOL, (label, rel.max(), int(np.argmax(rel)))
    return rel.max()


def check_common(res, k, label):
    """Same bits on a repeat; device peaks == nanmax / nanargmax of the returned power, with and without the spectrum."""
    power = res[k + "_power"]
    assert bool(res[k + "_same_bits"]), label
    amax, arg = res[k + "_peaks"], res[k + "_args"]
    for b in range(power.shape[0]):
        j = int(np.nanargmax(power[b]))
        assert arg[0][b] == j and amax[0][b] == power[b][j], (label, b)
    assert np.array_equal(amax[0], amax[1]) and np.array_equal(arg[0], arg[1]), label
    assert record(res, k + "_rec_scan") == record(res, k + "_rec_peaks"), label


def check_plain(power, plain, label):
    np.testing.assert_allclose(power, plain, rtol=1e-9, atol=1e-14 * np.nanmax(plain), err_msg=label)


def sinusoid(n, seed, period, span=None):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, float(span or n), n)) + JD
    dy = rng.uniform(0.05, 0.2, n)
    y = 1.0 + 0.5 * np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)
    return t, y, dy


def grid(f0, delta, nf, j_begin=0):
    return f0 + delta * np.arange(j_begin, j_begin + nf)       # the device's fill rule: one product, one sum


# ---- balanced pieces -------------------------------------------------------------------------------------------------
# gls_scan_kernel<16, MODE, S, true> + the piece branch of gls_finish_kernel: K = 16, S >= 2, fewer than 16384 samples
# (no sample parts), more than half of the next multiple of 512 tiles and >= 32 chunks of 128 samples.
#   name: (S, n, nf, fit_mean, psd, j_begin) -> tiles / slots
BALANCED = {
    "s4_257": (4, 3969, 257 * 1024 - 5, True, False, 0),      # every tile cut in 2-3, last tile partial, last chunk 1 sample
    "s4_512": (4, 4100, 512 * 1024, False, True, 0),          # remainder 0: only when forced
    "s4_514": (4, 4173, 513 * 1024 + 1, True, True, 0),       # 514 tiles in 1024 slots
    "s2_301": (2, 5000, 300 * 2048 + 1000, False, False, 0),
    "s2_301_slab": (2, 5000, 300 * 2048 + 1000, True, False, 123_457),
    "model_385": (4, 4001, 385 * 1024 - 3, True, False, 0),   # no switch set: the cost model's own choice
}


def balanced_inputs(name):
    S, n, nf, fit_mean, psd, j_begin = BALANCED[name]
    t, y, dy = sinusoid(n, 7000 + n, period=37.3)
    delta = 1.0 / (t[-1] - t[0]) / 5
    f0 = 0.5 * delta
    case = dict(name=name, B=1, n=n, f0=f0, delta=delta, nf=nf, fit_mean=fit_mean, psd=psd, shared_t=False,
                j_begin=j_begin)
    return case, {name + "_t": t, name + "_y": y, name + "_dy": dy}


def cut_tiles(tiles, chunks, slots):
    """Tiles whose chunk range [tile * chunks, (tile + 1) * chunks) holds a run boundary s U / W strictly inside."""
    units = tiles * chunks
    edges = np.arange(1, slots, dtype=np.int64) * units // slots
    return np.unique(edges[edges % chunks != 0] // chunks)


_exact_cache = {}


def balanced_exact(name):
    """Every bin by the double-precision direct sums, re-proved on >= 512 stratified bins against the long-double
    sums: first and last frequency of every tile, the tiles a piece boundary cuts (their middle and a random bin as
    well), random interior bins.  The re-proof bound is 1e-8, two orders under the 1e-6 gate, so that the checker's own
    rounding can never decide a verdict: its sums carry an absolute error of ~ 1e-16 sqrt(n), which at a bin of
    relative power p is a relative error ~ 1 / sqrt(p) (1e-12 at the peak, 1e-9 at p = 1e-5 with these 4000-sample
    curves; the full-size C2 test meets 1e-10 because its 25 times longer curve averages the noise floor down)."""
    if name in _exact_cache:
        return _exact_cache[name]
    S, n, nf, fit_mean, psd, j_begin = BALANCED[name]
    case, arr = balanced_inputs(name)
    t, y, dy = arr[name + "_t"], arr[name + "_y"], arr[name + "_dy"]
    freq = grid(case["f0"], case["delta"], nf, j_begin)
    tile = (256 // S) * 16
    tiles = (nf + tile - 1) // tile
    chunks, slots = (n + 127) // 128, (tiles + 511) // 512 * 512
    rng = np.random.default_rng(1)
    starts = np.arange(0, nf, tile)
    ends = np.minimum(starts + tile, nf) - 1
    cut = cut_tiles(tiles, chunks, slots)
    assert cut.size == (0 if tiles == slots else tiles)   # (every tile is cut, but for one tile per slot)
    span = ends[cut] - starts[cut] + 1
    pick = np.unique(np.concatenate([starts, ends, starts[cut] + span // 2, starts[cut] + rng.integers(0, span),
                                     rng.integers(0, nf, 200), [0, nf - 1]]))
    assert pick.size >= 512
    exact = np.asarray(co.gls_power_exact(t, y, dy, freq[pick], fit_mean, psd))
    fast = np.asarray(co.gls_power_f64(t, y, dy, freq[pick], fit_mean, psd))
    assert np.max(np.abs(fast - exact) / np.abs(exact)) <= 1e-8
    full = np.asarray(co.gls_power_f64(t, y, dy, freq, fit_mean, psd))
    _exact_cache[name] = (full, pick, exact, tiles, slots, chunks)
    return _exact_cache[name]


def check_balanced(res, plain, name):
    S = BALANCED[name][0]
    full, pick, exact, tiles, slots, chunks = balanced_exact(name)
    check_record(record(res, name + "_rec_scan"), route="balanced", K=16, S=S, tiles=tiles, parts=1, parts_by_xcd=0,
                 bal_slots=slots, bal_chunks=chunks, wide_prep=0)
    power = res[name + "_power"][0]
    tier_e(power[pick], exact, f"balanced {name} (long double, {pick.size} bins)")
    tier_e(power, full, f"balanced {name} (every bin)")
    assert int(np.argmax(full)) == int(res[name + "_args"][0][0])
    check_common(res, name, name)
    if plain is not None:
        check_record(record(plain, name + "_rec_scan"), route="general", K=16, S=S, tiles=tiles, parts=1, bal_slots=0)
        check_plain(power, plain[name + "_power"][0], name)


@pytest.mark.parametrize("S", [4, 2])
def test_balanced_pieces_forced(tmp_path, S):
    """PDC_GLS_K=16, PDC_GLS_BAL=1 and PDC_GLS_S: both S, all four (fit_mean, psd) pairs over the cases, a slab with
    j_begin != 0; the plain route is the same tile shape with PDC_GLS_BAL=0."""
    names = [k for k, v in BALANCED.items() if v[0] == S and not k.startswith("model")]
    cases, arrays = [], {}
    for k in names:
        c, a = balanced_inputs(k)
        cases.append(c)
        arrays.update(a)
    res = run_child(tmp_path, "bal", dict(PDC_GLS_K=16, PDC_GLS_S=S, PDC_GLS_BAL=1), cases, arrays)
    plain = run_child(tmp_path, "plain", dict(PDC_GLS_K=16, PDC_GLS_S=S, PDC_GLS_BAL=0), cases, arrays)
    for k in names:
        check_balanced(res, plain, k)


def test_balanced_pieces_by_the_cost_model(tmp_path):
    """No switch set: at 385 tiles of 1024 frequencies the model itself picks K = 16, S = 4 and the balanced launch."""
    c, a = balanced_inputs("model_385")
    check_balanced(run_child(tmp_path, "model", {}, [c], a), None, "model_385")


def test_a_forced_balanced_launch_still_needs_enough_tiles(tmp_path):
    """PDC_GLS_BAL=1 with 256 tiles (not more than half of 512 slots) or with 31 chunks stays on the general route:
    the hook says so and the numbers are right."""
    cases, arrays = [], {}
    for name, n, nf in (("few_tiles", 3969, 256 * 1024), ("few_chunks", 3968, 257 * 1024)):
        t, y, dy = sinusoid(n, 11, period=37.3)
        delta = 1.0 / (t[-1] - t[0]) / 5
        cases.append(dict(name=name, B=1, n=n, f0=0.5 * delta, delta=delta, nf=nf, fit_mean=True, psd=False,
                          shared_t=False, j_begin=0))
        arrays.update({name + "_t": t, name + "_y": y, name + "_dy": dy})
    res = run_child(tmp_path, "nobal", dict(PDC_GLS_K=16, PDC_GLS_S=4, PDC_GLS_BAL=1), cases, arrays)
    rng = np.random.default_rng(2)
    for c in cases:
        k = c["name"]
        check_record(record(res, k + "_rec_scan"), route="general", K=16, S=4, bal_slots=0, parts=1)
        pick = np.unique(np.concatenate([np.arange(0, c["nf"], 1024), rng.integers(0, c["nf"], 300), [c["nf"] - 1]]))
        exact = co.gls_power_exact(arrays[k + "_t"], arrays[k + "_y"], arrays[k + "_dy"],
                                   grid(c["f0"], c["delta"], c["nf"])[pick])
        tier_e(res[k + "_power"][0][pick], exact, f"general {k}")
        check_common(res, k, k)


# ---- sample parts ----------------------------------------------------------------------------------------------------
# GlsArgs::partial: one curve of >= 16384 samples on a short grid; fewer than 8 parts ride on grid.y, 8 or more are
# dealt to the XCDs (part z on XCD z % 8; with a count that is no multiple of 8 the spare workgroups return early).
# z_len = the part length rounded up to 128 samples, which may leave fewer parts than asked for.
#   name: (Z asked, n, nf, K, S, fit_mean, psd, final parts, z_len, samples in the last part)
PARTS = {
    "z2": (2, 16400, 37, 8, 1, True, True, 2, 8320, 8080),
    "z7": (7, 16400, 700, 16, 2, False, True, 7, 2432, 1808),
    "z8": (8, 16385, 1500, 4, 4, True, False, 8, 2176, 1153),
    "z9": (9, 18500, 700, 8, 2, False, False, 9, 2176, 1092),            # 16 XCD slots, 7 early returns
    "z17_one_sample": (17, 34817, 37, 16, 4, True, False, 17, 2176, 1),    # the last part holds one sample
    "z18_shrinks": (18, 36865, 700, 4, 2, False, True, 17, 2176, 2049),    # rounding z_len up leaves 17 of 18 parts
    "z512": (512, 1 << 20, 100, 8, 4, True, False, 512, 2048, 2048),       # kPartsMax
}


def parts_inputs(name, n, nf, fit_mean, psd, seed=31):
    t, y, dy = sinusoid(n, seed, period=12.3)
    delta = 2e-7                                           # a zoom on the peak
    f0 = 1 / 12.3 - (nf // 2) * delta
    case = dict(name=name, B=1, n=n, f0=f0, delta=delta, nf=nf, fit_mean=fit_mean, psd=psd, shared_t=False, j_begin=0,
                twin=True)
    return case, {name + "_t": t, name + "_y": y, name + "_dy": dy}


def parts_exact(key, case, arrays):
    if key not in _exact_cache:
        k = case["name"]
        _exact_cache[key] = np.asarray(co.gls_power_exact(arrays[k + "_t"], arrays[k + "_y"], arrays[k + "_dy"],
                                                          grid(case["f0"], case["delta"], case["nf"]),
                                                          case["fit_mean"], case["psd"]))
    return _exact_cache[key]


def check_parts(res, case, arrays, key, label, **want):
    k = case["name"]
    check_record(record(res, k + "_rec_scan"), wide_prep=1, **want)
    power = res[k + "_power"][0]
    tier_e(power, parts_exact(key, case, arrays), label)
    check_common(res, k, label)
    check_record(record(res, k + "_rec_twin"), route="general", parts=1, K=want["K"], S=want["S"], wide_prep=0)
    check_plain(power, res[k + "_twin"], label)


@pytest.mark.parametrize("name", list(PARTS))
def test_sample_parts_forced(tmp_path, name):
    Z, n, nf, K, S, fit_mean, psd, parts, z_len, last = PARTS[name]
    assert (n + z_len - 1) // z_len == parts and n - (parts - 1) * z_len == last      # (what the table claims)
    case, arrays = parts_inputs(name, n, nf, fit_mean, psd)
    res = run_child(tmp_path, name, dict(PDC_GLS_Z=Z, PDC_GLS_K=K, PDC_GLS_S=S), [case], arrays)
    tile = (256 // S) * K
    check_parts(res, case, arrays, name, f"parts {name}", route="parts", K=K, S=S, parts=parts,
                parts_by_xcd=int(parts >= 8), z_len=z_len, tiles=(nf + tile - 1) // tile, bal_slots=0)


@pytest.mark.parametrize("Z", [1, 3, 8])
@pytest.mark.parametrize("K,S", [(K, S) for K in (4, 8, 16) for S in (1, 2, 4)])
def test_every_tile_shape_behind_the_wide_prologue_and_with_parts(tmp_path, K, S, Z):
    """All nine (K, S) instantiations at n = 16385 (gls_prep_wide_*), uncut, on grid.y and dealt to the XCDs."""
    n = 16385
    cases, arrays = [], {}
    for name, nf, fit_mean, psd in (("nf1500", 1500, True, False), ("nf37", 37, False, True)):
        c, a = parts_inputs(name, n, nf, fit_mean, psd, seed=32)
        cases.append(c)
        arrays.update(a)
    res = run_child(tmp_path, "ks", dict(PDC_GLS_Z=Z, PDC_GLS_K=K, PDC_GLS_S=S, PDC_GLS_BAL=0), cases, arrays)
    z_len = {1: 0, 3: 5504, 8: 2176}[Z]
    tile = (256 // S) * K
    for c in cases:
        check_parts(res, c, arrays, "ks_" + c["name"], f"K{K} S{S} Z{Z} {c['name']}",
                    route="parts" if Z > 1 else "general", K=K, S=S, parts=Z, parts_by_xcd=int(Z >= 8), z_len=z_len,
                    tiles=(c["nf"] + tile - 1) // tile, bal_slots=0)


# ---- shared time axis ------------------------------------------------------------------------------------------------
# gls_shared2_kernel (individual weights, two frequencies per lane, 64 curves per workgroup), gls_shared_kernel<*, false>
# (individual weights, PDC_GLS_SH2=0, 128 curves per workgroup) and gls_shared_kernel<*, true> (equal weights, 256
# curves per workgroup): curve counts on both sides of a group boundary, sample counts around the 32-sample chunk and
# its two read-ahead rows, grids shorter than and straddling a 64- / 128-frequency tile.
#   (B, n, nf, fit_mean, psd); two samples cannot carry a fitted mean, hence fit_mean = False there
SHARED = [(2, 257, 700, True, False),          # the [sample][curve] table does not fit: falls back to the general kernel
          (96, 2, 1, False, True),
          (128, 31, 63, True, True),
          (129, 32, 64, False, False),
          (257, 33, 65, True, False),
          (96, 257, 127, False, True),
          (128, 33, 128, True, True),
          (129, 31, 129, False, False),
          (257, 32, 700, True, False)]
KERNELS = {"two_per_lane": (True, {}), "one_per_lane": (True, {"PDC_GLS_SH2": 0}), "equal_weights": (False, {})}


def shared_inputs(with_dy):
    cases, arrays = [], {}
    for i, (B, n, nf, fit_mean, psd) in enumerate(SHARED):
        rng = np.random.default_rng(500 + i)
        name = f"b{B}_n{n}_nf{nf}"
        t = np.sort(rng.uniform(0, 40.0, n)) + JD
        y = 1.0 + np.sin(2 * np.pi * t / 3.3)[None, :] + 0.5 * rng.standard_normal((B, n))
        arrays.update({name + "_t": t, name + "_y": y.ravel()})
        if with_dy:
            arrays[name + "_dy"] = rng.uniform(0.1, 0.5, (B, n)).ravel()
        cases.append(dict(name=name, B=B, n=n, f0=0.0113, delta=0.0021 if nf > 1 else 0.0, nf=nf, fit_mean=fit_mean,
                          psd=psd, shared_t=True, j_begin=0))
    # GLS.bootstrap's call: replicates by index
    t, y, dy = sinusoid(257, 77, period=3.3, span=40.0)
    rng = np.random.default_rng(9)
    arrays.update({"boot_t": t, "boot_y": y, "boot_picks": rng.integers(0, 257, (130, 257)).astype(np.int32)})
    if with_dy:
        arrays["boot_dy"] = dy
    cases.append(dict(name="boot", boot=True, f0=0.0113, delta=0.0021, nf=700, fit_mean=True, psd=False))
    return cases, arrays


def shared_exact(with_dy, case, arrays):
    key = ("shared", with_dy, case["name"])
    if key not in _exact_cache:
        k = case["name"]
        t, freq = arrays[k + "_t"], grid(case["f0"], case["delta"], case["nf"])
        fit_mean, psd = case["fit_mean"], case["psd"]
        if "boot" in case:
            picks = arrays[k + "_picks"]
            y = arrays[k + "_y"][picks]
            dy = arrays[k + "_dy"][picks] if with_dy else None
        else:
            y = arrays[k + "_y"].reshape(case["B"], case["n"])
            dy = arrays[k + "_dy"].reshape(case["B"], case["n"]) if with_dy else None
        _exact_cache[key] = np.stack([np.asarray(co.gls_power_exact(t, y[b], None if dy is None else dy[b], freq,
                                                                    fit_mean, psd)) for b in range(y.shape[0])])
    return _exact_cache[key]


_plain_cache = {}


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_shared_time_axis_kernels(tmp_path, kernel):
    with_dy, extra = KERNELS[kernel]
    cases, arrays = shared_inputs(with_dy)
    res = run_child(tmp_path, kernel, dict(PDC_GLS_SHARED=1, **extra), cases, arrays)
    if with_dy not in _plain_cache:     # the plain route: one curve per tile column, PDC_GLS_SHARED=0
        _plain_cache[with_dy] = dict(run_child(tmp_path, "plain", dict(PDC_GLS_SHARED=0), cases, arrays))
    plain = _plain_cache[with_dy]
    per_group = {"two_per_lane": 64, "one_per_lane": 128, "equal_weights": 256}[kernel]
    pad = 256 if kernel == "equal_weights" else 128
    per_lane = 2 if kernel == "two_per_lane" else 1
    for c in cases:
        k = c["name"]
        B = arrays[k + "_picks"].shape[0] if "boot" in c else c["B"]
        bpad = (B + pad - 1) // pad * pad
        want = dict(route="shared2" if per_lane == 2 else "shared", K=per_lane, S=0, bpad=bpad, groups=bpad // per_group,
                    tiles=(c["nf"] + 64 * per_lane - 1) // (64 * per_lane), parts=1, wide_prep=0)
        if B == 2:
            want = dict(route="general", bpad=0, groups=0, parts=1)     # no room for the table: the general kernel
        check_record(record(res, k + "_rec_scan"), **want)
        check_record(record(plain, k + "_rec_scan"), route="general", bpad=0)
        exact = shared_exact(with_dy, c, arrays)
        power = res[k + "_power"]
        label = f"shared {kernel} {k}" if B > 2 else f"shared-forced fallback {kernel} {k}"
        tier_e(power, exact, label)
        check_common(res, k, label)
        for b in range(B):
            check_plain(power[b], plain[k + "_power"][b], f"{label} row {b}")
        if "boot" in c:
            # the replicates by index: the same route, the same bits as the expanded batch, the oracle's peak
            check_record(record(res, k + "_rec"), **want)
            assert np.array_equal(res[k + "_amax"], res[k + "_peaks"][0]), label
            assert np.array_equal(res[k + "_arg"], res[k + "_args"][0]), label
            assert np.array_equal(res[k + "_arg"], np.argmax(exact, axis=1)), label
            assert np.max(np.abs(res[k + "_amax"] / exact.max(axis=1) - 1)) <= RTOL, label
