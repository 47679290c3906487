"""The mirrored-pair kernel of the GLS scan (``gls_scan_kernel<16, MODE, S, BAL, PAIR = true>`` in csrc/gls.hip).

A thread owns its sixteen frequencies as a centre and eight mirrored offsets; the sines and cosines of the offset angles
come from a per-sample table as scalar operands, twelve running sums per offset are recombined into the six sums of its
two frequencies after the sample loop, and two sample-only remainders per offset (G_m, F_m) are added per chunk by the
table fill.  Every case runs in a child interpreter with ``PDC_GLS_K=16`` and ``PDC_GLS_PAIR=1`` and again with
``PDC_GLS_PAIR=0`` (the switches are read once per process) and asserts

* through ``pdc_test_gls_last_pair`` that the pair kernel ran (and did not in the plain run), with a table of
  256 bytes per sample plus the two rows read ahead;
* Tier E against the long-double sums: 1e-6 relative on every bin, with inputs whose exact spectrum has no bin under
  1e-13 of its maximum (asserted); the two large cases check every bin against the double-precision direct sums,
  re-proved against the long-double sums on a stratified subset to 1e-8;
* rtol 1e-9 / atol 1e-14 max against the plain kernel;
* the same bits on a repeated call.

The identities themselves are checked without a GPU in ``test_twelve_sums_recombine_into_the_six``.

Three samples determine a mean, a sine and a cosine exactly (the fitted-mean periodogram is 1 with a vanishing
denominator), so the N = 3 cases run without the fitted mean; N = 129 runs all four (fit_mean, psd) pairs.

Every grid starts at f0 T = 0.1 and steps by 1 / (5 T) (T the time span), as the grids of
tests/test_gls_dispatch_gpu.py do: for f T << 1 the sine, the cosine and the constant are nearly collinear over the
samples, the periodogram's 2 x 2 solve loses ~ (f T)^-4 in conditioning, and two correct fp64 kernels agree with the
long-double sums and with each other only that much worse (at f T = 0.016 the plain and the pair kernel sit 7e-10 and
6e-9 from the exact value: the bound against the exact sums holds, a 1e-9 comparison between the kernels cannot).
The far slab keeps the same step: its first frequency is at f T = 24 691.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-6            # Tier E (BASELINE.json north_star)
FLOOR = 1e-13
JD = 2.45e6            # days: the exact phase product of the offset table has ~1e5 whole cycles to drop
FOUR = [(True, False), (False, True), (True, True), (False, False)]     # (fit_mean, psd)

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
    args = (t, y, dy, np.asarray(c["offsets"], dtype=np.int64), c["f0"], c["delta"], c["nf"], c["fit_mean"], c["psd"])
    power, _, _ = _cabi.gls_scan_batch(*args, j_begin=c["j_begin"])
    out[k + "_pair"] = np.array(_cabi.gls_last_pair(), dtype=np.int64)
    out[k + "_rec"] = json.dumps(_cabi.gls_last_dispatch())
    again, _, _ = _cabi.gls_scan_batch(*args, j_begin=c["j_begin"])
    out[k + "_power"] = power
    out[k + "_same_bits"] = np.array_equal(power, again, equal_nan=True)
np.savez(sys.argv[3], **out)
print("ok")
"""


def run_child(tmp_path, tag, env, cases, arrays):
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


def both(tmp_path, env, cases, arrays):
    """The pair run and the plain run of the same cases under the same switches."""
    return (run_child(tmp_path, "pair", dict(env, PDC_GLS_K=16, PDC_GLS_PAIR=1), cases, arrays),
            run_child(tmp_path, "plain", dict(env, PDC_GLS_K=16, PDC_GLS_PAIR=0), cases, arrays))


def curve(n, seed, period=37.3, span=None, with_dy=True):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, float(span or max(n, 40)), n)) + JD
    dy = rng.uniform(0.05, 0.2, n)
    y = 1.0 + 0.5 * np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)
    return t, y, (dy if with_dy else None)


def grid(c):
    return c["f0"] + c["delta"] * np.arange(c["j_begin"], c["j_begin"] + c["nf"])   # the device's fill rule


def make_case(name, t, y, dy, nf, fit_mean, psd, j_begin=0, over=5.0, f0_bins=0.5, offsets=None):
    delta = 1.0 / (t[-1] - t[0]) / over
    case = dict(name=name, offsets=[0, int(t.size)] if offsets is None else [int(o) for o in offsets], f0=f0_bins * delta,
                delta=delta, nf=int(nf), fit_mean=bool(fit_mean), psd=bool(psd), j_begin=int(j_begin))
    arrays = {name + "_t": t, name + "_y": y}
    if dy is not None:
        arrays[name + "_dy"] = dy
    return case, arrays


def tier_e(power, exact, label):
    exact = np.asarray(exact)
    assert power.shape == exact.shape
    ok = np.abs(exact) > FLOOR * np.nanmax(np.abs(exact))
    assert ok.all(), (label, int((~ok).sum()))          # the input condition: no bin under the floor
    rel = np.abs(power - exact) / np.abs(exact)
    print(f"PAIR-REL {label} max rel err {np.nanmax(rel):.3e}")
    assert np.all(np.isfinite(power)) and rel.max() <= RTOL, (label, rel.max(), int(np.argmax(rel)))


def check_ran(pair, plain, c, **want):
    k = c["name"]
    n_total = c["offsets"][-1]
    assert list(pair[k + "_pair"]) == [1, (n_total + 2) * 256], (k, pair[k + "_pair"])
    assert list(plain[k + "_pair"]) == [0, 0], (k, plain[k + "_pair"])
    for res in (pair, plain):
        rec = json.loads(str(res[k + "_rec"]))
        got = {key: rec[key] for key in dict(want, K=16)}
        assert got == dict(want, K=16), (k, rec)
        assert bool(res[k + "_same_bits"]), k


def check_plain(pair, plain, c):
    k = c["name"]
    a, b = pair[k + "_power"], plain[k + "_power"]
    diff = np.nanmax(np.abs(a - b) / (1e-9 * np.abs(b) + 1e-14 * np.nanmax(b)))
    print(f"PAIR-PLAIN {k} worst |pair - plain| / tolerance {diff:.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-14 * np.nanmax(b), err_msg=k)


def check_exact_every_bin(pair, plain, c, arrays, **want):
    k = c["name"]
    check_ran(pair, plain, c, **want)
    power = pair[k + "_power"]
    off = c["offsets"]
    for b in range(len(off) - 1):
        sl = slice(off[b], off[b + 1])
        dy = arrays[k + "_dy"][sl] if k + "_dy" in arrays else None
        exact = co.gls_power_exact(arrays[k + "_t"][sl], arrays[k + "_y"][sl], dy, grid(c), c["fit_mean"], c["psd"])
        tier_e(power[b], exact, f"{k} curve {b}")
    check_plain(pair, plain, c)


# ---- the identities, without a GPU -----------------------------------------------------------------------------------
def test_twelve_sums_recombine_into_the_six():
    """u+- = a c +- b s, v+- = b c -+ a s at the two frequencies centre +- (m + 1/2) delta: the twelve sums of products
    with the offset table and the remainders G = sum w s^2, F = sum w s2 give the direct six sums to <= 1e-12."""
    rng = np.random.default_rng(5)
    n = 4000
    t = np.sort(rng.uniform(0, 300.0, n))
    w = rng.uniform(0.2, 3.0, n)
    w /= w.sum()
    yv = rng.standard_normal(n)
    rw, delta, centre = np.sqrt(w), 1.0 / 1500.0, 0.3171
    a, b = rw * np.sin(2 * np.pi * centre * t), rw * np.cos(2 * np.pi * centre * t)
    A1, B1, A2, B2, a2, ab = rw * yv * a, rw * yv * b, rw * a, rw * b, a * a, a * b
    worst = 0.0
    for m in range(8):
        psi = 2 * np.pi * (m + 0.5) * delta * t
        c, s, c2, s2 = np.cos(psi), np.sin(psi), np.cos(2 * psi), np.sin(2 * psi)
        G, F = np.sum(w * s * s), np.sum(w * s2)
        P1, Q1, P2, Q2 = np.sum(A1 * c), np.sum(B1 * s), np.sum(B1 * c), np.sum(A1 * s)
        P3, Q3, P4, Q4 = np.sum(A2 * c), np.sum(B2 * s), np.sum(B2 * c), np.sum(A2 * s)
        R1, R2, R3, R4 = np.sum(a2 * c2), np.sum(ab * s2), np.sum(ab * c2), np.sum(a2 * s2)
        for sign in (+1, -1):
            got = np.array([P1 + sign * Q1, P2 - sign * Q2, P3 + sign * Q3, P4 - sign * Q4,
                            (R1 + G) + sign * R2, R3 + sign * (0.5 * F - R4)])
            f = centre + sign * (m + 0.5) * delta
            sn, cs = np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)
            direct = np.array([np.sum(w * yv * sn), np.sum(w * yv * cs), np.sum(w * sn), np.sum(w * cs),
                               np.sum(w * sn * sn), np.sum(w * sn * cs)])
            # relative to the size of the sums' terms (sum w = 1, |y| ~ 1): a sum may itself be near zero
            worst = max(worst, np.max(np.abs(got - direct)))
    assert worst <= 1e-12, worst


# ---- one thread's worth and less -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_thread_and_less(tmp_path):
    """nf = 1, 7, 16, 17 with N = 3 and N = 129: the centre may lie past nf, partners are masked, the chunk has a tail
    of one sample."""
    cases, arrays = [], {}
    for i, nf in enumerate((1, 7, 16, 17)):
        for n in (3, 129):
            fit_mean, psd = FOUR[i] if n > 3 else (False, bool(i & 1))
            t, y, dy = curve(n, 100 + i)
            c, a = make_case(f"nf{nf}_n{n}", t, y, dy, nf, fit_mean, psd, over=5.0)
            cases.append(c)
            arrays.update(a)
    pair, plain = both(tmp_path, {}, cases, arrays)
    for c in cases:
        check_exact_every_bin(pair, plain, c, arrays, route="general", tiles=1)


# ---- tile edges --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 4])
def test_tile_edges(tmp_path, S):
    """nf = one tile - 5 and one tile + 1 (tile = 256 / S x 16), N = 128 and 257; every bin is checked, so the first and
    last frequency of every tile and the pairs across every thread boundary 16 q +- 1 are."""
    tile = 256 // S * 16
    cases, arrays = [], {}
    for i, (nf, n) in enumerate(((tile - 5, 128), (tile - 5, 257), (tile + 1, 128), (tile + 1, 257))):
        fit_mean, psd = FOUR[(i + S) % 4]
        t, y, dy = curve(n, 200 + 10 * S + i)
        c, a = make_case(f"s{S}_nf{nf}_n{n}", t, y, dy, nf, fit_mean, psd)
        cases.append(c)
        arrays.update(a)
    pair, plain = both(tmp_path, dict(PDC_GLS_S=S), cases, arrays)
    for c in cases:
        check_exact_every_bin(pair, plain, c, arrays, route="general", S=S, tiles=(c["nf"] + tile - 1) // tile)


# ---- slabs, equal weights, a ragged batch ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_slabs_equal_weights_and_a_ragged_batch(tmp_path):
    """j_begin = 123 457; a grid stitched from slabs against the same grid in one call (rtol 1e-9, as
    test_slabs_tile_the_grid_bitwise); dy = None; two curves of different lengths in one batch (the offset table is
    indexed by the global sample)."""
    cases, arrays = [], {}
    t, y, dy = curve(257, 31)
    c, a = make_case("slab_far", t, y, dy, 2 * 2048 + 3, True, False, j_begin=123_457)
    cases.append(c)
    arrays.update(a)
    t, y, dy = curve(300, 32)
    nf = 8200
    cuts = [0, 1, 2047, 2048, 5000, nf]
    c, a = make_case("whole", t, y, dy, nf, True, True)
    cases.append(c)
    arrays.update(a)
    for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        cs, a = make_case(f"slab{i}", t, y, dy, hi - lo, True, True, j_begin=lo)
        cases.append(cs)
        arrays.update(a)
    t, y, _ = curve(129, 33, with_dy=False)
    c, a = make_case("equal_weights", t, y, None, 2048 + 17, False, False)
    cases.append(c)
    arrays.update(a)
    (t1, y1, d1), (t2, y2, d2) = curve(129, 34), curve(300, 35, span=129)
    c, a = make_case("ragged", np.concatenate([t1, t2]), np.concatenate([y1, y2]), np.concatenate([d1, d2]), 2048 + 17,
                     True, False, offsets=[0, 129, 429])
    c["delta"] = 1.0 / 129.0 / 5.0
    c["f0"] = 0.5 * c["delta"]
    cases.append(c)
    arrays.update(a)
    pair, plain = both(tmp_path, dict(PDC_GLS_S=2), cases, arrays)
    for c in cases:
        check_exact_every_bin(pair, plain, c, arrays, route="general", S=2)
    stitched = np.concatenate([pair[f"slab{i}_power"][0] for i in range(len(cuts) - 1)])
    whole = pair["whole_power"][0]
    np.testing.assert_allclose(stitched, whole, rtol=1e-9, atol=1e-14 * whole.max())


# ---- pieces and parts: the per-chunk remainders ------------------------------------------------------------------------
def big_exact(c, arrays, starts_every, extra):
    """Every bin by the double-precision direct sums, re-proved on a stratified subset (the first and last frequency of
    every tile, `extra`, random bins) against the long-double sums to 1e-8 (see balanced_exact in
    tests/test_gls_dispatch_gpu.py for why that bound)."""
    k = c["name"]
    t, y, dy = arrays[k + "_t"], arrays[k + "_y"], arrays[k + "_dy"]
    freq, nf = grid(c), c["nf"]
    rng = np.random.default_rng(1)
    starts = np.arange(0, nf, starts_every)
    pick = np.unique(np.concatenate([starts, np.minimum(starts + starts_every, nf) - 1, extra, rng.integers(0, nf, 200),
                                     [0, nf - 1]]))
    exact = np.asarray(co.gls_power_exact(t, y, dy, freq[pick], c["fit_mean"], c["psd"]))
    fast = np.asarray(co.gls_power_f64(t, y, dy, freq[pick], c["fit_mean"], c["psd"]))
    assert np.max(np.abs(fast - exact) / np.abs(exact)) <= 1e-8
    return np.asarray(co.gls_power_f64(t, y, dy, freq, c["fit_mean"], c["psd"])), pick, exact


@pytest.mark.gpu
def test_balanced_pieces(tmp_path):
    """S = 2, 301 tiles in 512 slots, N = 5000 (40 chunks; the last holds 8 samples): every tile is cut into pieces, each
    with its own remainders."""
    n, nf, tile = 5000, 300 * 2048 + 1000, 2048
    t, y, dy = curve(n, 7000 + n)
    c, arrays = make_case("s2_301", t, y, dy, nf, False, False)
    pair, plain = both(tmp_path, dict(PDC_GLS_S=2, PDC_GLS_BAL=1), [c], arrays)
    check_ran(pair, plain, c, route="balanced", S=2, tiles=301, bal_slots=512, bal_chunks=40)
    full, pick, exact = big_exact(c, arrays, tile, np.minimum(np.arange(0, nf, tile) + tile // 2 - 1, nf - 1))
    power = pair["s2_301_power"][0]
    tier_e(power[pick], exact, f"balanced (long double, {pick.size} bins)")
    tier_e(power, full, "balanced (every bin)")
    check_plain(pair, plain, c)


@pytest.mark.gpu
def test_sample_parts(tmp_path):
    """N = 60 000, nf = 3000: two tiles, the samples cut into parts dealt to the XCDs; every part sums its own chunks'
    remainders and gls_finish_kernel adds the parts."""
    n, nf = 60_000, 3000
    t, y, dy = curve(n, 41, period=12.3)
    c, arrays = make_case("parts", t, y, dy, nf, True, False)
    c["delta"] = 2e-7                                       # a zoom on the peak
    c["f0"] = 1 / 12.3 - (nf // 2) * c["delta"]
    pair, plain = both(tmp_path, dict(PDC_GLS_S=2), [c], arrays)
    check_ran(pair, plain, c, route="parts", S=2, tiles=2, wide_prep=1)
    rec = json.loads(str(pair["parts_rec"]))
    assert rec["parts"] >= 8 and rec["parts_by_xcd"] == 1, rec
    full, pick, exact = big_exact(c, arrays, 2048, np.arange(15, nf, 16))
    power = pair["parts_power"][0]
    tier_e(power[pick], exact, f"parts (long double, {pick.size} bins)")
    tier_e(power, full, "parts (every bin)")
    check_plain(pair, plain, c)
