"""The lead swap of the mirrored-pair GLS kernel (``GlsArgs::lead_swap`` in csrc/gls.hip).

Two column-waves that stream the same offset table take the two halves of every sample's row in opposite orders, so
that each leads on one half and finds the other in the scalar cache.  The accumulators of offsets m < 4 and m >= 4 are
disjoint registers, so the order changes no bit of any sum.  Every case runs in a child interpreter with
``PDC_GLS_K=16 PDC_GLS_PAIR=1 PDC_GLS_LEAD=1`` and again with ``PDC_GLS_LEAD=0`` (the switches are read once per
process, as in tests/test_gls_pair_gpu.py) and asserts

* power, amax and argmax of the two runs equal bit for bit (``np.array_equal``, NaNs equal);
* the same bits on a repeated call;
* ``lead_swap`` = 1 in the dispatch record of the first run and 0 in the second; 0 in both at S = 4, whose tile has
  one column (nothing shares a stream);
* independently of the library's other path: the N = 129 and N = 257 cases within Tier E (1e-6 relative, no bin of
  the exact spectrum under 1e-13 of its maximum, asserted) of the long-double sums of ``oracle.c_oracle``.

The shapes are the smallest at which an odd column owns live frequencies (nf = 2064 at S = 2: column 1 holds bins
1024 ... 2047, a second tile holds 16; nf = 4112 at S = 1: columns 1 and 3, a second tile) and every loop edge is met
(N = 1, 3, 64, 65, 129, 257: one sample, a stretch that ends inside a part, exactly one part, one part plus one
sample, a chunk plus one sample).  Three samples determine a mean, a sine and a cosine exactly, so N <= 3 runs without
the fitted mean; N = 129 runs all four (fit_mean, psd) pairs.  Grids start at f0 T = 0.1 and step by 1 / (5 T), as
tests/test_gls_pair_gpu.py explains; the far slab keeps that step and starts at f T = 25 000.

``PDC_GLS_BAL=1`` and ``PDC_GLS_Z=3`` take effect only where the dispatcher admits the route (balanced pieces: more
than 256 tiles and 32 chunks of samples; sample parts: N >= 16 384), so the two small cases under those switches
(N = 300 x 3 tiles; N = 700) run the general route - they are kept and the record is not asked for a route - and
``bal_real`` (257 tiles, N = 4097: a run covers pieces of two tiles) and ``parts_real`` (N = 16 384, three parts) are
the smallest shapes that do take them; there the route is asserted.
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
JD = 2.45e6
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
    t, y, dy = data[k + "_t"], data[k + "_y"], data[k + "_dy"]
    args = (t, y, dy, np.asarray(c["offsets"], dtype=np.int64), c["f0"], c["delta"], c["nf"], c["fit_mean"], c["psd"])
    power, amax, argmax = _cabi.gls_scan_batch(*args, want_peaks=True, j_begin=c["j_begin"])
    out[k + "_pair"] = np.array(_cabi.gls_last_pair(), dtype=np.int64)
    out[k + "_rec"] = json.dumps(_cabi.gls_last_dispatch())
    again = _cabi.gls_scan_batch(*args, want_peaks=True, j_begin=c["j_begin"])
    out[k + "_power"], out[k + "_amax"], out[k + "_argmax"] = power, amax, argmax
    out[k + "_same_bits"] = all(np.array_equal(p, q, equal_nan=True) for p, q in zip((power, amax, argmax), again))
np.savez(sys.argv[3], **out)
print("ok")
"""


def run_child(tmp, tag, env, cases, arrays):
    spec, inp, res = (str(tmp / f"{tag}.{ext}") for ext in ("json", "in.npz", "out.npz"))
    with open(spec, "w") as fh:
        json.dump(cases, fh)
    np.savez(inp, **arrays)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PDC_GLS_")}
    clean.update({k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, "-c", _CHILD, spec, inp, res], env=clean, cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stderr[-2000:])
    return np.load(res)


def curve(n, seed, period=37.3, span=None):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, float(span or max(n, 40)), n)) + JD
    dy = rng.uniform(0.05, 0.2, n)
    y = 1.0 + 0.5 * np.sin(2 * np.pi * t / period) + dy * rng.standard_normal(n)
    return t, y, dy


def make_case(name, curves, nf, fit_mean, psd, j_begin=0):
    """One call: `curves` = [(t, y, dy), ...] on one grid, f0 = delta / 2, delta = 1 / (5 T) of the longest span."""
    span = max(max(float(t[-1] - t[0]) for t, _, _ in curves), 40.0)     # (one sample: no span of its own)
    delta = 1.0 / span / 5.0
    offsets = np.concatenate([[0], np.cumsum([t.size for t, _, _ in curves])])
    case = dict(name=name, offsets=[int(o) for o in offsets], f0=0.5 * delta, delta=delta, nf=int(nf),
                fit_mean=bool(fit_mean), psd=bool(psd), j_begin=int(j_begin))
    arrays = {name + "_" + key: np.concatenate([c[i] for c in curves]) for i, key in enumerate(("t", "y", "dy"))}
    return case, arrays


def grid(c):
    return c["f0"] + c["delta"] * np.arange(c["j_begin"], c["j_begin"] + c["nf"])   # the device's fill rule


def build_groups():
    """{group: (switches, [case], arrays, lead_swap expected with PDC_GLS_LEAD=1)}"""
    groups = {}

    def add(group, env, want, case_arrays):
        g = groups.setdefault(group, (env, [], {}, want))
        g[1].append(case_arrays[0])
        g[2].update(case_arrays[1])

    s2 = dict(PDC_GLS_S=2)
    for n in (1, 3, 64, 65, 257):
        add("s2", s2, 1, make_case(f"s2_n{n}", [curve(n, 300 + n)], 2064, n > 3, False))
    for i, (fit_mean, psd) in enumerate(FOUR):
        add("s2", s2, 1, make_case(f"s2_n129_{i}", [curve(129, 429)], 2064, fit_mean, psd))
    # a curve's last read-ahead lands in the next curve's first row
    add("s2", s2, 1, make_case("s2_ragged", [curve(3, 51), curve(130, 52, span=130), curve(64, 53, span=130)], 2064,
                               False, False))
    add("s2", s2, 1, make_case("s2_far", [curve(129, 54)], 2064, True, False, j_begin=125_000))
    for n in (3, 65, 130):
        add("s1", dict(PDC_GLS_S=1), 1, make_case(f"s1_n{n}", [curve(n, 600 + n)], 4112, n > 3, False))
    add("s4", dict(PDC_GLS_S=4), 0, make_case("s4_n129", [curve(129, 71)], 1040, True, False))
    bal = dict(PDC_GLS_S=2, PDC_GLS_BAL=1)
    add("bal", bal, 1, make_case("bal_n300", [curve(300, 81)], 3 * 2048, True, False))
    add("bal", bal, 1, make_case("bal_real", [curve(4097, 82, span=400)], 256 * 2048 + 16, True, False))
    z3 = dict(PDC_GLS_S=2, PDC_GLS_Z=3)
    add("z3", z3, 1, make_case("z3_n700", [curve(700, 91)], 2064, True, False))
    add("z3", z3, 1, make_case("parts_real", [curve(16384, 92, span=2000)], 2064, True, False))
    return groups


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every group once with the swap and once without; shared, read-only."""
    tmp = tmp_path_factory.mktemp("lead")
    out = {}
    for name, (env, cases, arrays, want) in build_groups().items():
        base = dict(env, PDC_GLS_K=16, PDC_GLS_PAIR=1)
        out[name] = (env, cases, arrays, want,
                     run_child(tmp, name + "_lead", dict(base, PDC_GLS_LEAD=1), cases, arrays),
                     run_child(tmp, name + "_plain", dict(base, PDC_GLS_LEAD=0), cases, arrays))
    return out


GROUPS = ["s2", "s1", "s4", "bal", "z3"]


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_swapped_order_gives_the_same_bits(runs, group):
    env, cases, _, want, lead, plain = runs[group]
    for c in cases:
        k = c["name"]
        for key in ("_power", "_amax", "_argmax"):
            assert lead[k + key].shape == plain[k + key].shape and lead[k + key].size > 0
            assert np.array_equal(lead[k + key], plain[k + key], equal_nan=True), (k, key)
        assert lead[k + "_power"].shape == (len(c["offsets"]) - 1, c["nf"])
        assert bool(lead[k + "_same_bits"]) and bool(plain[k + "_same_bits"]), k
        n_total = c["offsets"][-1]
        for res, flag in ((lead, want), (plain, 0)):
            assert list(res[k + "_pair"]) == [1, (n_total + 2) * 256], (k, res[k + "_pair"])     # the pair kernel ran
            rec = json.loads(str(res[k + "_rec"]))
            assert rec["K"] == 16 and rec["S"] == env["PDC_GLS_S"] and rec["lead_swap"] == flag, (k, rec)


@pytest.mark.gpu
def test_the_forced_routes_ran(runs):
    """`bal_real` runs balanced pieces (257 tiles in 512 slots: every run covers pieces of two tiles), `parts_real`
    three sample parts."""
    _, _, _, _, lead, plain = runs["bal"]
    for res in (lead, plain):
        rec = json.loads(str(res["bal_real_rec"]))
        assert rec["route"] == "balanced" and rec["tiles"] == 257 and rec["bal_slots"] == 512, rec
    _, _, _, _, lead, plain = runs["z3"]
    for res in (lead, plain):
        rec = json.loads(str(res["parts_real_rec"]))
        assert rec["route"] == "parts" and rec["parts"] == 3 and rec["tiles"] == 2, rec


@pytest.mark.gpu
def test_tier_e_against_the_long_double_sums(runs):
    _, cases, arrays, _, lead, _ = runs["s2"]
    checked = 0
    for c in cases:
        k = c["name"]
        if c["offsets"][-1] not in (129, 257) or c["j_begin"]:
            continue
        exact = np.asarray(co.gls_power_exact(arrays[k + "_t"], arrays[k + "_y"], arrays[k + "_dy"], grid(c),
                                              c["fit_mean"], c["psd"]))
        power = lead[k + "_power"][0]
        ok = np.abs(exact) > FLOOR * np.nanmax(np.abs(exact))
        assert ok.all(), (k, int((~ok).sum()))          # the input condition: no bin under the floor
        rel = np.abs(power - exact) / np.abs(exact)
        print(f"LEAD-REL {k} max rel err {np.nanmax(rel):.3e}")
        assert np.all(np.isfinite(power)) and rel.max() <= RTOL, (k, rel.max(), int(np.argmax(rel)))
        checked += 1
    assert checked == 5          # N = 257 and the four (fit_mean, psd) pairs of N = 129
