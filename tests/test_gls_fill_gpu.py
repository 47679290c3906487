"""The table fill of the mirrored-pair GLS kernel after its tile-independent work moved to the prologue
(csrc/gls.hip: ``gls_pair_step_kernel``, ``gls_pair_chunk_kernel``, ``GlsArgs::chunk_sums``).

The two step sincos of a sample and the sixteen remainders ``G_m``, ``F_m`` of a chunk are made once per call with
the operations the fill used, and a wave of the fill runs one role.  No operand and no order of additions changes, so
the output must be the output of the commit before, bit for bit.  Every case runs in a child interpreter with
``PDC_GLS_K=16 PDC_GLS_PAIR=1`` (the switches are read once per process, as in tests/test_gls_lead_gpu.py), once with
the remainders taken from the per-call array and once with ``PDC_GLS_CHUNK_SUMS=0`` (every tile sums them in its fill,
the path a launch with unaligned stretches would take; no launch of today's dispatcher produces one: sample parts are
multiples of 128 samples), and asserts

* sha256 of the bytes of power, amax and argmax equal to the digests in tests/golden/gls_fill_digests.json, which were
  recorded with the library of the commit before this kernel change on the same seeded inputs
  (``PDC_LIBRARY=<that build> python tests/test_gls_fill_gpu.py OUT.json`` writes them);
* the same bits on a repeated call;
* ``chunk_sums`` in the dispatch record says which remainder path ran, and the forced routes ran;
* independently of the recorded digests: the N = 129 and N = 257 cases within Tier E (1e-6 relative, no bin of the
  exact spectrum under 1e-13 of its maximum, asserted) of the long-double sums of ``oracle.c_oracle``.

Shapes, the smallest that meet every edge of the new code: S = 2 with nf = 2064 (a second tile of 16 bins) and
N = 1, 3, 64, 65, 129, 257 (one sample; a chunk that ends inside a wave's part; exactly one part; one part plus one
sample; a chunk plus one sample; two chunks plus one), all four (fit_mean, psd) pairs at N = 129, a ragged batch of
3, 130 and 64 samples (chunk rows are counted from each curve's first sample, the read-ahead crosses a seam) and a far
slab; S = 1 with nf = 4112 (64-sample chunks: one walking and one chaining wave); S = 4; balanced pieces at 257 tiles
and N = 4097 (a run covers pieces of two tiles, so a piece starts at a chunk other than 0); sample parts at
N = 16 384 in three parts.  Three samples determine a mean, a sine and a cosine exactly, so N <= 3 runs without the
fitted mean.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gls_fill_digests.json")
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
    spec, inp, res = (os.path.join(str(tmp), f"{tag}.{ext}") for ext in ("json", "in.npz", "out.npz"))
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
    """{group: (switches, [case], arrays)}"""
    groups = {}

    def add(group, env, case_arrays):
        g = groups.setdefault(group, (env, [], {}))
        g[1].append(case_arrays[0])
        g[2].update(case_arrays[1])

    s2 = dict(PDC_GLS_S=2)
    for n in (1, 3, 64, 65, 257):
        add("s2", s2, make_case(f"s2_n{n}", [curve(n, 1300 + n)], 2064, n > 3, False))
    for i, (fit_mean, psd) in enumerate(FOUR):
        add("s2", s2, make_case(f"s2_n129_{i}", [curve(129, 1429)], 2064, fit_mean, psd))
    add("s2", s2, make_case("s2_ragged", [curve(3, 151), curve(130, 152, span=130), curve(64, 153, span=130)], 2064,
                            False, False))
    add("s2", s2, make_case("s2_far", [curve(129, 154)], 2064, True, False, j_begin=125_000))
    for n in (3, 65, 130):
        add("s1", dict(PDC_GLS_S=1), make_case(f"s1_n{n}", [curve(n, 1600 + n)], 4112, n > 3, False))
    add("s4", dict(PDC_GLS_S=4), make_case("s4_n129", [curve(129, 171)], 1040, True, False))
    add("bal", dict(PDC_GLS_S=2, PDC_GLS_BAL=1), make_case("bal_real", [curve(4097, 182, span=400)], 256 * 2048 + 16, True, False))
    add("z3", dict(PDC_GLS_S=2, PDC_GLS_Z=3), make_case("parts_real", [curve(16384, 192, span=2000)], 2064, True, False))
    return groups


GROUPS = ["s2", "s1", "s4", "bal", "z3"]
KEYS = ("power", "amax", "argmax")


def digests(res, cases):
    return {c["name"]: {key: hashlib.sha256(np.ascontiguousarray(res[c["name"] + "_" + key]).tobytes()).hexdigest() for key in KEYS}
            for c in cases}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every group once per remainder path; shared, read-only."""
    tmp = tmp_path_factory.mktemp("fill")
    out = {}
    for name, (env, cases, arrays) in build_groups().items():
        base = dict(env, PDC_GLS_K=16, PDC_GLS_PAIR=1)
        out[name] = (env, cases, arrays,
                     run_child(tmp, name + "_stored", dict(base, PDC_GLS_CHUNK_SUMS=1), cases, arrays),
                     run_child(tmp, name + "_infill", dict(base, PDC_GLS_CHUNK_SUMS=0), cases, arrays))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_bits_of_the_commit_before(runs, golden, group):
    env, cases, _, stored, infill = runs[group]
    for res, flag in ((stored, 1), (infill, 0)):
        got = digests(res, cases)
        for c in cases:
            k = c["name"]
            assert res[k + "_power"].shape == (len(c["offsets"]) - 1, c["nf"])
            assert got[k] == golden[k], (k, flag)
            assert bool(res[k + "_same_bits"]), (k, flag)
            n_total = c["offsets"][-1]
            assert list(res[k + "_pair"]) == [1, (n_total + 2) * 256], (k, res[k + "_pair"])     # the pair kernel ran
            rec = json.loads(str(res[k + "_rec"]))
            assert rec["K"] == 16 and rec["S"] == env["PDC_GLS_S"] and rec["chunk_sums"] == flag, (k, rec)


@pytest.mark.gpu
def test_the_forced_routes_ran(runs):
    """`bal_real` runs balanced pieces (257 tiles in 512 slots: every run covers pieces of two tiles), `parts_real`
    three sample parts of a multiple of the chunk, so their remainders come from the per-call array too."""
    for res in runs["bal"][3:]:
        rec = json.loads(str(res["bal_real_rec"]))
        assert rec["route"] == "balanced" and rec["tiles"] == 257 and rec["bal_slots"] == 512, rec
    for res in runs["z3"][3:]:
        rec = json.loads(str(res["parts_real_rec"]))
        assert rec["route"] == "parts" and rec["parts"] == 3 and rec["tiles"] == 2 and rec["z_len"] % 128 == 0, rec


@pytest.mark.gpu
def test_tier_e_against_the_long_double_sums(runs):
    from oracle import c_oracle as co
    _, cases, arrays, stored, _ = runs["s2"]
    checked = 0
    for c in cases:
        k = c["name"]
        if c["offsets"][-1] not in (129, 257) or c["j_begin"]:
            continue
        exact = np.asarray(co.gls_power_exact(arrays[k + "_t"], arrays[k + "_y"], arrays[k + "_dy"], grid(c),
                                              c["fit_mean"], c["psd"]))
        power = stored[k + "_power"][0]
        ok = np.abs(exact) > FLOOR * np.nanmax(np.abs(exact))
        assert ok.all(), (k, int((~ok).sum()))          # the input condition: no bin under the floor
        rel = np.abs(power - exact) / np.abs(exact)
        print(f"FILL-REL {k} max rel err {np.nanmax(rel):.3e}")
        assert np.all(np.isfinite(power)) and rel.max() <= RTOL, (k, rel.max(), int(np.argmax(rel)))
        checked += 1
    assert checked == 5          # N = 257 and the four (fit_mean, psd) pairs of N = 129


if __name__ == "__main__":
    # record the digests: run with PDC_LIBRARY naming a build of the commit before the kernel change
    import tempfile
    book = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (env, cases, arrays) in build_groups().items():
            res = run_child(tmp, name, dict(env, PDC_GLS_K=16, PDC_GLS_PAIR=1), cases, arrays)
            book.update(digests(res, cases))
    with open(sys.argv[1], "w") as fh:
        json.dump(book, fh, indent=1, sort_keys=True)
        fh.write("\n")
