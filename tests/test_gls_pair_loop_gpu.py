"""The sample loop of the mirrored-pair GLS kernel after its addressing changed (csrc/gls.hip, the ``PAIR`` branch of
``gls_scan_kernel``): three bases fixed per chunk, one unsigned byte offset for the table rows and one for the records,
advanced per sample, instead of three 64-bit addresses rebuilt from the sample index.

No operand and no order of additions changes, so the output must be the output of the commit before, bit for bit.
Every case runs in a child interpreter with ``PDC_GLS_K=16 PDC_GLS_PAIR=1`` (the switches are read once per process,
as in tests/test_gls_fill_gpu.py) and asserts

* sha256 of the bytes of power, amax and argmax equal to the digests in tests/golden/gls_pair_loop_digests.json, which
  were recorded with the library of the commit before this kernel change on the same seeded inputs
  (``PDC_LIBRARY=<that build> python tests/test_gls_pair_loop_gpu.py OUT.json`` writes them);
* the same bits on a repeated call;
* the dispatch record shows the pair kernel, the forced S and, where asked for, the lead swap;
* independently of the recorded digests: the N = 66 and N = 193 cases within Tier E (1e-6 relative, no bin of the
  exact spectrum under 1e-13 of its maximum, asserted) of the long-double sums of ``oracle.c_oracle``.

Shapes: the trip counts and starting offsets of a wave's stretch that tests/test_gls_fill_gpu.py does not meet.  A wave
of part p starts at sample p * (chunk / S) of a chunk, so its offsets start at 0 only in part 0.
S = 2 (parts of 64 samples, nf = 2064: a second tile of 16 bins): N = 2, 63, 66, 127, 128, 130, 191, 193 - a second
part with 0, 1 (N = 193: of the second chunk), 2, 63 and 64 trips, a chunk boundary after an odd and after an even
number of trips; the same shapes with ``PDC_GLS_LEAD=1``, where both table bases move by the lead swap's quarter; a
ragged batch of 2, 66 and 63 samples (the read-ahead crosses a curve seam at both parities).  S = 4 (parts of 32):
N = 31, 33, 95, 97.  S = 1 (64-sample chunks, nf = 4112): N = 63, 66.  Three samples determine a mean, a sine and a
cosine exactly, so N <= 3 runs without the fitted mean.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gls_pair_loop_digests.json")
RTOL = 1e-6            # Tier E (BASELINE.json north_star)
FLOOR = 1e-13
JD = 2.45e6

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


def make_case(name, curves, nf, fit_mean, psd=False, j_begin=0):
    """One call: `curves` = [(t, y, dy), ...] on one grid, f0 = delta / 2, delta = 1 / (5 T) of the longest span."""
    span = max(max(float(t[-1] - t[0]) for t, _, _ in curves), 40.0)     # (two samples: hardly a span of their own)
    delta = 1.0 / span / 5.0
    offsets = np.concatenate([[0], np.cumsum([t.size for t, _, _ in curves])])
    case = dict(name=name, offsets=[int(o) for o in offsets], f0=0.5 * delta, delta=delta, nf=int(nf),
                fit_mean=bool(fit_mean), psd=bool(psd), j_begin=int(j_begin))
    arrays = {name + "_" + key: np.concatenate([c[i] for c in curves]) for i, key in enumerate(("t", "y", "dy"))}
    return case, arrays


def grid(c):
    return c["f0"] + c["delta"] * np.arange(c["j_begin"], c["j_begin"] + c["nf"])   # the device's fill rule


S2_SIZES = (2, 63, 66, 127, 128, 130, 191, 193)


def build_groups():
    """{group: (switches, [case], arrays)}"""
    groups = {}

    def add(group, env, case_arrays):
        g = groups.setdefault(group, (env, [], {}))
        g[1].append(case_arrays[0])
        g[2].update(case_arrays[1])

    for group, env in (("s2", dict(PDC_GLS_S=2, PDC_GLS_LEAD=0)), ("lead", dict(PDC_GLS_S=2, PDC_GLS_LEAD=1))):
        for n in S2_SIZES:
            add(group, env, make_case(f"{group}_n{n}", [curve(n, 3100 + n)], 2064, n > 3))
        add(group, env, make_case(f"{group}_ragged", [curve(2, 351), curve(66, 352, span=66), curve(63, 353, span=66)],
                                  2064, False))
    for n in (31, 33, 95, 97):
        add("s4", dict(PDC_GLS_S=4, PDC_GLS_LEAD=0), make_case(f"s4_n{n}", [curve(n, 3400 + n)], 2064, True))
    for n in (63, 66):
        add("s1", dict(PDC_GLS_S=1, PDC_GLS_LEAD=0), make_case(f"s1_n{n}", [curve(n, 3600 + n)], 4112, True))
    return groups


GROUPS = ["s2", "lead", "s4", "s1"]
KEYS = ("power", "amax", "argmax")


def digests(res, cases):
    return {c["name"]: {key: hashlib.sha256(np.ascontiguousarray(res[c["name"] + "_" + key]).tobytes()).hexdigest() for key in KEYS}
            for c in cases}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every group once; shared, read-only."""
    tmp = tmp_path_factory.mktemp("pair_loop")
    out = {}
    for name, (env, cases, arrays) in build_groups().items():
        out[name] = (env, cases, arrays, run_child(tmp, name, dict(env, PDC_GLS_K=16, PDC_GLS_PAIR=1), cases, arrays))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_bits_of_the_commit_before(runs, golden, group):
    env, cases, _, res = runs[group]
    got = digests(res, cases)
    for c in cases:
        k = c["name"]
        assert res[k + "_power"].shape == (len(c["offsets"]) - 1, c["nf"])
        assert got[k] == golden[k], k
        assert bool(res[k + "_same_bits"]), k
        n_total = c["offsets"][-1]
        assert list(res[k + "_pair"]) == [1, (n_total + 2) * 256], (k, res[k + "_pair"])     # the pair kernel ran
        rec = json.loads(str(res[k + "_rec"]))
        assert rec["K"] == 16 and rec["S"] == env["PDC_GLS_S"] and rec["lead_swap"] == env["PDC_GLS_LEAD"], (k, rec)


@pytest.mark.gpu
def test_the_lead_swap_changes_no_bit(runs):
    """The halves of a row feed disjoint sums: the swapped waves' bases start two quarters apart, the bits stay."""
    _, plain_cases, _, plain = runs["s2"]
    _, lead_cases, _, lead = runs["lead"]
    assert len(plain_cases) == len(lead_cases) == len(S2_SIZES) + 1
    for p, q in zip(plain_cases, lead_cases):
        for key in KEYS:
            assert np.array_equal(plain[p["name"] + "_" + key], lead[q["name"] + "_" + key], equal_nan=True), (q["name"], key)


@pytest.mark.gpu
def test_tier_e_against_the_long_double_sums(runs):
    from oracle import c_oracle as co
    _, cases, arrays, res = runs["s2"]
    checked = 0
    for c in cases:
        k = c["name"]
        if c["offsets"] not in ([0, 66], [0, 193]):
            continue
        exact = np.asarray(co.gls_power_exact(arrays[k + "_t"], arrays[k + "_y"], arrays[k + "_dy"], grid(c),
                                              c["fit_mean"], c["psd"]))
        power = res[k + "_power"][0]
        ok = np.abs(exact) > FLOOR * np.nanmax(np.abs(exact))
        assert ok.all(), (k, int((~ok).sum()))          # the input condition: no bin under the floor
        rel = np.abs(power - exact) / np.abs(exact)
        print(f"PAIR-LOOP-REL {k} max rel err {np.nanmax(rel):.3e}")
        assert np.all(np.isfinite(power)) and rel.max() <= RTOL, (k, rel.max(), int(np.argmax(rel)))
        checked += 1
    assert checked == 2          # N = 66 and N = 193


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
