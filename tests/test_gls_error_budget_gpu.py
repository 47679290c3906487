"""Every route of the GLS direct sums against its DERIVED rounding budget (tests/gls_error_budget.py).

The other GLS tests gate on Tier E, 1e-6 of the power: the contract with BASELINE, six to eight orders above what the
arithmetic is built to hold.  Here every route - the general kernel in all nine (K, S) shapes, the mirrored-pair kernel
with and without the lead swap, sample parts on grid.y and dealt to the XCDs, the wide prologue, balanced pieces forced
and by the cost model, the three shared-time-axis kernels, the bootstrap by index and the ragged batch - is held to

    |p_dev - p_exact| <= 2 bound_p + 64 u |p_exact|        on every picked bin, none left out,

with bound_p propagated in first order from ``|sigma_dev - sigma_exact| <= C_route u A_sigma`` on the six raw sums, and the
raw sums of ``pdc_trig_sums`` to ``C_route u sum |w|`` directly.  C_route comes from the launch the dispatch hook reports
(K, S, parts, z_len, the prologue that ran), never from what the device returns.  The inputs sit on a lattice on which
the grid, ``t - t[0]`` and the fractional phase are exact, the reference is ``oracle_gls_sums_reduced`` (pinned to integer
arithmetic by the host test), and one case of every route runs on a slab at ~4e6 cycles, where ``lo`` of
``frac_product`` is live.  Every case first asserts the route through the hooks and prints ``worst |err| / gate``
(profiles/r22_gls_error_budget.txt keeps the figures).  Each group of cases runs in a child interpreter: the
``PDC_GLS_*`` switches are read once per process.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gls_error_budget as eb
from test_gls_dispatch_gpu import check_record, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
    if c["kind"] == "raw":
        out[k + "_S"], out[k + "_C"] = _cabi.trig_sums(t, y, c["f0"], c["delta"], c["nf"])
    elif c["kind"] == "boot":
        out[k + "_amax"], out[k + "_arg"] = _cabi.gls_bootstrap(t, y, dy, data[k + "_picks"], c["f0"], c["delta"], c["nf"],
                                                                c["fit_mean"], c["psd"])
    elif c["kind"] == "ragged":
        power, amax, arg = _cabi.gls_scan_ragged(t, y, dy, np.array(c["offsets"]), np.array(c["f0s"]), np.array(c["deltas"]),
                                                 np.array(c["f_offsets"]), c["fit_mean"], c["psd"], want_power=True,
                                                 want_peaks=True)
        out[k + "_power"], out[k + "_amax"], out[k + "_arg"] = power, amax, arg
    else:
        offsets = np.arange(c["B"] + 1, dtype=np.int64) * c["n"]
        power, amax, arg = _cabi.gls_scan_batch(t, y, dy, offsets, c["f0"], c["delta"], c["nf"], c["fit_mean"], c["psd"],
                                                c["shared_t"], want_power=True, want_peaks=True, j_begin=c["j_begin"])
        out[k + "_power"], out[k + "_amax"], out[k + "_arg"] = power, amax, arg
    if c["kind"] != "ragged":
        out[k + "_rec"] = json.dumps(_cabi.gls_last_dispatch())
        out[k + "_pair"] = np.array(_cabi.gls_last_pair()[0])
np.savez(sys.argv[3], **out)
print("ok")
"""


def run_child(tmp_path, tag, env, cases, arrays):
    """``run_child`` of tests/test_gls_dispatch_gpu.py for this file's calls: one fresh interpreter with the
    ``PDC_GLS_*`` switches of ``env`` and no others."""
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


def child_case(case, arrays):
    """A case of gls_error_budget.GROUPS as the child wants it (floats for f0 / delta), and its arrays under its name."""
    k = case["name"]
    named = {f"{k}_{a}": v for a, v in arrays.items() if a != "T"}
    c = dict(name=k, kind=case["kind"], fit_mean=case["fit_mean"], psd=case["psd"])
    if case["kind"] == "ragged":
        c.update(offsets=[0] + list(np.cumsum(case["ns"]).tolist()), f_offsets=[0] + list(np.cumsum(case["nfs"]).tolist()),
                 f0s=[F / 2.0 ** eb.FBITS for F in case["F0s"]], deltas=[D / 2.0 ** eb.FBITS for D in case["Ds"]])
    else:
        c.update(n=case["n"], nf=case["nf"], B=case["B"], shared_t=case["shared_t"], j_begin=case["j_begin"],
                 f0=case["F0"] / 2.0 ** eb.FBITS, delta=case["D"] / 2.0 ** eb.FBITS)
    return c, named


@pytest.mark.parametrize("group", list(eb.GROUPS))
def test_power_within_its_budget(tmp_path, group):
    g = eb.GROUPS[group]
    cases, arrays, inputs = [], {}, {}
    for case in g["cases"]:
        inputs[case["name"]] = eb.case_arrays(group, case)
        c, named = child_case(case, inputs[case["name"]])
        cases.append(c)
        arrays.update(named)
    res = run_child(tmp_path, group, g["env"], cases, arrays)
    for case in g["cases"]:
        k = case["name"]
        label = f"{group} {k}"
        if case["kind"] == "ragged":
            rec = dict(route="ragged")       # (one kernel, no dispatcher: gls_ragged.hip)
        else:
            rec = record(res, k + "_rec")
            check_record(rec, **eb.expected_record(group, case))
            assert bool(res[k + "_pair"]) == g["pair"], label
        worst = 0.0
        for curve in eb.case_curves(group, case, inputs[k]):
            name, t, y, dy, F0, D, j_begin, nf, row, offset = curve
            consts = eb.route_constants(rec, t.size, pair=g["pair"])
            dev_arg = int(res[k + "_arg"][row])
            pick, p, bound, unit = eb.curve_reference(group, case, curve, consts, extra=(dev_arg - 1, dev_arg, dev_arg + 1))
            assert (bound > eb.CAP * unit).sum() <= 0.01 * pick.size, label
            gate = eb.gate(bound, p)
            if case["kind"] == "boot":      # only the maxima come back
                at = int(np.argmax(p))
                assert pick[at] == dev_arg, (label, name)
                err = np.abs(np.longdouble(res[k + "_amax"][row]) - p[at]) / gate[at]
            else:
                power = res[k + "_power"]
                dev = power[offset:offset + nf] if case["kind"] == "ragged" else power[row]
                assert np.all(np.isfinite(dev)), label
                ratio = np.abs(dev[pick].astype(np.longdouble) - p) / gate
                err = ratio.max()
                at = int(np.argmax(ratio))
                # the peak: the oracle's argmax over the picked bins (they hold the device's peak and its neighbours)
                assert pick[int(np.argmax(p))] == dev_arg, (label, name, dev_arg)
                assert res[k + "_amax"][row] == dev[dev_arg], (label, name)
            worst = max(worst, float(err))
            assert err <= 1, (label, name, float(err), int(pick[at]), consts)
        print(f"BUDGET {label}: route {rec['route']} K={rec.get('K')} S={rec.get('S')} parts={rec.get('parts')} "
              f"C = {consts[0]} / {consts[1]}: worst |err| / gate = {worst:.4f}")


def test_raw_sums_within_their_budget(tmp_path):
    """``pdc_trig_sums`` (MODE_RAW): |S_dev - S_exact| and |C_dev - C_exact| <= C_route u sum |w| on the picked bins of a
    2049-bin grid, n = 129 and 4000, from delta / 2 and from ~4e6 cycles (the table fill's ``lo``, the records')."""
    cases, arrays = [], {}
    for k, c in eb.RAW.items():
        t, h, T = eb.raw_inputs(c)
        cases.append(dict(name=k, kind="raw", nf=c["nf"], f0=c["F0"] / 2.0 ** eb.FBITS, delta=c["D"] / 2.0 ** eb.FBITS,
                          fit_mean=False, psd=False))
        arrays.update({k + "_t": t, k + "_y": h})
    res = run_child(tmp_path, "raw", {}, cases, arrays)
    for k, c in eb.RAW.items():
        rec = record(res, k + "_rec")
        check_record(rec, route="general", parts=1, wide_prep=0, bal_slots=0)
        assert rec["K"] in (4, 8, 16) and rec["S"] in (1, 2, 4) and not bool(res[k + "_pair"])
        tile = 256 // rec["S"] * rec["K"]
        assert rec["tiles"] == -(-c["nf"] // tile)
        pick = eb.pick_bins(c["nf"], tile, limit=1024 if c["n"] < 1000 else 512)
        S, C, A = eb.raw_exact(c, pick)
        c_lin = eb.route_constants(rec, c["n"], raw=True)[0]
        gate = c_lin * np.longdouble(eb.U) * A
        err = max(np.abs(res[k + "_S"][pick] - S).max(), np.abs(res[k + "_C"][pick] - C).max()) / gate
        print(f"BUDGET raw {k}: route general K={rec['K']} S={rec['S']} C = {c_lin}: worst |err| / gate = {float(err):.4f}")
        assert err <= 1, (k, float(err), c_lin)
