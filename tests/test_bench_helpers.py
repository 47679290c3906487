"""CPU checks of bench.py's host-side helpers: the slab arithmetic of the sharded extras, the kernel matching
of the two roofline fields, and the CPU-baseline child process (multiprocessing.Pool as upstream,
/root/reference/src/periodicity/phase.py:69-70,185-186) at a toy size."""
import json
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_covers_the_grid_once():
    for total in (0, 1, 7, 4096, 100_000):
        for n in (1, 2, 3, 8):
            cuts = [bench.slab(total, n, i) for i in range(n)]
            assert cuts[0][0] == 0 and cuts[-1][1] == total
            assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
            assert max(e - b for b, e in cuts) <= -(-total // n) if total else True


def test_two_fracs_match_kernels_by_every_given_substring(tmp_path, monkeypatch):
    summ = {"src_sha": bench.source_hashes(), "kernels": {
        "pdm_scan_kernel<256, 4, true, 0> grid=1200384": {"SQ_INSTS_VALU": 1_000_000_000, "ms": 2.5, "GRBM_GUI_ACTIVE": 44_000_000},
        "pdm_scan_kernel<256, 4, true, 1> grid=1200384": {"SQ_INSTS_VALU": 1_100_000_000, "ms": 2.6},
        "pdm_scan_kernel<256, 4, false, 2> grid=400128": {"SQ_INSTS_VALU": 1_400_000_000, "ms": 2.8}}}
    path = tmp_path / "pmc.json"
    path.write_text(json.dumps(summ))
    monkeypatch.setattr(bench, "PMC_SUMMARY", str(path))
    fr, blk = bench.two_fracs(("pdm_scan_kernel<", ", 1> grid"), 2.6, 0.9, "unit")
    assert blk["kernel"].endswith(", 1> grid=1200384") and fr["algorithmic_frac"] == 0.9
    assert abs(fr["executed_issue_frac"] - 1.1e9 * 4 / 1024 / 2.4e9 / 2.6e-3) < 1e-3
    fr, blk = bench.two_fracs(("pdm_scan_kernel<", ", 0> grid"), 2.5, 1.0, "unit")
    assert "profiled_clock_GHz" in fr["executed_issue"] and 2.0 < fr["executed_issue"]["profiled_clock_GHz"] < 2.5
    fr, blk = bench.two_fracs("no_such_kernel", 1.0, None, "unit")
    assert blk is None and fr["executed_issue_frac"] is None and "no profiled" in fr["executed_issue_note"]


def test_cpu_pool_baseline_child_process_runs():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cpu_pool_baseline.py"), "16", "2"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-1500:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    assert res["cores"] == 2 and res["periods_sampled"] == 16
    for key in ("pdm", "stringlength"):
        assert res[key]["map_s"] > 0 and res[key]["Gpair_per_s"] > 0


def test_shared_axis_entry_finds_whichever_shared_kernel_ran(tmp_path, monkeypatch):
    """Round-5 defect: the c3_shared_t entry looked up "gls_shared_kernel" while `gls_shared2_kernel` is what runs
    (individual weights), so its issue fraction came back None.  The lookup key is now the common prefix."""
    mix = {c: 10 for c in bench.F64_COUNTERS}
    summ = {"src_sha": bench.source_hashes(), "kernels": {
        "gls_shared2_kernel<true> grid=12812288": dict(mix, SQ_INSTS_VALU=40_000_000_000, ms=88.0),
        "gls_scan_kernel<16, 0, 2, true> grid=131072": dict(mix, SQ_INSTS_VALU=13_000_000_000, ms=27.0)}}
    path = tmp_path / "pmc.json"
    path.write_text(json.dumps(summ))
    monkeypatch.setattr(bench, "PMC_SUMMARY", str(path))
    fr, blk = bench.two_fracs("gls_shared", 87.0, 2.0, "unit")
    assert blk is not None and blk["kernel"].startswith("gls_shared2_kernel") and fr["executed_issue_frac"] is not None
    assert bench.two_fracs("gls_shared_kernel", 87.0, 2.0, "unit")[1] is None      # the old key: no match


def test_executed_flops_are_counted_from_the_typed_counters():
    blk = {"mix": {"fma_f64": 12_651_000_000, "add_f64": 486_000_000, "mul_f64": 9_000_000}}
    got = bench.executed_flops(blk, 26.35)
    assert abs(got["TFLOPs"] - (2 * 12.651e9 + 0.486e9 + 0.009e9) * 64 / 26.35e-3 / 1e12) < 0.01     # 62.7 (round-5 verdict)
    assert 0.79 < got["frac_of_peak"] < 0.81
    assert bench.executed_flops(None, 1.0) is None and bench.executed_flops({"mix": {"fma_f64": 1}}, 1.0) is None


def test_fft_path_roofline_counts_passes_and_reads_the_traffic(tmp_path, monkeypatch):
    r = bench.fft_path_roofline(100_000, 1_000_000, 0.5)
    assert r["bound"] == "hbm" and r["nfft"] == 1 << 23 and r["passes_per_grid"] == 3 and r["grids"] == 3
    assert 1.5e9 < r["algorithmic_bytes"] < 2.2e9 and abs(r["frac"] - r["achieved"] / 8000.0) < 1e-3
    summ = {"src_sha": bench.source_hashes(), "kernels": {
        "fft_pass_lds_kernel<16> grid=524288": {"hbm_bytes": 200_000_000, "dispatches_per_pass": 36, "ms": 0.046},
        "glsfft_epilogue_kernel grid=1000192": {"hbm_bytes": 50_000_000, "dispatches_per_pass": 6, "ms": 0.02},
        "glsfft_epilogue_kernel grid=4096": {"hbm_bytes": 1_000, "dispatches_per_pass": 5, "ms": 0.002},
        "gls_scan_kernel<16, 0, 2, true> grid=131072": {"hbm_bytes": 1, "dispatches_per_pass": 6, "ms": 27.0}}}
    path = tmp_path / "pmc.json"
    path.write_text(json.dumps(summ))
    monkeypatch.setattr(bench, "PMC_SUMMARY", str(path))
    r = bench.fft_path_roofline(100_000, 1_000_000, 0.5)
    assert r["traffic"] == 6 * 200_000_000 + 50_000_000          # per launch: 36 / 6 pass dispatches + one epilogue
    summ["src_sha"]["glsfft.hip"] = "0" * 16
    path.write_text(json.dumps(summ))
    r = bench.fft_path_roofline(100_000, 1_000_000, 0.5)
    assert r["traffic"] is None and "stale" in r["traffic_note"]


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_the_same_way(tmp_path):
    small = np.linspace(0.0, 1.0, 1_000_000)                  # C2's power array: 8 MB, written whole
    bench.dump_outputs(str(tmp_path / "a"), power=small)
    assert np.array_equal(np.load(tmp_path / "a" / "power.npy"), small)
    assert not (tmp_path / "a" / "power_index.npy").exists()
    big = np.arange(8_000_000, dtype=np.float64) * 0.5        # loopback 8: 64 MB, a seeded sample under the limit
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), power=big)
    got, idx = np.load(tmp_path / "b" / "power.npy"), np.load(tmp_path / "b" / "power_index.npy")
    assert got.dtype == idx.dtype == np.float64 and got.nbytes + idx.nbytes <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(got, big[idx.astype(np.int64)]) and np.all(np.diff(idx) > 0)
    assert np.array_equal(got, np.load(tmp_path / "c" / "power.npy"))


def test_ss_oracle_full_grids_put_every_kind_of_period_in_every_batch_and_sub_batch():
    """tools/ss_oracle_full.py without a GPU: its spec parser, and the grid builder's promise for every spec of the seam
    test - a period beyond the baseline in each batch, with even sampling a commensurate one in each sub-batch and 40+
    consecutive commensurate periods inside one batch beyond its first 64 slots; the launch shape is asked of the
    library's own pdc_test_ss_shape (no device involved)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ss_oracle_full", os.path.join(ROOT, "tools", "ss_oracle_full.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from test_supersmoother_gpu import SEAM_SPECS, SWITCH_SPECS
    assert tool.parse_spec("4097x787e@3") == (4097, 787, "e", 3.0) and tool.parse_spec("300000x203du") == (300000, 203, "du", 0.0)
    for bad in ("4097", "10x10q", "x5"):
        try:
            tool.parse_spec(bad)
            raise AssertionError(bad)
        except ValueError:
            pass
    for text in [s for specs in SEAM_SPECS.values() for s in specs] + SWITCH_SPECS:
        n, n_per, flags, _ = tool.parse_spec(text)
        gt, gy, t, y = tool.make_curve(n, n_per, flags)
        assert np.all(np.diff(t) >= 0) and sorted(gt) == list(t)
        periods, kind = tool.build_grid(t, n_per, flags)
        base = t[-1] - t[0]
        assert periods.size == n_per and np.all(periods > 0) and np.all((periods > base) == (kind == 1)), text
        z = tool.shape_of(n, n_per)
        if text in SWITCH_SPECS:
            continue
        assert n_per > z["batch"], (text, z)                           # at least one batch seam
        assert n_per % z["batch"] != 0 or text == "50000x4096", text   # a partial last batch (the bench shape is whole)
        if z["sb"]:
            assert (n_per % z["batch"]) % z["sb"] % 8 != 0 or text == "50000x4096", (text, z)
        for p0 in range(0, n_per, z["batch"]):
            assert np.any(kind[p0:p0 + z["batch"]] == 1), (text, p0)
            for q0 in range(p0, min(p0 + z["batch"], n_per), z["sb"] or z["batch"]):
                if "e" in flags:
                    assert np.any(kind[q0:min(q0 + (z["sb"] or z["batch"]), p0 + z["batch"])] == 2), (text, q0)
        if "e" in flags:
            lo, hi = tool.STRETCH
            assert hi - lo >= 40 and np.all(kind[lo:hi] == 2) and lo >= 64 and hi <= z["batch"], (text, z)
    assert any(tool.shape_of(*tool.parse_spec(s)[:2])["sb"] not in (0, tool.shape_of(*tool.parse_spec(s)[:2])["batch"])
               for s in SEAM_SPECS["lds_tiled"] + SEAM_SPECS["bench"])      # some spec does cross a sub-batch seam
