"""The route of the phase-binning scans (PDM theta, AoV, conditional entropy, Gregory-Loredo), asked of the library's own
plan function at every boundary of its ladder.  No device is touched: ``pdc_test_phase_shape`` runs ``phase_route`` of
csrc/pdm.hip, the one function the launcher takes its route from, and honours ``PDC_PDM_SPLIT`` / ``PDC_PDM_NZ`` as the
launcher does.  The switches are read once per process, so every question is put to a child interpreter whose
environment holds exactly the switches the case names.

The expected values are worked out here from the rules in ``phase_route``, with the arithmetic beside them:

* unsplit instance by period groups ``G = ceil(P / 64)``: ``<256, 4>`` below 2048, ``<256, 2>`` from 2048, ``<256, 1>``
  from 4096, and ``<64, 1>`` whenever ``lds(last, 256)`` exceeds 150 KB, with
  ``lds(last, block) = 16 max(256, block) + hist + 8 (last + 2) + 64`` and ``hist = 12 (last + 1) block`` for the kinds
  that keep sums, ``4 ((last + 2) // 2 + 1) block`` for the counts-only kinds;
* split mode from 8192 samples on when both kernels' histograms fit: ``G < 768`` asks for ``ceil(4096 / 4G)`` slices,
  otherwise the rounds-filled score picks 1 .. 16 slices or none; at most ``n // 2048`` slices, slice length a multiple
  of 256 samples;
* the counts-only kinds must cut more than 65 280 samples whatever else is decided.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PDM, AOV, CE, GL = 0, 1, 2, 4
SCAN_LDS_CAP, FINISH_LDS_CAP = 150 * 1024, 128 * 1024        # what the launcher raises the two kernels' limits to
CELL_SAMPLES = 65280
# one small histogram per kind, (nb, nc) as pdc_phase_scan_dev takes them: PDM 5 x 2, AoV 10 bins, conditional entropy
# 10 x 5 cells, Gregory-Loredo m = 6 with 4 offsets
SMALL = {PDM: (5, 2), AOV: (10, 1), CE: (10, 5), GL: (24, 6)}

_CHILD = r"""
import json, sys
from periodicity_amd import _cabi
lib = _cabi.lib()
out = []
for kind, n, P, nb, nc in json.load(open(sys.argv[1])):
    out.append([_cabi.phase_shape(kind, n, P, nb, nc), int(lib.pdc_phase_work_bytes(kind, n, P, nb, nc))])
json.dump(out, open(sys.argv[2], "w"))
print("ok")
"""


def ask(tmp_path, shapes, **env):
    """``(plan, pdc_phase_work_bytes)`` per ``(kind, n, P, nb, nc)`` from a fresh interpreter whose only ``PDC_PDM_*``
    variables are ``env``."""
    spec, res = str(tmp_path / "shapes.json"), str(tmp_path / "plans.json")
    with open(spec, "w") as fh:
        json.dump([[int(v) for v in s] for s in shapes], fh)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PDC_PDM_")}
    clean.update({k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, "-c", _CHILD, spec, res], env=clean, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stderr[-2000:])
    return [tuple(p) for p in json.load(open(res))]


def last_bin(kind, nb, nc):
    return (nb + 1) * nc - 1 if kind == CE else (nb if kind in (AOV, GL) else nb * nc)


def lds(kind, nb, nc, block):
    last = last_bin(kind, nb, nc)
    hist = 4 * ((last + 2) // 2 + 1) * block if kind in (CE, GL) else 12 * (last + 1) * block
    return 16 * max(256, block) + hist + 8 * (last + 2) + 64


def scratch_bytes(plan, kind, nb, nc):
    """What the split mode's arrays take (PdmArgs in csrc/pdm.hip): 3 x 512 statistics' partial sums, then per slice and
    padded period the histogram's sums and counts and the two overflow sums - counts alone, two cells per word, for the
    counts-only kinds."""
    if not plan["split"]:
        return 0
    bins, pad, z = last_bin(kind, nb, nc) + 1, 64 * plan["workgroups"], plan["n_z"]
    if kind in (CE, GL):
        return 3 * 512 * 8 + z * ((bins + 1) // 2) * pad * 4
    return 3 * 512 * 8 + z * bins * pad * 8 + z * 2 * pad * 8 + z * bins * pad * 4


def unsplit(kind, block, waves, P, nb, nc):
    per = block // waves
    return dict(kind=kind, split=0, block=block, waves=waves, periods_per_wg=per, workgroups=-(-P // per), n_z=1,
                z_len=0, n_stat=0, scan_lds=lds(kind, nb, nc, block), finish_lds=0)


def split(kind, n, P, nb, nc, n_z, z_len):
    bins = last_bin(kind, nb, nc) + 1
    return dict(kind=kind, split=1, block=256, waves=4, periods_per_wg=64, workgroups=-(-P // 64), n_z=n_z, z_len=z_len,
                n_stat=min(512, -(-n // 1024)), scan_lds=lds(kind, nb, nc, 256),
                finish_lds=bins * 64 * (8 if kind in (CE, GL) else 16))


def test_the_lds_rule_restated_here_is_the_issue_s_arithmetic():
    assert lds(PDM, 47, 1, 256) == 152008 and lds(AOV, 47, 1, 256) == 152008 <= SCAN_LDS_CAP
    assert lds(PDM, 48, 1, 256) == 155088 > SCAN_LDS_CAP
    assert lds(PDM, 5, 2, 256) == 38048


def test_period_count_picks_the_unsplit_instance(tmp_path):
    """n = 387 is far below the split threshold.  131 008 = 2047 x 64 periods; 131 009 make 2048 groups; 262 080 =
    4095 x 64; 262 081 make 4096."""
    ladder = ((131_008, 4, 2047), (131_009, 2, 1024), (262_080, 2, 2048), (262_081, 1, 1024))
    shapes = [(kind, 387, P) + SMALL[kind] for kind in SMALL for P, _, _ in ladder]
    plans = iter(ask(tmp_path, shapes))
    for kind in SMALL:
        for P, waves, wgs in ladder:
            plan, work = next(plans)
            assert plan == unsplit(kind, 256, waves, P, *SMALL[kind]), (kind, P, plan)
            assert plan["workgroups"] == wgs and work == 0


def test_histogram_size_picks_the_block(tmp_path):
    """47 fine bins are the most a [bin][thread] histogram of 256 threads holds under the 150 KB cap (152 008 B); 48
    (155 088 B) fall to one wave per workgroup, at any period count.  The counts-only kinds stay at 256 threads up to
    the 191-bin limit of every kind (two 16-bit cells per word)."""
    shapes, want = [], []
    for kind, nb47, nb48 in ((PDM, (47, 1), (48, 1)), (PDM, (1, 47), (6, 8)), (AOV, (47, 1), (48, 1))):
        for n, P in ((3000, 130), (3000, 262_081), (8191, 64)):
            shapes += [(kind, n, P) + nb47, (kind, n, P) + nb48]
            want += [unsplit(kind, 256, 1 if P == 262_081 else 4, P, *nb47), unsplit(kind, 64, 1, P, *nb48)]
    for plan, exp in zip(ask(tmp_path, shapes), want):
        assert plan[0] == exp and plan[0]["scan_lds"] <= SCAN_LDS_CAP, plan
    assert all(w["scan_lds"] == 152008 for w in want[0::2]) and all(w["scan_lds"] == 42192 for w in want[1::2])
    # split mode needs the 256-thread histogram: 47 bins split 9000 samples x 64 periods (one group asks for 1024
    # slices, 9000 // 2048 = 4 are allowed, of ceil(2250 / 256) x 256 = 2304 samples), 48 bins stay unsplit on <64, 1>
    for kind in (PDM, AOV):
        (p47, w47), (p48, w48) = ask(tmp_path, [(kind, 9000, 64, 47, 1), (kind, 9000, 64, 48, 1)])
        assert p47 == split(kind, 9000, 64, 47, 1, 4, 2304) and p47["scan_lds"] == 152008 and p47["finish_lds"] == 49152
        assert p48 == unsplit(kind, 64, 1, 64, 48, 1) and w48 == 0 and w47 >= scratch_bytes(p47, kind, 47, 1)
    big = [(CE, 190, 1), (CE, 18, 10), (CE, 94, 2), (GL, 190, 10), (GL, 190, 190), (GL, 189, 1)]
    shapes = [(kind, n, P, nb, nc) for kind, nb, nc in big for n, P in ((3000, 130), (9000, 64), (70_000, 300_000))]
    for plan, _ in ask(tmp_path, shapes) + ask(tmp_path, shapes, PDC_PDM_SPLIT=0):
        assert plan["block"] == 256 and plan["scan_lds"] <= SCAN_LDS_CAP and plan["finish_lds"] <= FINISH_LDS_CAP, plan


def test_split_threshold_and_the_two_slice_rules(tmp_path):
    """32 chunks of 256 samples open the split mode.  767 period groups (49 088 periods) are the last the few-groups rule
    takes: ceil(4096 / 3068) = 2 slices of 4096.  768 groups go to the score: 4 PDM workgroups of 38 048 + 512 B fit a
    CU, 1024 slots; unsplit fills 768 / 1024 of one round and scores 0.75 - 0.05 = 0.70; z slices fill 768 z / (1024
    ceil(768 z / 1024)) = 0.75, 0.75, 0.75, 1.0 for z = 1 .. 4 = 8192 // 2048 and cost 0.012 z (5e4 / 8192) = 0.0732 z:
    only z = 4 (1.0 - 0.293 = 0.707) beats 0.70."""
    for kind in SMALL:
        nbc = SMALL[kind]
        plans = ask(tmp_path, [(kind, n, P) + nbc for n in (8191, 8192) for P in (49_088, 49_089)])
        assert plans[0][0] == unsplit(kind, 256, 4, 49_088, *nbc) and plans[1][0] == unsplit(kind, 256, 4, 49_089, *nbc)
        assert plans[2][0] == split(kind, 8192, 49_088, *nbc, 2, 4096), plans[2]
        # AoV at 10 bins is PDM's 38 048 B; conditional entropy at 10 x 5 cells takes 34 304 + 512 B, 4 per CU as well.
        # Gregory-Loredo's 25 fine bins take 18 704 + 512 B: the cap of 8 per CU, 2048 slots - unsplit 0.375 - 0.05,
        # z = 1 .. 4 fill 0.375, 0.75, 0.5625, 0.75: z = 2 (0.75 - 0.146) wins.
        want = split(kind, 8192, 49_089, *nbc, 2, 4096) if kind == GL else split(kind, 8192, 49_089, *nbc, 4, 2048)
        assert plans[3][0] == want, plans[3]
        assert plans[2][1] == scratch_bytes(plans[2][0], kind, *nbc) and plans[3][1] == scratch_bytes(want, kind, *nbc)


def test_the_score_may_decline_to_split(tmp_path):
    """2048 groups: the unsplit <256, 2> launch has 1024 workgroups, exactly one round of 1024 slots: 1.0 - 0.05 = 0.95.
    At n = 8192 a slice costs 0.0732: nothing reaches 0.95.  At n = 50 000 (slices of at most 16 384 samples: from 4 on,
    at most 24) 4 slices fill 8192 / 8192 and cost 0.048: 0.952 > 0.95; 5 cost 0.06.  Slices of ceil(12 500 / 256) x 256
    = 12 544 samples."""
    (declined, w0), (taken, w1) = ask(tmp_path, [(PDM, 8192, 131_009, 5, 2), (PDM, 50_000, 131_009, 5, 2)])
    assert declined == unsplit(PDM, 256, 2, 131_009, 5, 2) and w0 == 0
    assert taken == split(PDM, 50_000, 131_009, 5, 2, 4, 12_544) and w1 >= scratch_bytes(taken, PDM, 5, 2)
    # PDC_PDM_NZ stands in for the score's answer, and only there: 3 slices of ceil(2731 / 256) x 256 = 2816 samples
    forced = ask(tmp_path, [(PDM, 8192, 131_009, 5, 2), (PDM, 8192, 49_088, 5, 2), (PDM, 8191, 131_009, 5, 2)],
                 PDC_PDM_NZ=3)
    assert forced[0][0] == split(PDM, 8192, 131_009, 5, 2, 3, 2816)
    assert forced[1][0] == split(PDM, 8192, 49_088, 5, 2, 2, 4096)
    assert forced[2][0] == unsplit(PDM, 256, 2, 131_009, 5, 2)


@pytest.mark.parametrize("env", [{}, {"PDC_PDM_SPLIT": 0}], ids=["default", "split_off"])
def test_counts_only_kinds_cut_long_curves(tmp_path, env):
    """Two 16-bit cells per word: a workgroup bins at most 65 280 samples, with or without the optional split."""
    sizes = (65_280, 65_281, 130_560, 130_561, 140_000, 1_000_000)
    grids = (33, 5000, 131_009, 262_081)
    shapes = [(kind, n, P) + SMALL[kind] for kind in (CE, GL) for n in sizes for P in grids]
    shapes += [(CE, n, 33, 190, 1) for n in sizes] + [(CE, n, 33, 18, 10) for n in sizes]
    for (kind, n, P, nb, nc), (plan, work) in zip(shapes, ask(tmp_path, shapes, **env)):
        if plan["split"]:
            assert plan["z_len"] <= CELL_SAMPLES and plan["z_len"] % 256 == 0, plan
            assert plan["n_z"] * plan["z_len"] >= n > (plan["n_z"] - 1) * plan["z_len"], plan
            assert work >= scratch_bytes(plan, kind, nb, nc)
        else:
            assert n <= CELL_SAMPLES and work == 0, plan
        if env:      # nothing but the forced slices: ceil(n / 65 280) of them, unsplit up to 65 280 samples
            assert plan["split"] == int(n > CELL_SAMPLES) and plan["n_z"] == -(-n // CELL_SAMPLES), plan
    if env:          # 65 281 samples: two slices of ceil(32 641 / 256) x 256
        (plan, _), = ask(tmp_path, [(GL, 65_281, 33, 24, 6)], **env)
        assert plan == split(GL, 65_281, 33, 24, 6, 2, 32_768)
    # the kinds that keep sums are never forced
    for plan, _ in ask(tmp_path, [(PDM, 1_000_000, 33, 5, 2), (AOV, 70_000, 262_081, 10, 1)], PDC_PDM_SPLIT=0):
        assert plan["split"] == 0


def test_more_slices_than_the_finishing_kernel_has_waves(tmp_path):
    """One period group asks for 1024 slices; 34 816 // 2048 = 17 are allowed, of exactly 2048 samples: one more than
    the 16 waves of pdm_finish_kernel, so its wave 0 adds two slices."""
    for kind in SMALL:
        (plan, work), = ask(tmp_path, [(kind, 34_816, 64) + SMALL[kind]])
        assert plan == split(kind, 34_816, 64, *SMALL[kind], 17, 2048) and work >= scratch_bytes(plan, kind, *SMALL[kind])
    (plan, _), = ask(tmp_path, [(PDM, 1 << 20, 64, 5, 2)])
    assert plan == split(PDM, 1 << 20, 64, 5, 2, 512, 2048)


def test_invariants_over_a_seeded_sweep(tmp_path):
    """A few thousand shapes, around every threshold and far from them: both kernels' LDS within what the launcher
    raises their limits to, the workspace the size function reports holds the plan's arrays, the grid covers the
    periods, the slices cover the samples in chunks of 256."""
    rng = np.random.default_rng(20241021)
    shapes = []
    n_edges = np.array([0, 1, 255, 256, 257, 8191, 8192, 8193, 16_384, 16_385, 34_816, 65_280, 65_281, 130_561, 10 ** 6])
    p_edges = np.array([1, 63, 64, 65, 49_088, 49_089, 131_008, 131_009, 262_080, 262_081, 10 ** 6])
    for _ in range(3000):
        kind = int(rng.choice([PDM, AOV, CE, GL]))
        n = int(rng.choice(n_edges)) if rng.random() < 0.5 else int(10 ** rng.uniform(0, 6.5))
        P = int(rng.choice(p_edges)) if rng.random() < 0.5 else int(10 ** rng.uniform(0, 6.3))
        if kind == PDM:
            nc = int(rng.integers(1, 6))
            nb = int(rng.integers(1, 190 // nc + 1))
        elif kind == AOV:
            nb, nc = int(rng.integers(1, 191)), 1
        elif kind == CE:
            nc = int(rng.integers(1, 12))
            nb = int(rng.integers(1, 191 // nc))          # (nb + 1) nc <= 191
        else:
            nc = int(rng.integers(1, 20))
            nb = nc * int(rng.integers(1, 190 // nc + 1))
        shapes.append((kind, n, P, nb, nc))
    seen = set()
    for env in ({}, {"PDC_PDM_SPLIT": 0}, {"PDC_PDM_NZ": 7}):
        for (kind, n, P, nb, nc), (plan, work) in zip(shapes, ask(tmp_path, shapes, **env)):
            assert plan["kind"] == kind
            assert plan["scan_lds"] == lds(kind, nb, nc, plan["block"]) <= SCAN_LDS_CAP, (kind, n, P, nb, nc, plan)
            assert plan["finish_lds"] <= FINISH_LDS_CAP
            assert plan["periods_per_wg"] * plan["waves"] == plan["block"]
            assert plan["periods_per_wg"] * plan["workgroups"] >= P > plan["periods_per_wg"] * (plan["workgroups"] - 1)
            assert work == scratch_bytes(plan, kind, nb, nc), (kind, n, P, nb, nc, plan, work)
            if plan["split"]:
                assert (plan["block"], plan["waves"]) == (256, 4) and (n >= 8192 or kind in (CE, GL))
                assert plan["z_len"] % 256 == 0 and plan["n_z"] * plan["z_len"] >= n > (plan["n_z"] - 1) * plan["z_len"]
                assert 1 <= plan["n_stat"] <= 512 and plan["n_stat"] * 1024 >= min(n, 512 * 1024)
                assert plan["n_z"] <= 65_535                    # grid.y
            else:
                assert (plan["n_z"], plan["z_len"], plan["n_stat"], plan["finish_lds"]) == (1, 0, 0, 0)
            if kind in (CE, GL):
                assert plan["block"] == 256 and (plan["z_len"] if plan["split"] else n) <= CELL_SAMPLES
            seen.add((plan["split"], plan["block"], plan["waves"]))
    assert seen == {(0, 256, 4), (0, 256, 2), (0, 256, 1), (0, 64, 1), (1, 256, 4)}


def test_bad_arguments_are_refused_without_a_device():
    from periodicity_amd import _cabi
    for bad in ((3, 100, 10, 5, 2), (5, 100, 10, 5, 2), (0, -1, 10, 5, 2), (0, 100, -1, 5, 2), (0, 100, 10, 0, 2),
                (0, 100, 10, 96, 2), (1, 100, 10, 191, 1), (2, 100, 10, 95, 2), (4, 100, 10, 25, 6), (4, 100, 10, 192, 2)):
        with pytest.raises(ValueError):
            _cabi.phase_shape(*bad)
    assert _cabi.phase_shape("pdm", 100, 0, 5, 2)["block"] == 0           # no periods: nothing is launched
    assert _cabi.phase_shape("aov", 0, 10, 10)["block"] == 256           # no samples: one unsplit launch of NaNs
    assert set(_cabi.phase_last_dispatch()) == set(_cabi.phase_shape(0, 1, 1, 1, 1))
