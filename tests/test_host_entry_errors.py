"""The single-call host entries (numpy in, numpy out) refuse a bad call before they look for a device: every class of
argument each of them rejects, with its status and the whole ``pdc_last_error()`` text, straight through ``_cabi.lib()``.
Without a GPU one VALID call per entry then fails loudly with ``PDC_ERR_NODEVICE`` - never an answer from the CPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from periodicity_amd import _cabi

INVALID, NODEVICE = -1, -2

T = np.array([0.0, 1.1, 2.3, 3.2, 4.7, 5.1, 6.4, 7.9])
Y = np.array([1.0, 0.4, -0.3, 0.8, 1.2, -0.9, 0.1, 0.6])
DY = np.full(8, 0.1)
MAG = np.array([0.0, 1.0, 2.0, 4.0, 3.0, 1.0, 0.0, 2.0])
PERIODS = np.array([2.0, 3.0, 4.5, 6.0])
SCALARS = np.array([800.0, 5.0, 1.0, 2.0, 3.0, 0.5, 0.0, 0.125, 1.0, 1.0, 1.0, 0.0])
OFFSETS = np.array([0, 5, 8], dtype=np.int64)
DECREASING = np.array([0, 5, 3], dtype=np.int64)
NOT_FROM_ZERO = np.array([1, 5, 8], dtype=np.int64)
POWER = np.linspace(0.0, 1.0, 8)          # one spectrum of 8 bins, or two of 4
F64, F64B, I64, I64B, I64C = np.empty(64), np.empty(64), np.empty(64, np.int64), np.empty(64, np.int64), np.empty(64, np.int64)
I32, I32B = np.empty(64, np.int32), np.empty(64, np.int32)

# entry -> its arguments in the ABI's order, with the values of a call the library accepts
GLS_IN = dict(t=T, y=Y, dy=DY, offsets=OFFSETS, n_curves=2, shared_t=0)
TABLE = dict(count=I64, idx=I64B, height=F64, prom=F64B, half_lo=I64C, half_hi=None)
ENTRIES = {
    "pdc_gls_scan": dict(t=T, y=Y, dy=DY, n=8, f0=0.01, delta=0.01, j_begin=0, nf=4, fit_mean=1, psd=0, power=F64, device=0),
    "pdc_gls_scan_batch": dict(**GLS_IN, f0=0.01, delta=0.01, j_begin=0, nf=4, fit_mean=1, psd=0, power=F64, amax=F64B,
                               argmax=I64, device=0),
    "pdc_bglst_scan": dict(t=T, y=Y, dy=DY, n=8, f0=0.01, delta=0.01, j_begin=0, nf=4, scalars=SCALARS, loglik=F64, device=0),
    "pdc_trig_sums": dict(t=T, w=Y, n=8, f0=0.01, delta=0.01, nf=4, S=F64, C=F64B, device=0),
    "pdc_gls_scan_fft": dict(t=T, y=Y, dy=DY, n=8, fmin=0.01, df=0.01, nf=4, fit_mean=1, psd=0, power=F64, device=0),
    "pdc_gls_scan_fft_batch": dict(**GLS_IN, fmin=0.01, df=0.01, nf=4, fit_mean=1, psd=0, power=F64, amax=F64B, argmax=I64,
                                   device=0),
    "pdc_trig_sums_fft": dict(t=T, h=Y, n=8, df=0.01, nf=4, fmin=0.01, S=F64, C=F64B, device=0),
    "pdc_mhgls_scan": dict(t=T, y=Y, dy=DY, n=8, f0=0.01, delta=0.01, j_begin=0, nf=4, nterms=1, fit_mean=1, psd=0, power=F64,
                           device=0),
    "pdc_bls_scan": dict(t=T, y=Y, dy=DY, n=8, periods=PERIODS, n_periods=4, n_bins=4, len_min=1, len_max=2, min_points=1,
                         dips_only=0, slices=0, power=F64, depth=F64B, start_bin=I32, box_bins=I32B, device=0),
    "pdc_pdm_scan": dict(t=T, x=Y, n=8, periods=PERIODS, n_periods=4, nb=5, nc=2, sigma=1.0, out=F64, device=0),
    "pdc_aov_scan": dict(t=T, x=Y, n=8, periods=PERIODS, n_periods=4, n_bins=4, out=F64, device=0),
    "pdc_cond_entropy_scan": dict(t=T, x=MAG, n=8, periods=PERIODS, n_periods=4, n_phase=4, n_mag=5, out=F64, device=0),
    "pdc_gl_scan": dict(t=T, n=8, periods=PERIODS, n_periods=4, m=3, n_offsets=2, out=F64, device=0),
    "pdc_stringlength_scan": dict(t=T, v=Y, n=8, periods=PERIODS, n_periods=4, out=F64, device=0),
    "pdc_supersmoother_scan": dict(t=T, v=Y, n=8, periods=PERIODS, n_periods=4, alpha=0.0, out=F64, device=0),
    "pdc_highest_peak": dict(power=POWER, n_curves=2, nf=4, idx=I64, val=F64, device=0),
    "pdc_peaks_topk": dict(power=POWER, n_curves=2, nf=4, k=2, by_prominence=0, **TABLE, device=0),
    "pdc_gls_batch_peaks": dict(**GLS_IN, f0=0.01, delta=0.01, nf=4, fit_mean=1, psd=0, k=2, by_prominence=0, **TABLE,
                                device=0),
    "pdc_gls_batch_highest_peak": dict(**GLS_IN, f0=0.01, delta=0.01, nf=4, fit_mean=1, psd=0, idx=I64, val=F64, device=0),
}


def call(entry, **changed):
    args = dict(ENTRIES[entry])
    assert set(changed) <= set(args), (entry, changed)
    args.update(changed)
    lib = _cabi.lib()
    status = getattr(lib, entry)(*[_cabi._ptr(v) if isinstance(v, np.ndarray) else v for v in args.values()])
    return status, lib.pdc_last_error().decode()


NO_OUTPUT3 = dict(power=None, amax=None, argmax=None)
NO_TABLE = dict(count=None, idx=None, height=None, prom=None, half_lo=None, half_hi=None)
BAD_MAG = np.array([0.0, 1.0, 5.0, 4.0, 3.0, 1.0, 0.0, 2.0])
NEGATIVE_MAG = np.array([0.0, -1.0, 2.0, 4.0, 3.0, 1.0, 0.0, 2.0])


def batch_cases(entry, what):
    """The three ways a GLS batch's offsets are wrong; `what` starts the messages."""
    return [(entry, dict(offsets=DECREASING), f"{what}: offsets must be non-decreasing"),
            (entry, dict(shared_t=1), f"{what}: with a shared time axis every curve must have the same length"),
            (entry, dict(offsets=NOT_FROM_ZERO), f"{what}: offsets[0] must be 0")]


def phase_cases(entry, values):
    return [(entry, dict(t=None), "phase scan: NULL argument"), (entry, {values: None}, "phase scan: NULL argument"),
            (entry, dict(periods=None), "phase scan: NULL argument"), (entry, dict(out=None), "phase scan: NULL argument"),
            (entry, dict(n=-1), "phase scan: negative size"), (entry, dict(n_periods=-1), "phase scan: negative size")]


CASES = [
    ("pdc_gls_scan", dict(n=-1), "gls: negative sample count"),
    ("pdc_gls_scan", dict(power=None), "gls: power_out is NULL"),
    ("pdc_gls_scan", dict(t=None), "gls: t, y and offsets must not be NULL"),
    ("pdc_gls_scan", dict(nf=-1), "gls: negative size"),
    ("pdc_gls_scan_batch", dict(t=None), "gls: t, y and offsets must not be NULL"),
    ("pdc_gls_scan_batch", dict(y=None), "gls: t, y and offsets must not be NULL"),
    ("pdc_gls_scan_batch", dict(offsets=None), "gls: t, y and offsets must not be NULL"),
    ("pdc_gls_scan_batch", dict(n_curves=0), "gls: negative size"),
    ("pdc_gls_scan_batch", dict(nf=-1), "gls: negative size"),
    ("pdc_gls_scan_batch", dict(j_begin=-1), "gls: negative size"),
    ("pdc_gls_scan_batch", NO_OUTPUT3, "gls: no output requested"),
    *batch_cases("pdc_gls_scan_batch", "gls"),
    ("pdc_bglst_scan", dict(t=None), "bglst: NULL argument"),
    ("pdc_bglst_scan", dict(scalars=None), "bglst: NULL argument"),
    ("pdc_bglst_scan", dict(loglik=None), "bglst: NULL argument"),
    ("pdc_bglst_scan", dict(n=-1), "bglst: negative size"),
    ("pdc_bglst_scan", dict(nf=-1), "bglst: negative size"),
    ("pdc_trig_sums", dict(w=None), "trig_sums: NULL argument"),
    ("pdc_trig_sums", dict(C=None), "trig_sums: NULL argument"),
    ("pdc_trig_sums", dict(n=-1), "trig_sums: negative size"),
    ("pdc_trig_sums", dict(nf=-1), "trig_sums: negative size"),
    ("pdc_gls_scan_fft", dict(y=None), "gls_fft: NULL argument"),
    ("pdc_gls_scan_fft", dict(power=None), "gls_fft: NULL argument"),
    ("pdc_gls_scan_fft", dict(n=-1), "gls_fft: negative size"),
    ("pdc_gls_scan_fft", dict(nf=-1), "gls_fft: negative size"),
    ("pdc_gls_scan_fft_batch", dict(t=None), "gls_fft_batch: t, y and offsets must not be NULL"),
    ("pdc_gls_scan_fft_batch", dict(offsets=None), "gls_fft_batch: t, y and offsets must not be NULL"),
    ("pdc_gls_scan_fft_batch", dict(n_curves=0), "gls_fft_batch: bad size"),
    ("pdc_gls_scan_fft_batch", dict(nf=-1), "gls_fft_batch: bad size"),
    ("pdc_gls_scan_fft_batch", NO_OUTPUT3, "gls_fft_batch: no output requested"),
    *batch_cases("pdc_gls_scan_fft_batch", "gls_fft_batch"),
    ("pdc_trig_sums_fft", dict(h=None), "trig_sums_fft: NULL argument"),
    ("pdc_trig_sums_fft", dict(S=None), "trig_sums_fft: NULL argument"),
    ("pdc_trig_sums_fft", dict(n=-1), "trig_sums_fft: need at least one sample and one frequency"),
    ("pdc_trig_sums_fft", dict(n=0), "trig_sums_fft: need at least one sample and one frequency"),
    ("pdc_trig_sums_fft", dict(nf=0), "trig_sums_fft: need at least one sample and one frequency"),
    ("pdc_mhgls_scan", dict(t=None), "mhgls: NULL argument"),
    ("pdc_mhgls_scan", dict(power=None), "mhgls: NULL argument"),
    ("pdc_mhgls_scan", dict(n=-1), "mhgls: negative size"),
    ("pdc_mhgls_scan", dict(nf=-1), "mhgls: negative size"),
    ("pdc_mhgls_scan", dict(j_begin=-1), "mhgls: negative size"),
    ("pdc_bls_scan", dict(n=-1), "bls: negative size"),
    ("pdc_bls_scan", dict(n_periods=-1), "bls: negative size"),
    ("pdc_bls_scan", dict(y=None), "bls: NULL argument"),
    ("pdc_bls_scan", dict(periods=None), "bls: NULL argument"),
    ("pdc_bls_scan", dict(power=None), "bls: NULL argument"),
    *phase_cases("pdc_pdm_scan", "x"),
    *phase_cases("pdc_aov_scan", "x"),
    *phase_cases("pdc_cond_entropy_scan", "x"),
    ("pdc_cond_entropy_scan", dict(x=BAD_MAG), "cond_entropy: mag_bin[2] = 5 is not a bin index in 0 .. 4"),
    ("pdc_cond_entropy_scan", dict(x=NEGATIVE_MAG), "cond_entropy: mag_bin[1] = -1 is not a bin index in 0 .. 4"),
    ("pdc_gl_scan", dict(t=None), "phase scan: NULL argument"),
    ("pdc_gl_scan", dict(out=None), "phase scan: NULL argument"),
    ("pdc_gl_scan", dict(n=-1), "phase scan: negative size"),
    ("pdc_gl_scan", dict(m=20, n_offsets=10), "gregory_loredo: m * n_offsets must be 1..190"),
    ("pdc_gl_scan", dict(m=191, n_offsets=1), "gregory_loredo: m * n_offsets must be 1..190"),
    ("pdc_gl_scan", dict(m=0), "gregory_loredo: m * n_offsets must be 1..190"),
    ("pdc_stringlength_scan", dict(v=None), "stringlength: NULL argument"),
    ("pdc_stringlength_scan", dict(out=None), "stringlength: NULL argument"),
    ("pdc_stringlength_scan", dict(n=-1), "stringlength: negative size"),
    ("pdc_stringlength_scan", dict(n_periods=-1), "stringlength: negative size"),
    ("pdc_supersmoother_scan", dict(t=None), "supersmoother: NULL argument"),
    ("pdc_supersmoother_scan", dict(periods=None), "supersmoother: NULL argument"),
    ("pdc_supersmoother_scan", dict(n=-1), "supersmoother: negative size"),
    ("pdc_highest_peak", dict(power=None), "highest_peak: power is NULL"),
    ("pdc_highest_peak", dict(idx=None, val=None), "highest_peak: no output requested"),
    ("pdc_highest_peak", dict(n_curves=-1), "highest_peak: negative size"),
    ("pdc_highest_peak", dict(nf=-1), "highest_peak: negative size"),
    ("pdc_peaks_topk", dict(power=None), "peaks_topk: power is NULL"),
    ("pdc_peaks_topk", dict(k=0), "peaks_topk: k must be 1..1024"),
    ("pdc_peaks_topk", dict(k=1025), "peaks_topk: k must be 1..1024"),
    ("pdc_peaks_topk", dict(nf=-1), "peaks_topk: negative size"),
    ("pdc_peaks_topk", NO_TABLE, "peaks_topk: no output requested"),
    ("pdc_gls_batch_peaks", dict(y=None), "gls_batch_peaks: NULL argument"),
    ("pdc_gls_batch_peaks", dict(offsets=None), "gls_batch_peaks: NULL argument"),
    ("pdc_gls_batch_peaks", dict(n_curves=0), "gls_batch_peaks: bad size"),
    ("pdc_gls_batch_peaks", dict(nf=-1), "gls_batch_peaks: bad size"),
    ("pdc_gls_batch_peaks", dict(k=0), "gls_batch_peaks: k must be 1..1024"),
    ("pdc_gls_batch_peaks", dict(k=1025), "gls_batch_peaks: k must be 1..1024"),
    *batch_cases("pdc_gls_batch_peaks", "gls"),
    ("pdc_gls_batch_highest_peak", dict(t=None), "gls_batch_highest_peak: NULL argument"),
    ("pdc_gls_batch_highest_peak", dict(idx=None, val=None), "gls_batch_highest_peak: NULL argument"),
    ("pdc_gls_batch_highest_peak", dict(n_curves=0), "gls_batch_highest_peak: bad size"),
    ("pdc_gls_batch_highest_peak", dict(nf=-1), "gls_batch_highest_peak: bad size"),
    *batch_cases("pdc_gls_batch_highest_peak", "gls"),
]


@pytest.mark.parametrize("entry,changed,text", CASES, ids=[f"{e}-{i}" for i, (e, _, _) in enumerate(CASES)])
def test_a_bad_call_is_refused_with_its_text_before_any_device(entry, changed, text):
    # device 99 exists nowhere: a call that reached the device table would say so (or PDC_ERR_NODEVICE) instead
    status, message = call(entry, device=99, **changed)
    assert (status, message) == (INVALID, text)


def test_a_batch_wrong_in_two_ways_keeps_the_text_of_its_entry():
    """The direct batch looks at every pair of offsets before offsets[0], the FFT batch at offsets[0] first."""
    twice = np.array([1, 5, 3], dtype=np.int64)
    assert call("pdc_gls_scan_batch", offsets=twice, device=99) == (INVALID, "gls: offsets must be non-decreasing")
    assert call("pdc_gls_scan_fft_batch", offsets=twice, device=99) == (INVALID, "gls_fft_batch: offsets[0] must be 0")


def test_every_case_names_an_entry_and_every_entry_has_cases():
    assert {e for e, _, _ in CASES} == set(ENTRIES)


def test_without_a_device_a_valid_call_fails_loudly():
    if _cabi.device_count() != 0:
        return   # (a device is visible: tests/test_host_entries_gpu.py runs the valid calls)
    for entry in ENTRIES:
        status, message = call(entry)
        assert status == NODEVICE and message, entry


HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_offsets_check_alone_under_the_host_sanitizers(tmp_path):
    """The one piece of the host frame that makes no HIP call, as a program of its own (tests/csrc/) built for the host
    with AddressSanitizer and UBSan: the offsets above, good and bad, and the sizes a good one gives."""
    exe = tmp_path / "gls_batch_offsets_check"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "gls_batch_offsets_check.cpp")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-std=c++17", "-g", src, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
