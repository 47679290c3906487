"""The single-call host entries (numpy in, numpy out) at shapes where the frame around them still does everything - 64
samples, 96 bins or periods, batches of 5 / 64 / 33 samples and of 3 x 64 on one time axis, k = 2, 8 BLS bins, every
optional array once there and once NULL: (a) a host entry returns the bits of its `_dev` twin run on DeviceBuffer copies
of the same arrays, (b) it allocates at most one block per slot, and nothing from the second call on, (c) a call refused
only after its uploads (BGLST with three samples) leaves the device ready for the next one."""
import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import scan_oracle as so
from periodicity_amd import _cabi
from periodicity_amd.spectral import BGLST

pytestmark = pytest.mark.gpu

N, NF, K, SLOT_COUNT = 64, 96, 2, 8
F0, DELTA = 0.004, 0.0021
LENS = (5, 64, 33)
RNG = np.random.default_rng(1664)
T = np.sort(RNG.uniform(0.0, 64.0, N))
DY = RNG.uniform(0.05, 0.2, N)
Y = 1.0 + 0.5 * np.sin(2 * np.pi * T / 7.3) + DY * RNG.standard_normal(N)
PERIODS = np.linspace(1.5, 20.0, NF)
MAG = so.magnitude_bins(Y, 5).astype(np.float64)
M = so.stringlength_scale(Y)
SPECTRA = RNG.uniform(0.0, 1.0, (3, NF))
# the ragged batch: three curves of their own, concatenated; the shared one: three value rows on T
RAGGED_T = np.concatenate([np.sort(RNG.uniform(0.0, 64.0, n)) for n in LENS])
RAGGED_DY = RNG.uniform(0.05, 0.2, RAGGED_T.size)
RAGGED_Y = np.sin(RAGGED_T / 1.7) + RAGGED_DY * RNG.standard_normal(RAGGED_T.size)
RAGGED_OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
SHARED_Y = np.concatenate([Y, Y[::-1], Y * Y])
SHARED_OFF = (np.arange(4) * N).astype(np.int64)
BATCHES = {"ragged": (RAGGED_T, RAGGED_Y, RAGGED_DY, RAGGED_OFF, 0), "shared": (T, SHARED_Y, None, SHARED_OFF, 1)}


def ok(status):
    _cabi.check(status)


class Device:
    """DeviceBuffer copies for a `_dev` call on the NULL stream; `down` waits (a blocking copy) and reads one back."""

    def __init__(self):
        self.bufs = []

    def up(self, a):
        if a is None:
            return None
        self.bufs.append(_cabi.DeviceBuffer.from_array(a))
        return self.bufs[-1].ptr

    def new(self, dtype, count, wanted=True):
        if not wanted:
            return None
        self.bufs.append(_cabi.DeviceBuffer(max(int(count) * np.dtype(dtype).itemsize, 8)))
        self.bufs[-1].dtype, self.bufs[-1].count = dtype, int(count)
        return self.bufs[-1]

    def work(self, nbytes):
        assert nbytes >= 0
        self.bufs.append(_cabi.DeviceBuffer(max(int(nbytes), 8)))
        return self.bufs[-1].ptr, int(nbytes)

    @staticmethod
    def down(buf):
        return None if buf is None else buf.to_array(buf.dtype, buf.count)

    def free(self):
        for b in self.bufs:
            b.free()


def ptr(buf):
    return None if buf is None else buf.ptr


def host_out(dtype, count, wanted=True):
    return np.empty(int(count), dtype=dtype) if wanted else None


P = _cabi._ptr


# ---- every entry as a pair (host call, `_dev` twin): both return the tuple of their outputs (None where not asked for) --
def gls_batch(which, outputs):
    t, y, dy, off, shared = BATCHES[which]
    B, n_total = off.size - 1, int(off[-1])
    want = [name in outputs for name in ("power", "amax", "argmax")]

    def host():
        o = [host_out(np.float64, B * NF, want[0]), host_out(np.float64, B, want[1]), host_out(np.int64, B, want[2])]
        ok(_cabi.lib().pdc_gls_scan_batch(P(t), P(y), P(dy), P(off), B, shared, F0, DELTA, 0, NF, 1, 0, P(o[0]), P(o[1]),
                                          P(o[2]), 0))
        return tuple(o)

    def twin(d):
        o = [d.new(np.float64, B * NF, want[0]), d.new(np.float64, B, want[1]), d.new(np.int64, B, want[2])]
        work, wb = d.work(_cabi.lib().pdc_gls_work_bytes(n_total, B, NF))
        ok(_cabi.lib().pdc_gls_scan_dev(0, None, d.up(t), d.up(y), d.up(dy), d.up(off), n_total, B, shared, F0, DELTA, 0, NF,
                                        1, 0, ptr(o[0]), ptr(o[1]), ptr(o[2]), work, wb))
        return tuple(d.down(b) for b in o)

    return host, twin


def bglst(with_dy):
    dy = DY if with_dy else None
    scalars = BGLST._scalars(T, Y, DY if with_dy else np.ones(N), 1.0, 1.0, 1.0, 0.5 * (T[0] + T[-1]))

    def host():
        out = np.empty(NF)
        ok(_cabi.lib().pdc_bglst_scan(P(T), P(Y), P(dy), N, F0, DELTA, 0, NF, P(scalars), P(out), 0))
        return (out,)

    def twin(d):
        out = d.new(np.float64, NF)
        work, wb = d.work(_cabi.lib().pdc_gls_work_bytes(N, 1, NF))
        ok(_cabi.lib().pdc_bglst_scan_dev(0, None, d.up(T), d.up(Y), d.up(dy), N, F0, DELTA, 0, NF, P(scalars), out.ptr, work,
                                          wb))
        return (d.down(out),)

    return host, twin


def gls_fft(with_dy):
    dy = DY if with_dy else None

    def host():
        out = np.empty(NF)
        ok(_cabi.lib().pdc_gls_scan_fft(P(T), P(Y), P(dy), N, F0, DELTA, NF, 1, 0, P(out), 0))
        return (out,)

    def twin(d):
        out = d.new(np.float64, NF)
        work, wb = d.work(_cabi.lib().pdc_gls_fft_work_bytes(N, NF))
        ok(_cabi.lib().pdc_gls_scan_fft_dev(0, None, d.up(T), d.up(Y), d.up(dy), N, F0, DELTA, NF, 1, 0, out.ptr, work, wb))
        return (d.down(out),)

    return host, twin


def mhgls(with_dy):
    dy = DY if with_dy else None

    def host():
        out = np.empty(NF)
        ok(_cabi.lib().pdc_mhgls_scan(P(T), P(Y), P(dy), N, F0, DELTA, 0, NF, 2, 1, 0, P(out), 0))
        return (out,)

    def twin(d):
        out = d.new(np.float64, NF)
        ok(_cabi.lib().pdc_mhgls_scan_dev(0, None, d.up(T), d.up(Y), d.up(dy), N, F0, DELTA, 0, NF, 2, 1, 0, out.ptr))
        return (d.down(out),)

    return host, twin


def bls(with_dy, optional):
    dy = DY if with_dy else None
    args = (8, 1, 3, 2, 0, 0)   # n_bins, len_min, len_max, min_points, dips_only, slices

    def host():
        o = [np.empty(NF), host_out(np.float64, NF, optional), host_out(np.int32, NF, optional), host_out(np.int32, NF, optional)]
        ok(_cabi.lib().pdc_bls_scan(P(T), P(Y), P(dy), N, P(PERIODS), NF, *args, *[P(a) for a in o], 0))
        return tuple(o)

    def twin(d):
        o = [d.new(np.float64, NF), d.new(np.float64, NF, optional), d.new(np.int32, NF, optional), d.new(np.int32, NF, optional)]
        ok(_cabi.lib().pdc_bls_scan_dev(0, None, d.up(T), d.up(Y), d.up(dy), N, d.up(PERIODS), NF, *args, *[ptr(b) for b in o]))
        return tuple(d.down(b) for b in o)

    return host, twin


def phase(entry, values, params):
    """pdm / aov / cond_entropy / gl: `values` None for Gregory-Loredo, which takes arrival times only."""
    arrays = (T,) if values is None else (T, values)

    def host():
        out = np.empty(NF)
        ok(getattr(_cabi.lib(), f"pdc_{entry}")(*[P(a) for a in arrays], N, P(PERIODS), NF, *params, P(out), 0))
        return (out,)

    def twin(d):
        out = d.new(np.float64, NF)
        ok(getattr(_cabi.lib(), f"pdc_{entry}_dev")(0, None, *[d.up(a) for a in arrays], N, d.up(PERIODS), NF, *params, out.ptr))
        return (d.down(out),)

    return host, twin


def sorted_scan(entry, values, params):
    """stringlength / supersmoother: the twin takes its workspace from the matching `*_work_bytes`."""
    def host():
        out = np.empty(NF)
        ok(getattr(_cabi.lib(), f"pdc_{entry}_scan")(P(T), P(values), N, P(PERIODS), NF, *params, P(out), 0))
        return (out,)

    def twin(d):
        out = d.new(np.float64, NF)
        work, wb = d.work(getattr(_cabi.lib(), f"pdc_{entry}_work_bytes")(N, NF))
        ok(getattr(_cabi.lib(), f"pdc_{entry}_scan_dev")(0, None, d.up(T), d.up(values), N, d.up(PERIODS), NF, *params, out.ptr,
                                                         work, wb))
        return (d.down(out),)

    return host, twin


def highest_peak(outputs):
    want = ["idx" in outputs, "val" in outputs]

    def host():
        o = [host_out(np.int64, 3, want[0]), host_out(np.float64, 3, want[1])]
        ok(_cabi.lib().pdc_highest_peak(P(SPECTRA), 3, NF, P(o[0]), P(o[1]), 0))
        return tuple(o)

    def twin(d):
        o = [d.new(np.int64, 3, want[0]), d.new(np.float64, 3, want[1])]
        ok(_cabi.lib().pdc_highest_peak_dev(0, None, d.up(SPECTRA), 3, NF, ptr(o[0]), ptr(o[1])))
        return tuple(d.down(b) for b in o)

    return host, twin


TABLE = (("count", np.int64, 1), ("idx", np.int64, K), ("height", np.float64, K), ("prom", np.float64, K),
         ("half_lo", np.int64, K), ("half_hi", np.int64, K))


def peaks_topk(by_prominence, outputs):
    def host():
        o = [host_out(dt, 3 * w, name in outputs) for name, dt, w in TABLE]
        ok(_cabi.lib().pdc_peaks_topk(P(SPECTRA), 3, NF, K, by_prominence, *[P(a) for a in o], 0))
        return tuple(o)

    def twin(d):
        o = [d.new(dt, 3 * w, name in outputs) for name, dt, w in TABLE]
        ok(_cabi.lib().pdc_peaks_topk_dev(0, None, d.up(SPECTRA), 3, NF, K, by_prominence, *[ptr(b) for b in o]))
        return tuple(d.down(b) for b in o)

    return host, twin


def gls_batch_then(which, reduce, outputs):
    """pdc_gls_batch_peaks / pdc_gls_batch_highest_peak: the twin is the scan's `_dev` entry, then the reduction's."""
    t, y, dy, off, shared = BATCHES[which]
    B, n_total = off.size - 1, int(off[-1])
    common = (B, shared, F0, DELTA, NF, 1, 0)

    def scan(d):
        power = d.new(np.float64, B * NF)
        work, wb = d.work(_cabi.lib().pdc_gls_work_bytes(n_total, B, NF))
        ok(_cabi.lib().pdc_gls_scan_dev(0, None, d.up(t), d.up(y), d.up(dy), d.up(off), n_total, B, shared, F0, DELTA, 0, NF,
                                        1, 0, power.ptr, None, None, work, wb))
        return power.ptr

    if reduce == "peaks":
        def host():
            o = [host_out(dt, B * w, name in outputs) for name, dt, w in TABLE]
            ok(_cabi.lib().pdc_gls_batch_peaks(P(t), P(y), P(dy), P(off), *common, K, 1, *[P(a) for a in o], 0))
            return tuple(o)

        def twin(d):
            o = [d.new(dt, B * w, name in outputs) for name, dt, w in TABLE]
            ok(_cabi.lib().pdc_peaks_topk_dev(0, None, scan(d), B, NF, K, 1, *[ptr(b) for b in o]))
            return tuple(d.down(b) for b in o)
    else:
        want = ["idx" in outputs, "val" in outputs]

        def host():
            o = [host_out(np.int64, B, want[0]), host_out(np.float64, B, want[1])]
            ok(_cabi.lib().pdc_gls_batch_highest_peak(P(t), P(y), P(dy), P(off), *common, P(o[0]), P(o[1]), 0))
            return tuple(o)

        def twin(d):
            o = [d.new(np.int64, B, want[0]), d.new(np.float64, B, want[1])]
            ok(_cabi.lib().pdc_highest_peak_dev(0, None, scan(d), B, NF, ptr(o[0]), ptr(o[1])))
            return tuple(d.down(b) for b in o)

    return host, twin


ALL_TABLE = tuple(name for name, _, _ in TABLE)
PAIRS = {
    "gls_scan_batch-ragged-dy-all_outputs": gls_batch("ragged", ("power", "amax", "argmax")),
    "gls_scan_batch-shared-no_dy-power_only": gls_batch("shared", ("power",)),
    "gls_scan_batch-ragged-peaks_only": gls_batch("ragged", ("amax", "argmax")),
    "bglst_scan-dy": bglst(True),
    "bglst_scan-no_dy": bglst(False),
    "gls_scan_fft-dy": gls_fft(True),
    "gls_scan_fft-no_dy": gls_fft(False),
    "mhgls_scan-dy": mhgls(True),
    "mhgls_scan-no_dy": mhgls(False),
    "bls_scan-dy-all_outputs": bls(True, True),
    "bls_scan-no_dy-power_only": bls(False, False),
    "pdm_scan": phase("pdm_scan", Y, (5, 2, float(np.var(Y, ddof=1)))),
    "aov_scan": phase("aov_scan", Y, (6,)),
    "cond_entropy_scan": phase("cond_entropy_scan", MAG, (6, 5)),
    "gl_scan-no_values": phase("gl_scan", None, (4, 3)),
    "stringlength_scan": sorted_scan("stringlength", M, ()),
    "supersmoother_scan": sorted_scan("supersmoother", Y, (0.0,)),
    "highest_peak-both": highest_peak(("idx", "val")),
    "highest_peak-idx_only": highest_peak(("idx",)),
    "peaks_topk-height-all_outputs": peaks_topk(0, ALL_TABLE),
    "peaks_topk-prominence-idx_prom_only": peaks_topk(1, ("idx", "prom")),
    "gls_batch_peaks-ragged-dy-all_outputs": gls_batch_then("ragged", "peaks", ALL_TABLE),
    "gls_batch_peaks-shared-no_dy-count_idx_only": gls_batch_then("shared", "peaks", ("count", "idx")),
    "gls_batch_highest_peak-ragged-dy-both": gls_batch_then("ragged", "highest", ("idx", "val")),
    "gls_batch_highest_peak-shared-no_dy-val_only": gls_batch_then("shared", "highest", ("val",)),
}


@pytest.mark.parametrize("name", list(PAIRS))
def test_host_entry_returns_the_bits_of_its_dev_twin(name):
    host, twin = PAIRS[name]
    d = Device()
    try:
        got, want = host(), twin(d)
    finally:
        d.free()
    assert len(got) == len(want) and any(g is not None for g in got)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), i
        if g is not None:
            assert np.any(np.isfinite(w)) and np.array_equal(g, w, equal_nan=True), (name, i)


def trig_sums_host():
    S, Cc = np.empty(NF), np.empty(NF)
    ok(_cabi.lib().pdc_trig_sums(P(T), P(Y), N, F0, DELTA, NF, P(S), P(Cc), 0))
    return S, Cc


def trig_sums_fft_host(h=Y, df=DELTA, fmin=F0):
    S, Cc = np.empty(NF), np.empty(NF)
    ok(_cabi.lib().pdc_trig_sums_fft(P(T), P(h), N, df, NF, fmin, P(S), P(Cc), 0))
    return S, Cc


def fft_batch_host(which="ragged", outputs=("power", "amax", "argmax")):
    t, y, dy, off, shared = BATCHES[which]
    B = off.size - 1
    o = [host_out(np.float64, B * NF, "power" in outputs), host_out(np.float64, B, "amax" in outputs),
         host_out(np.int64, B, "argmax" in outputs)]
    ok(_cabi.lib().pdc_gls_scan_fft_batch(P(t), P(y), P(dy), P(off), B, shared, F0, DELTA, NF, 1, 0, *[P(a) for a in o], 0))
    return tuple(o)


def assert_tier_f(got, ref):
    """|got - ref| <= 1e-9 |ref| + 1e-12 max|ref|: DESIGN.md section 1 (Tier F) and tests/test_gls_fft_gpu.py::
    test_batched_fft_path_equals_single_calls, whose pair this is."""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin) and np.any(fin)
    err, bound = np.abs(got[fin] - ref[fin]), 1e-9 * np.abs(ref[fin]) + 1e-12 * np.max(np.abs(ref[fin]))
    assert np.all(err <= bound), float(np.max(err / bound))


def test_trig_sums_has_no_twin_and_equals_the_exact_sums():
    """No `_dev` form exists: the long-double sums, at the bound tests/test_gls_gpu.py puts on this entry (1e-9 n)."""
    S, Cc = trig_sums_host()
    Se, Ce = co.trig_sums_exact(T, Y, F0 + DELTA * np.arange(NF))
    assert np.max(np.abs(S - Se)) < 1e-9 * N and np.max(np.abs(Cc - Ce)) < 1e-9 * N


def test_trig_sums_fft_has_no_twin_and_rebuilds_the_fft_scan():
    """The three sums the reference's periodogram takes, through its own epilogue, against pdc_gls_scan_fft."""
    w, yc, _ = so.gls_weights(Y, DY, True)
    Sh, Ch = trig_sums_fft_host(w * yc)
    S2, C2 = trig_sums_fft_host(w, 2 * DELTA, 2 * F0)
    S, Cc = trig_sums_fft_host(w)
    rebuilt = so.gls_epilogue(Sh, Ch, S2, C2, S, Cc, np.dot(w, yc ** 2), True, False, DY)
    assert_tier_f(rebuilt, gls_fft(True)[0]()[0])


@pytest.mark.parametrize("which,outputs", [("ragged", ("power", "amax", "argmax")), ("shared", ("power",)),
                                           ("ragged", ("amax", "argmax"))])
def test_fft_batch_has_no_twin_and_equals_the_single_calls(which, outputs):
    t, y, dy, off, _ = BATCHES[which]
    power, amax, argmax = fft_batch_host(which, outputs)
    for b in range(off.size - 1):
        a, e = int(off[b]), int(off[b + 1])
        tb = t if which == "shared" else t[a:e]
        yb = np.ascontiguousarray(y[a:e])
        dyb = None if dy is None else np.ascontiguousarray(dy[a:e])
        single = np.empty(NF)
        ok(_cabi.lib().pdc_gls_scan_fft(P(tb), P(yb), P(dyb), e - a, F0, DELTA, NF, 1, 0, P(single), 0))
        if power is not None:
            assert_tier_f(power[b * NF:(b + 1) * NF], single)
        if amax is not None:   # the row's maximum, where the single call has its own to the same bound
            at = int(argmax[b])
            assert abs(amax[b] - single[at]) <= 1e-9 * abs(single[at]) + 1e-12 * np.nanmax(np.abs(single))
            assert single[at] >= np.nanmax(single) * (1 - 2e-9) - 2e-12 * np.nanmax(np.abs(single))
            if power is not None:
                row = power[b * NF:(b + 1) * NF]
                assert at == np.nanargmax(row) and amax[b] == np.nanmax(row)


HOST_CALLS = dict({name: pair[0] for name, pair in PAIRS.items()}, trig_sums=trig_sums_host, trig_sums_fft=trig_sums_fft_host,
                  gls_scan_fft_batch=fft_batch_host)


@pytest.mark.parametrize("name", list(HOST_CALLS))
def test_one_block_per_slot_at_most_then_nothing(name):
    call = HOST_CALLS[name]
    ok(_cabi.lib().pdc_release())                 # (the slots of whatever ran before: this call is a first one)
    before = _cabi.alloc_counts()
    call()
    first = _cabi.alloc_counts()
    assert 1 <= first[0] - before[0] <= SLOT_COUNT and first[1] == before[1]
    for _ in range(3):
        call()
    assert _cabi.alloc_counts() == first


def test_a_call_refused_after_its_uploads_leaves_the_device_ready():
    """pdc_bglst_scan learns that three samples are too few only in pdc_bglst_scan_dev, with t, y and dy already in the
    stream: PDC_ERR_INVALID with its text - an argument check, nothing faults -, and the next call is right."""
    host, twin = PAIRS["bglst_scan-dy"]
    scalars = BGLST._scalars(T[:3], Y[:3], DY[:3], 1.0, 1.0, 1.0, T[1])
    out = np.full(NF, -7.0)
    t3, y3, dy3 = T[:3].copy(), Y[:3].copy(), DY[:3].copy()
    status = _cabi.lib().pdc_bglst_scan(P(t3), P(y3), P(dy3), 3, F0, DELTA, 0, NF, P(scalars), P(out), 0)
    assert status == -1 and "at least four samples" in _cabi.lib().pdc_last_error().decode()
    assert np.all(out == -7.0)
    d = Device()
    try:
        got, want = host(), twin(d)
    finally:
        d.free()
    assert np.all(np.isfinite(want[0])) and np.array_equal(got[0], want[0])
