"""ctypes binding of ``libperiodicity_hip.so`` (``include/periodicity_hip.h``).

This is the only place the Python host code touches native code.  There is **no CPU fallback**:
if the shared library is missing, or no gfx950 device is visible, every scan raises — loudly.
"""
import ctypes as C
import os
import threading

import numpy as np

_LIB_NAME = "libperiodicity_hip.so"
_lib = None
_lock = threading.Lock()

c_double_p = C.POINTER(C.c_double)
c_int64_p = C.POINTER(C.c_int64)

STATUS_EXC = {-1: ValueError, -2: RuntimeError, -3: RuntimeError, -4: RuntimeError,
              -5: MemoryError}

# name -> (restype, argtypes); kept in the order of include/periodicity_hip.h
_VP, _I, _L, _D = C.c_void_p, C.c_int, C.c_int64, C.c_double
PROTOTYPES = {
    "pdc_last_error": (C.c_char_p, []),
    "pdc_version": (_I, []),
    "pdc_device_count": (_I, [C.POINTER(_I)]),
    "pdc_device_info": (_I, [_I, C.c_char_p, _I, C.POINTER(_I), c_int64_p, C.POINTER(_I)]),
    "pdc_release": (_I, []),
    "pdc_alloc_counts": (_I, [c_int64_p, c_int64_p]),
    "pdc_malloc": (_I, [_I, _L, C.POINTER(_VP)]),
    "pdc_free": (_I, [_I, _VP]),
    "pdc_memcpy_h2d": (_I, [_I, _VP, _VP, _L]),
    "pdc_memcpy_d2h": (_I, [_I, _VP, _VP, _L]),
    "pdc_memset": (_I, [_I, _VP, _I, _L]),
    "pdc_stream_create": (_I, [_I, C.POINTER(_VP)]),
    "pdc_stream_destroy": (_I, [_I, _VP]),
    "pdc_stream_sync": (_I, [_I, _VP]),
    "pdc_device_sync": (_I, [_I]),
    "pdc_test_scratch_pin": (_I, [_I, _VP, _L, C.POINTER(_VP)]),
    "pdc_test_scratch_unpin": (_I, [_I, _VP]),
    "pdc_event_create": (_I, [_I, C.POINTER(_VP)]),
    "pdc_event_destroy": (_I, [_I, _VP]),
    "pdc_event_record": (_I, [_I, _VP, _VP]),
    "pdc_event_elapsed_ms": (_I, [_I, _VP, _VP, C.POINTER(C.c_float)]),
    "pdc_clock_probe": (_I, [_I, _VP, _I, C.POINTER(C.c_float), C.POINTER(_D), C.POINTER(_D)]),
    "pdc_bglst_scan": (_I, [_VP, _VP, _VP, _L, _D, _D, _L, _L, _VP, _VP, _I]),
    "pdc_bglst_scan_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _D, _D, _L, _L, _VP, _VP, _VP, _L]),
    "pdc_mhgls_scan": (_I, [_VP, _VP, _VP, _L, _D, _D, _L, _L, _I, _I, _I, _VP, _I]),
    "pdc_mhgls_scan_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _D, _D, _L, _L, _I, _I, _I, _VP]),
    "pdc_mbgls_scan": (_I, [_VP, _VP, _VP, _VP, _L, _I, _D, _D, _L, _L, _I, _I, _I, _VP, _I]),
    "pdc_mbgls_scan_dev": (_I, [_I, _VP, _VP, _VP, _VP, _VP, _L, _I, _D, _D, _L, _L, _I, _I, _I, _VP]),
    "pdc_mbgls_tile_bins": (_I, [_I]),
    "pdc_htest_scan": (_I, [_VP, _VP, _L, _D, _D, _L, _L, _I, _I, _VP, _VP, _VP, _I]),
    "pdc_htest_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _D, _D, _L, _L, _I, _I, _VP, _VP, _VP]),
    "pdc_htest_tile_bins": (_L, [_I]),
    "pdc_htest_last_dispatch": (_I, [C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "pdc_htest_fdot_scan": (_I, [_VP, _VP, _L, _D, _D, _L, _L, _VP, _L, _D, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_htest_fdot_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _D, _D, _L, _L, _VP, _L, _D, _I, _I, _I,
                                     _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pdc_htest_fdot_last_dispatch": (_I, [C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), c_int64_p]),
    "pdc_htest_fdot_work_bytes": (_L, [_L, _L, _L, _I, _I, _I]),
    "pdc_wwz_scan": (_I, [_VP, _VP, _VP, _L, _D, _D, _L, _VP, _L, _D, _D, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_wwz_scan_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _D, _D, _L, _VP, _L, _D, _D,
                              _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pdc_wwz_tile_bins": (_L, []),
    "pdc_wwz_work_bytes": (_L, [_L, _L, _L]),
    "pdc_wwz_last_dispatch": (_I, [C.POINTER(_I), C.POINTER(_I), c_int64_p]),
    "pdc_wps_scan": (_I, [_VP, _VP, _L, _VP, _VP, _L, _VP, _D, _D, _D, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_wps_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _VP, _VP, _L, _VP, _D, _D, _D, _D, _D,
                              _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pdc_wps_taps": (_L, [_D, _D, _D, _VP, _VP, _VP, c_int64_p]),
    "pdc_wps_tile": (_L, []),
    "pdc_wps_work_bytes": (_L, [_L, _L]),
    "pdc_wps_last_dispatch": (_I, [c_int64_p, c_int64_p, c_int64_p, c_int64_p, c_int64_p]),
    "pdc_emd_batch": (_I, [_VP, _VP, _L, _L, _L, _I, _D, _D, _D, _I, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_emd_batch_dev": (_I, [_I, _VP, _VP, _VP, _L, _L, _L, _I, _D, _D, _D, _I, _VP, _VP, _VP, _VP, _VP]),
    "pdc_emd_sift": (_I, [_VP, _VP, _L, _I, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_ceemdan_stage_dev": (_I, [_I, _VP, _VP, _VP, _L, _VP, _VP, _L, _I, _I, _VP, _L, _I, _D, _D, _D,
                                   _VP, _VP, _VP, _VP]),
    "pdc_emd_lds_samples": (_L, []),
    "pdc_emd_work_bytes": (_L, [_L, _L, _I]),
    "pdc_emd_last_dispatch": (_I, [c_int64_p, c_int64_p, c_int64_p, c_int64_p]),
    "pdc_kepler_scan": (_I, [_VP, _VP, _VP, _L, _D, _D, _L, _VP, _L, _VP, _L, _I, _I, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_kepler_scan_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _D, _D, _L, _VP, _L, _VP, _L, _I, _I,
                                 _VP, _VP, _VP, _VP, _VP]),
    "pdc_kepler_anomaly": (_I, [_VP, _VP, _L, _VP, _VP, _I]),
    "pdc_kepler_cell_group": (_I, []),
    "pdc_kepler_tile_bins": (_L, []),
    "pdc_kepler_work_bytes": (_L, [_L, _L, _L, _L, _I]),
    "pdc_kepler_last_dispatch": (_I, [C.POINTER(_I), C.POINTER(_I), c_int64_p]),
    "pdc_dcf_scan": (_I, [_VP, _VP, _L, _VP, _VP, _L, _VP, _L, _I, _L, _VP, _VP, _I]),
    "pdc_dcf_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _VP, _VP, _L, _VP, _L, _I, _L, _VP, _VP]),
    "pdc_dcf_work_bytes": (_L, [_L, _L, _L, _L]),
    "pdc_dcf_chunk": (_L, [_L, _L, _L]),
    "pdc_dcf_last_dispatch": (_I, [c_int64_p, c_int64_p]),
    "pdc_gp_loglike": (_I, [_VP, _VP, _VP, _L, _VP, _I, _VP, _VP, _L, _I, _VP, _VP, _VP, _I]),
    "pdc_gp_loglike_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _VP, _I, _VP, _VP, _L, _I, _VP, _VP, _VP]),
    "pdc_gp_scan": (_I, [_VP, _VP, _VP, _L, _VP, _I, _VP, _VP, _L, _I, _L, _L, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_gp_scan_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _VP, _I, _VP, _VP, _L, _I, _L, _L,
                             _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pdc_gp_work_bytes": (_L, [_L, _L, _I, _I]),
    "pdc_gp_max_terms": (_I, []),
    "pdc_gp_chunk_samples": (_I, []),
    "pdc_gp_last_dispatch": (_I, [C.POINTER(_I), C.POINTER(_I), c_int64_p]),
    "pdc_bls_scan": (_I, [_VP, _VP, _VP, _L, _VP, _L, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _I]),
    "pdc_bls_scan_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _VP, _L, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "pdc_bls_scan_ragged": (_I, [_VP, _VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _I,
                                 _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_bls_ragged_peaks": (_I, [_VP, _VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _I,
                                  _VP, _VP, _VP, _VP, _VP, _VP,
                                  _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_bls_ragged_work_bytes": (_L, [_L, _L, _L, _L, _I]),
    "pdc_test_bls_ragged_groups": (_I, [C.POINTER(_L)]),
    "pdc_bls_scan_ragged_dev": (_I, [_I, _VP, _VP, _VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _I,
                                     _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _L, _VP, _L]),
    "pdc_gls_scan": (_I, [_VP, _VP, _VP, _L, _D, _D, _L, _L, _I, _I, _VP, _I]),
    "pdc_gls_scan_batch": (_I, [_VP, _VP, _VP, _VP, _L, _I, _D, _D, _L, _L, _I, _I,
                                _VP, _VP, _VP, _I]),
    "pdc_gls_scan_batch_multi": (_I, [_VP, _VP, _VP, _VP, _L, _I, _D, _D, _L, _I, _I, _VP, _VP, _VP, _VP, _I]),
    "pdc_gls_scan_multi": (_I, [_VP, _VP, _VP, _L, _D, _D, _L, _I, _I, _VP, _VP, _I]),
    "pdc_gls_bootstrap": (_I, [_VP, _VP, _VP, _L, _VP, _L, _D, _D, _L, _I, _I, _I, _VP, _VP, _VP, _I]),
    "pdc_gls_bootstrap_work_bytes": (_L, [_L, _L, _L]),
    "pdc_gls_bootstrap_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _VP, _L, _D, _D, _L, _I, _I, _VP, _VP, _VP, _L]),
    "pdc_gls_plan_create": (_I, [_VP, _I, _L, _L, C.POINTER(_VP)]),
    "pdc_gls_plan_create_loopback": (_I, [_I, _I, _L, _L, C.POINTER(_VP)]),
    "pdc_gls_plan_info": (_I, [_VP, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "pdc_gls_plan_init_error": (_I, [_VP, C.c_char_p, _I]),
    "pdc_gls_plan_upload": (_I, [_VP, _VP, _VP, _VP, _L]),
    "pdc_gls_plan_scan": (_I, [_VP, _D, _D, _L, _I, _I]),
    "pdc_gls_plan_wait": (_I, [_VP]),
    "pdc_gls_plan_download": (_I, [_VP, _VP, _L, _I]),
    "pdc_gls_plan_kernel_ms": (_I, [_VP, C.POINTER(C.c_float)]),
    "pdc_gls_plan_slot_ms": (_I, [_VP, C.POINTER(C.c_float), _I]),
    "pdc_gls_plan_destroy": (_I, [_VP]),
    "pdc_trig_sums": (_I, [_VP, _VP, _L, _D, _D, _L, _VP, _VP, _I]),
    "pdc_gls_work_bytes": (_L, [_L, _L, _L]),
    "pdc_gls_scan_dev": (_I, [_I, _VP, _VP, _VP, _VP, _VP, _L, _L, _I, _D, _D, _L, _L, _I, _I,
                              _VP, _VP, _VP, _VP, _L]),
    "pdc_test_gls_last_dispatch": (_I, [c_int64_p]),
    "pdc_test_gls_last_pair": (_I, [c_int64_p]),
    "pdc_gls_fft_work_bytes": (_L, [_L, _L]),
    "pdc_gls_scan_fft": (_I, [_VP, _VP, _VP, _L, _D, _D, _L, _I, _I, _VP, _I]),
    "pdc_gls_scan_fft_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _D, _D, _L, _I, _I, _VP, _VP, _L]),
    "pdc_trig_sums_fft": (_I, [_VP, _VP, _L, _D, _L, _D, _VP, _VP, _I]),
    "pdc_gls_scan_fft_batch": (_I, [_VP, _VP, _VP, _VP, _L, _I, _D, _D, _L, _I, _I, _VP, _VP, _VP, _I]),
    "pdc_highest_peak": (_I, [_VP, _L, _L, _VP, _VP, _I]),
    "pdc_highest_peak_dev": (_I, [_I, _VP, _VP, _L, _L, _VP, _VP]),
    "pdc_gls_batch_highest_peak": (_I, [_VP, _VP, _VP, _VP, _L, _I, _D, _D, _L, _I, _I, _VP, _VP, _I]),
    "pdc_peaks_topk": (_I, [_VP, _L, _L, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_peaks_topk_dev": (_I, [_I, _VP, _VP, _L, _L, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pdc_gls_batch_peaks": (_I, [_VP, _VP, _VP, _VP, _L, _I, _D, _D, _L, _I, _I, _I, _I,
                                 _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_gls_scan_ragged": (_I, [_VP, _VP, _VP, _VP, _L, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _I]),
    "pdc_gls_ragged_peaks": (_I, [_VP, _VP, _VP, _VP, _L, _VP, _VP, _VP, _I, _I, _I, _I,
                                  _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_gls_ragged_work_bytes": (_L, [_L, _L, _L, _L, _I]),
    "pdc_gls_scan_ragged_dev": (_I, [_I, _VP, _VP, _VP, _VP, _VP, _L, _VP, _VP, _VP, _I, _I,
                                     _VP, _VP, _L, _VP, _VP, _VP, _L]),
    "pdc_phase_scan_ragged": (_I, [_I, _VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _I]),
    "pdc_phase_ragged_peaks": (_I, [_I, _VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I,
                                    _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_phase_ragged_work_bytes": (_L, [_L, _L, _L, _I]),
    "pdc_test_phase_ragged_groups": (_I, [C.POINTER(_L)]),
    "pdc_phase_scan_ragged_dev": (_I, [_I, _I, _VP, _VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I,
                                       _VP, _VP, _L, _VP, _L]),
    "pdc_stringlength_scan_ragged": (_I, [_VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "pdc_stringlength_ragged_peaks": (_I, [_VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP,
                                           _VP, _VP, _VP, _I]),
    "pdc_stringlength_ragged_work_bytes": (_L, [_VP, _VP, _L]),
    "pdc_test_sl_ragged_stats": (_I, [C.POINTER(_L), C.POINTER(_L), C.POINTER(_L)]),
    "pdc_stringlength_scan_ragged_dev": (_I, [_I, _VP, _VP, _VP, _VP, _L, _VP, _VP, _VP, _VP, _VP, _VP, _L, _VP,
                                              _L]),
    "pdc_pdm_scan": (_I, [_VP, _VP, _L, _VP, _L, _I, _I, _D, _VP, _I]),
    "pdc_pdm_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _VP, _L, _I, _I, _D, _VP]),
    "pdc_aov_scan": (_I, [_VP, _VP, _L, _VP, _L, _I, _VP, _I]),
    "pdc_aov_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _VP, _L, _I, _VP]),
    "pdc_cond_entropy_scan": (_I, [_VP, _VP, _L, _VP, _L, _I, _I, _VP, _I]),
    "pdc_cond_entropy_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _VP, _L, _I, _I, _VP]),
    "pdc_stringlength_scan": (_I, [_VP, _VP, _L, _VP, _L, _VP, _I]),
    "pdc_stringlength_work_bytes": (_L, [_L, _L]),
    "pdc_stringlength_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _VP, _L, _VP, _VP, _L]),
    "pdc_gl_scan": (_I, [_VP, _L, _VP, _L, _I, _I, _VP, _I]),
    "pdc_gl_scan_dev": (_I, [_I, _VP, _VP, _L, _VP, _L, _I, _I, _VP]),
    "pdc_phase_work_bytes": (_L, [_I, _L, _L, _I, _I]),
    "pdc_phase_scan_dev": (_I, [_I, _I, _VP, _VP, _VP, _L, _VP, _L, _I, _I, _D, _VP, _VP, _L]),
    "pdc_test_phase_shape": (_I, [_I, _L, _L, _I, _I, c_int64_p]),
    "pdc_test_phase_last_dispatch": (_I, [c_int64_p]),
    "pdc_pdm_scan_multi": (_I, [_VP, _VP, _L, _VP, _L, _I, _I, _D, _VP, _VP, _I]),
    "pdc_aov_scan_multi": (_I, [_VP, _VP, _L, _VP, _L, _I, _VP, _VP, _I]),
    "pdc_cond_entropy_scan_multi": (_I, [_VP, _VP, _L, _VP, _L, _I, _I, _VP, _VP, _I]),
    "pdc_gl_scan_multi": (_I, [_VP, _L, _VP, _L, _I, _I, _VP, _VP, _I]),
    "pdc_phase_plan_create": (_I, [_VP, _I, _L, _L, C.POINTER(_VP)]),
    "pdc_phase_plan_upload": (_I, [_VP, _VP, _VP, _L]),
    "pdc_phase_plan_scan": (_I, [_VP, _I, _VP, _L, _I, _I, _D]),
    "pdc_phase_plan_wait": (_I, [_VP]),
    "pdc_phase_plan_download": (_I, [_VP, _VP, _L]),
    "pdc_phase_plan_kernel_ms": (_I, [_VP, C.POINTER(C.c_float)]),
    "pdc_phase_plan_destroy": (_I, [_VP]),
    "pdc_stringlength_scan_multi": (_I, [_VP, _VP, _L, _VP, _L, _VP, _VP, _I]),
    "pdc_supersmoother_scan": (_I, [_VP, _VP, _L, _VP, _L, _D, _VP, _I]),
    "pdc_supersmoother_scan_multi": (_I, [_VP, _VP, _L, _VP, _L, _D, _VP, _VP, _I]),
    "pdc_supersmoother_work_bytes": (_L, [_L, _L]),
    "pdc_supersmoother_scan_dev": (_I, [_I, _VP, _VP, _VP, _L, _VP, _L, _D, _VP, _VP, _L]),
    "pdc_test_ss_shape": (_I, [_L, _L, C.POINTER(_L)]),
}


def library_path():
    """The in-tree HIP library; ``PDC_LIBRARY`` names another build of it (kernel A/B experiments)."""
    override = os.environ.get("PDC_LIBRARY")
    if override:
        return override
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def lib():
    """The loaded shared library; raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                path = library_path()
                if not os.path.isfile(path):
                    raise RuntimeError(
                        f"{path} is missing: the HIP extension has not been built "
                        "(run `make -C periodicity_amd/csrc` or `python -c 'import "
                        "__graft_entry__ as g; g.build()'`). There is no CPU fallback.")
                handle = C.CDLL(path)
                for name, (res, args) in PROTOTYPES.items():
                    try:
                        fn = getattr(handle, name)
                    except AttributeError:
                        if os.environ.get("PDC_LIBRARY"):   # an older build under A/B comparison may lack newer entries
                            continue
                        raise
                    fn.restype, fn.argtypes = res, args
                _lib = handle
    return _lib


def check(status):
    if status != 0:
        msg = lib().pdc_last_error().decode("utf-8", "replace")
        raise STATUS_EXC.get(status, RuntimeError)(f"libperiodicity_hip: {msg} (status {status})")


def device_count():
    n = C.c_int(0)
    status = lib().pdc_device_count(C.byref(n))
    return n.value if status == 0 else 0


def pick_device(device=None, devices=None):
    """The ONE precedence rule for the ``device=`` / ``devices=`` pair every scan accepts: a ``devices``
    list, when given, wins (its first entry for a single-device call); else ``device``; else None (the
    process default, ``default_device()``)."""
    if devices is not None and len(devices) > 0:
        return int(devices[0])
    return device


def device_info(device=0):
    name = C.create_string_buffer(256)
    cu, mem, clk = C.c_int(0), C.c_int64(0), C.c_int(0)
    check(lib().pdc_device_info(device, name, 256, C.byref(cu), C.byref(mem), C.byref(clk)))
    return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value,
            "clock_khz": clk.value}


def alloc_counts():
    """(device, pinned-host) allocations the library has made so far in this process."""
    dev, pin = C.c_int64(0), C.c_int64(0)
    check(lib().pdc_alloc_counts(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


def default_device():
    return int(os.environ.get("PERIODICITY_AMD_DEVICE", "0"))


def _f64(a, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def grid_params(frequency):
    """(f0, delta, nf) of a grid built by ``np.arange`` — numpy fills ``start + i*delta`` with
    ``delta = a[1] - a[0]``, which is what the kernels recompute bit-for-bit."""
    frequency = np.asarray(frequency, dtype=np.float64)
    nf = frequency.size
    if nf == 0:
        return 0.0, 0.0, 0
    f0 = float(frequency[0])
    delta = float(frequency[1] - frequency[0]) if nf > 1 else 0.0
    return f0, delta, nf


# ---- host-buffer entry points ---------------------------------------------------------------------
def gls_scan(t, y, dy, f0, delta, nf, fit_mean=True, psd=False, j_begin=0, device=None):
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    out = np.empty(nf, dtype=np.float64)
    dev = default_device() if device is None else device
    check(lib().pdc_gls_scan(_ptr(t), _ptr(y), _ptr(dy), t.size, f0, delta, j_begin, nf,
                             int(bool(fit_mean)), int(bool(psd)), _ptr(out), dev))
    return out


def bglst_scan(t, y, dy, f0, delta, nf, scalars, j_begin=0, device=None):
    """Log marginal likelihood per trial frequency of the harmonic + linear-trend model (``pdc_bglst_scan``);
    ``scalars``: the twelve frequency-independent inputs listed in include/periodicity_hip.h."""
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    scalars = _f64(scalars, "scalars")
    if scalars.size != 12:
        raise ValueError("bglst_scan takes twelve scalars")
    out = np.empty(nf, dtype=np.float64)
    dev = default_device() if device is None else device
    check(lib().pdc_bglst_scan(_ptr(t), _ptr(y), _ptr(dy), t.size, f0, delta, j_begin, nf, _ptr(scalars), _ptr(out), dev))
    return out


def mhgls_scan(t, y, dy, f0, delta, nf, nterms=2, fit_mean=True, psd=False, j_begin=0, device=None):
    """Multi-harmonic GLS power per trial frequency (``pdc_mhgls_scan``): the weighted least-squares fit of a
    Fourier series of ``nterms`` harmonics, with a floating mean when ``fit_mean``."""
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    out = np.empty(nf, dtype=np.float64)
    dev = default_device() if device is None else device
    check(lib().pdc_mhgls_scan(_ptr(t), _ptr(y), _ptr(dy), t.size, f0, delta, j_begin, nf, int(nterms),
                               int(bool(fit_mean)), int(bool(psd)), _ptr(out), dev))
    return out


def mbgls_scan(t, y, dy, band, n_bands, f0, delta, nf, nterms=1, fit_mean=True, psd=False, j_begin=0, device=None):
    """Shared-phase multiband GLS power per trial frequency (``pdc_mbgls_scan``): one Fourier series of ``nterms``
    harmonics common to all bands and, with ``fit_mean``, one floating offset per band; ``band``: int labels in
    ``0 .. n_bands - 1``, one per sample."""
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    band = np.ascontiguousarray(band, dtype=np.int32)
    if y.size != t.size or (dy is not None and dy.size != t.size) or band.ndim != 1 or band.size != t.size:
        raise ValueError("Input arrays have incompatible lengths.")
    out = np.empty(nf, dtype=np.float64)
    dev = default_device() if device is None else device
    check(lib().pdc_mbgls_scan(_ptr(t), _ptr(y), _ptr(dy), _ptr(band), t.size, int(n_bands), f0, delta, j_begin, nf,
                               int(nterms), int(bool(fit_mean)), int(bool(psd)), _ptr(out), dev))
    return out


def mbgls_tile_bins(nterms):
    """Frequencies per tile of the kernel instance ``nterms`` runs (-1 when out of range); no GPU needed."""
    return int(lib().pdc_mbgls_tile_bins(int(nterms)))


def htest_scan(t, w, f0, delta, nf, nharm=20, parts=0, j_begin=0, want=("h", "m", "z2"), device=None):
    """H-test and Z^2 of an event list per trial frequency (``pdc_htest_scan``): arrival times ``t`` in ascending
    order, photon weights ``w`` (None: 1).  Returns ``(h, m, z2)`` - H, the harmonics that give it (int32) and
    Z^2 at ``nharm`` harmonics -, None for what ``want`` leaves out; ``parts``: workgroups that share one tile's
    events (0: chosen from the shape)."""
    t = _f64(t, "t")
    w = None if w is None else _f64(w, "w")
    if w is not None and w.size != t.size:
        raise ValueError("Input arrays have incompatible lengths.")
    unknown = set(want) - {"h", "m", "z2"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    h = np.empty(nf, dtype=np.float64) if "h" in want else None
    m = np.empty(nf, dtype=np.int32) if "m" in want else None
    z2 = np.empty(nf, dtype=np.float64) if "z2" in want else None
    dev = default_device() if device is None else device
    check(lib().pdc_htest_scan(_ptr(t), _ptr(w), t.size, f0, delta, j_begin, nf, int(nharm), int(parts), _ptr(h), _ptr(m),
                               _ptr(z2), dev))
    return h, m, z2


def htest_tile_bins(nharm):
    """Bins per tile of the kernel instance ``nharm`` runs (-1 when out of range); no GPU needed."""
    return int(lib().pdc_htest_tile_bins(int(nharm)))


def htest_last_dispatch():
    """``(ht, k, parts)`` of this thread's last H-test scan."""
    ht, k, parts = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().pdc_htest_last_dispatch(C.byref(ht), C.byref(k), C.byref(parts)))
    return ht.value, k.value, parts.value


FDOT_OUTPUTS = ("plane", "m_plane", "ridge", "ridge_row", "ridge_m", "best")


def htest_fdot_scan(t, w, f0, delta, nf, fdot, epoch, nharm=20, stat="h", parts=0, j_begin=0,
                    want=("plane", "m_plane", "ridge", "ridge_row", "ridge_m", "best"), device=None):
    """H (``stat="h"``) or Z^2 at ``nharm`` (``"z2"``) of an event list over the grid of frequencies times the rows
    ``fdot``, phase ``f tau + fdot tau**2 / 2`` with ``tau = t - epoch`` (``pdc_htest_fdot_scan``).  Returns a dict
    with what ``want`` names (None for the rest): ``plane`` / ``m_plane`` ``[nfd][nf]``, ``ridge`` / ``ridge_row`` /
    ``ridge_m`` ``[nf]`` (per frequency the best row), ``best`` = ``(value, bin, row, m)``.  Z^2 has no ``m``."""
    t, fdot = _f64(t, "t"), _f64(fdot, "fdot")
    w = None if w is None else _f64(w, "w")
    if w is not None and w.size != t.size:
        raise ValueError("Input arrays have incompatible lengths.")
    if stat not in ("h", "z2"):
        raise ValueError("stat must be 'h' or 'z2'")
    unknown = set(want) - set(FDOT_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    want = set(want) - ({"m_plane", "ridge_m"} if stat == "z2" else set())
    nfd = fdot.size
    shapes = {"plane": ((nfd, nf), np.float64), "m_plane": ((nfd, nf), np.int32), "ridge": (nf, np.float64),
              "ridge_row": (nf, np.int32), "ridge_m": (nf, np.int32)}
    out = {name: np.empty(*shapes[name]) if name in want else None for name in shapes}
    best = np.full(1, np.nan) if "best" in want else None
    best_at = np.full(3, -1, dtype=np.int64) if "best" in want else None
    dev = default_device() if device is None else device
    check(lib().pdc_htest_fdot_scan(_ptr(t), _ptr(w), t.size, f0, delta, j_begin, nf, _ptr(fdot), nfd, float(epoch),
                                    int(nharm), 0 if stat == "h" else 1, int(parts), _ptr(out["plane"]),
                                    _ptr(out["m_plane"]), _ptr(out["ridge"]), _ptr(out["ridge_row"]), _ptr(out["ridge_m"]),
                                    _ptr(best), _ptr(best_at), dev))
    out["best"] = None if best is None else (float(best[0]), int(best_at[0]), int(best_at[1]), int(best_at[2]))
    return out


def htest_fdot_last_dispatch():
    """``(ht, k, parts, rows_per_launch, launches)`` of this thread's last plane scan."""
    ht, k, parts, rows, launches = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().pdc_htest_fdot_last_dispatch(C.byref(ht), C.byref(k), C.byref(parts), C.byref(rows), C.byref(launches)))
    return ht.value, k.value, parts.value, rows.value, launches.value


def htest_fdot_work_bytes(n, nf, nfd, nharm=20, parts=0, want_plane=True):
    """Workspace bytes of a plane scan under the current ``PDC_WORK_BUDGET_GB`` (-1: sizes out of range); no GPU needed."""
    return int(lib().pdc_htest_fdot_work_bytes(int(n), int(nf), int(nfd), int(nharm), int(parts), int(bool(want_plane))))


def wwz_scan(t, y, dy, f0, delta, nf, tau, decay, min_neff=6.0, want_planes=True, device=None):
    """Weighted wavelet Z-transform over the time shifts ``tau`` times the grid of frequencies (``pdc_wwz_scan``):
    times ``t`` that never decrease, uncertainties ``dy`` (None: unit).  Returns a dict: ``wwz`` / ``amp`` / ``neff``
    ``[ntau][nf]`` (None without ``want_planes``), ``ridge_bin`` (int64) / ``ridge_wwz`` / ``ridge_amp`` ``[ntau]`` (per
    tau the best bin with ``neff >= min_neff``), ``best`` = ``(value, row, bin)`` and ``visited``, the samples inside
    the support cut summed over all (tile, tau)."""
    t, y, tau = _f64(t, "t"), _f64(y, "y"), _f64(tau, "tau")
    dy = None if dy is None else _f64(dy, "dy")
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    ntau = tau.size
    out = {name: np.empty((ntau, nf)) if want_planes else None for name in ("wwz", "amp", "neff")}
    out["ridge_bin"] = np.empty(ntau, dtype=np.int64)
    out["ridge_wwz"], out["ridge_amp"] = np.empty(ntau), np.empty(ntau)
    best, best_at, visited = np.full(1, np.nan), np.full(2, -1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    dev = default_device() if device is None else device
    check(lib().pdc_wwz_scan(_ptr(t), _ptr(y), _ptr(dy), t.size, f0, delta, nf, _ptr(tau), ntau, float(decay),
                             float(min_neff), _ptr(out["wwz"]), _ptr(out["amp"]), _ptr(out["neff"]),
                             _ptr(out["ridge_bin"]), _ptr(out["ridge_wwz"]), _ptr(out["ridge_amp"]), _ptr(best),
                             _ptr(best_at), _ptr(visited), dev))
    out["best"] = (float(best[0]), int(best_at[0]), int(best_at[1]))
    out["visited"] = int(visited[0])
    return out


def wwz_tile_bins():
    """Bins per tile of the WWZ scan, the unit of its support cut; no GPU needed."""
    return int(lib().pdc_wwz_tile_bins())


def wwz_work_bytes(n, nf, ntau):
    """Workspace bytes of a WWZ scan (-1: sizes out of range); no GPU needed."""
    return int(lib().pdc_wwz_work_bytes(int(n), int(nf), int(ntau)))


def wwz_last_dispatch():
    """``(k, rows_per_launch, launches)`` of this thread's last WWZ scan."""
    k, rows, launches = C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().pdc_wwz_last_dispatch(C.byref(k), C.byref(rows), C.byref(launches)))
    return k.value, rows.value, launches.value


WPS_TABLE = 1024   # entries of the tabulated wavelet


def wps_scan(x, t, periods, scales, table, step, span, corr, want_planes=True, want_coefs=False, device=None):
    """Morlet wavelet power spectrum (``pdc_wps_scan``) of the centred, evenly sampled ``x`` at times ``t``, one row per
    scale (samples per period; ``periods`` only feed the cone-of-influence mask, with ``corr``).  ``table``: the
    integrated wavelet, complex ``[1024]``, ``step`` apart over ``span``.  Returns a dict: ``spectrum`` ``[n_scales][N]``
    (None without ``want_planes``), ``coefs`` complex (None without ``want_coefs``), the marginals reduced on the device
    ``gwps`` / ``masked_gwps`` / ``gwps_count`` (int64) ``[n_scales]`` and ``sav`` / ``masked_sav`` / ``sav_count``
    ``[N]``."""
    x, t, periods, scales = _f64(x, "x"), _f64(t, "t"), _f64(periods, "periods"), _f64(scales, "scales")
    table = np.ascontiguousarray(table, dtype=np.complex128)
    if t.size != x.size or periods.size != scales.size:
        raise ValueError("Input arrays have incompatible lengths.")
    if table.shape != (WPS_TABLE,):
        raise ValueError(f"the wavelet table must have {WPS_TABLE} entries")
    n, ns = x.size, scales.size
    out = {"spectrum": np.empty((ns, n)) if want_planes else None,
           "coefs": np.empty((ns, n), dtype=np.complex128) if want_coefs else None,
           "gwps": np.empty(ns), "masked_gwps": np.empty(ns), "gwps_count": np.empty(ns, dtype=np.int64),
           "sav": np.empty(n), "masked_sav": np.empty(n), "sav_count": np.empty(n, dtype=np.int64)}
    dev = default_device() if device is None else device
    check(lib().pdc_wps_scan(_ptr(x), _ptr(t), n, _ptr(periods), _ptr(scales), ns, _ptr(table), float(step), float(span),
                             float(corr), _ptr(out["spectrum"]), _ptr(out["coefs"]), _ptr(out["gwps"]), _ptr(out["sav"]),
                             _ptr(out["masked_gwps"]), _ptr(out["gwps_count"]), _ptr(out["masked_sav"]),
                             _ptr(out["sav_count"]), dev))
    return out


def wps_taps(scale, step, span):
    """``(position, before, after, L)``: the filter positions of one scale where the table entry changes, ascending,
    with the entries on either side (-1: outside the filter), as the device builds them; no GPU needed."""
    position = np.empty(WPS_TABLE + 1, dtype=np.int64)
    before, after = np.empty(WPS_TABLE + 1, dtype=np.int32), np.empty(WPS_TABLE + 1, dtype=np.int32)
    length = C.c_int64(0)
    count = int(lib().pdc_wps_taps(float(scale), float(step), float(span), _ptr(position), _ptr(before), _ptr(after),
                                   C.byref(length)))
    if count < 0:
        check(count)
    return position[:count], before[:count], after[:count], length.value


def wps_tile():
    """Time indices per workgroup of the WPS scan; no GPU needed."""
    return int(lib().pdc_wps_tile())


def wps_work_bytes(n, n_scales):
    """Workspace bytes of a WPS scan under the current ``PDC_WORK_BUDGET_GB`` (-1: sizes out of range); no GPU needed."""
    return int(lib().pdc_wps_work_bytes(int(n), int(n_scales)))


def wps_last_dispatch():
    """``(tiles, chunks, scales_per_chunk, dense_scales, sparse_scales)`` of this thread's last WPS scan."""
    vals = [C.c_int64(0) for _ in range(5)]
    check(lib().pdc_wps_last_dispatch(*[C.byref(v) for v in vals]))
    return tuple(v.value for v in vals)


EMD_MAX_MODES = 64   # modes per row the device keeps


def _emd_inputs(t, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be two-dimensional: one row per curve")
    t = _f64(t, "t")
    if t.size != x.shape[1]:
        raise ValueError("t and the rows of x differ in length")
    return t, x


def emd_batch(t, x, max_iter=2000, pad_width=2, theta_1=0.05, theta_2=0.50, alpha=0.05, max_modes=EMD_MAX_MODES,
              device=None):
    """Empirical mode decomposition (``pdc_emd_batch``) of the rows ``x[B][N]`` on the shared times ``t[N]``.

    Returns a dict: ``modes`` ``[B][max_modes][N]`` (row ``b`` holds ``n_modes[b]`` modes, zeros after them), ``residue``
    ``[B][N]``, ``n_modes`` ``[B]``, ``sifts`` ``[B][max_modes]`` and ``flags`` ``[B]`` (bit 0: a mode ran into
    ``max_iter``; bit 1: ``max_modes`` reached with the residue not monotonic)."""
    t, x = _emd_inputs(t, x)
    B, n = x.shape
    max_modes = int(max_modes)
    out = {"modes": np.zeros((B, max(max_modes, 0), n)), "residue": np.empty((B, n)),
           "n_modes": np.zeros(B, dtype=np.int64), "sifts": np.zeros((B, max(max_modes, 0)), dtype=np.int64),
           "flags": np.zeros(B, dtype=np.int64)}
    device = default_device() if device is None else device
    check(lib().pdc_emd_batch(_ptr(t), _ptr(x), n, B, int(max_iter), int(pad_width), float(theta_1), float(theta_2),
                              float(alpha), max_modes, _ptr(out["modes"]), _ptr(out["residue"]), _ptr(out["n_modes"]),
                              _ptr(out["sifts"]), _ptr(out["flags"]), device))
    return out


def emd_sift(t, x, pad_width=2, device=None):
    """One sift evaluation (``pdc_emd_sift``) of the curve ``x`` at times ``t``: a dict with ``upper``, ``lower`` ``[N]``,
    the index lists ``maxima``, ``minima``, ``n_zero`` and ``monotonic`` (then the envelopes are None)."""
    t, x = _f64(t, "t"), _f64(x, "x")
    if t.size != x.size:
        raise ValueError("t and x differ in length")
    n = x.size
    upper, lower = np.empty(n), np.empty(n)
    imax, imin = np.zeros(n // 2 + 1, dtype=np.int32), np.zeros(n // 2 + 1, dtype=np.int32)
    counts = np.zeros(4, dtype=np.int64)
    device = default_device() if device is None else device
    check(lib().pdc_emd_sift(_ptr(t), _ptr(x), n, int(pad_width), _ptr(upper), _ptr(lower), _ptr(imax), _ptr(imin),
                             _ptr(counts), device))
    mono = bool(counts[3])
    return {"upper": None if mono else upper, "lower": None if mono else lower,
            "maxima": imax[:counts[0]].astype(np.int64), "minima": imin[:counts[1]].astype(np.int64),
            "n_zero": int(counts[2]), "monotonic": mono}


def emd_lds_samples():
    """Longest row the LDS route of the decomposition serves; no GPU needed."""
    return int(lib().pdc_emd_lds_samples())


def emd_work_bytes(n, n_rows, pad_width=2):
    """Workspace bytes of a decomposition (-1: sizes out of range); no GPU needed."""
    return int(lib().pdc_emd_work_bytes(int(n), int(n_rows), int(pad_width)))


def emd_last_dispatch():
    """``(route, threads, rows, sift_evaluations)`` of this thread's last EMD call; route is "lds" or "global"."""
    vals = [C.c_int64(0) for _ in range(4)]
    check(lib().pdc_emd_last_dispatch(*[C.byref(v) for v in vals]))
    route = {0: None, 1: "lds", 2: "global"}[vals[0].value]
    return (route,) + tuple(v.value for v in vals[1:])


class CeemdanPlan:
    """The ensemble of one CEEMDAN run kept on the device: the noise realisations are decomposed once
    (``pdc_emd_batch_dev``), then every stage (``pdc_ceemdan_stage_dev``) takes the current residue and ``beta[E]`` up and
    brings ``mu[N]`` and the realisations' trajectories back."""

    def __init__(self, t, noise, max_iter=2000, pad_width=2, theta_1=0.05, theta_2=0.50, alpha=0.05,
                 max_modes=EMD_MAX_MODES, device=None):
        t, noise = _emd_inputs(t, noise)
        self.device = default_device() if device is None else device
        self.E, self.n = noise.shape
        self.max_modes = int(max_modes)
        self.params = (int(max_iter), int(pad_width), float(theta_1), float(theta_2), float(alpha))
        E, n, K = self.E, self.n, self.max_modes
        self._bufs = []
        new = lambda nbytes: self._keep(DeviceBuffer(nbytes, self.device))
        self.d_t = self._keep(DeviceBuffer.from_array(t, self.device))
        d_noise = self._keep(DeviceBuffer.from_array(noise, self.device))
        self.d_modes, self.d_nm = new(E * K * n * 8), new(E * 8)
        d_res, d_sifts, d_flags = new(E * n * 8), new(E * K * 8), new(E * 8)
        self.d_residue, self.d_beta, self.d_mu = new(n * 8), new(E * 8), new(n * 8)
        self.d_snm, self.d_ssf, self.d_sfl = new(E * 8), new(E * 8), new(E * 8)
        check(lib().pdc_memset(self.device, d_sifts.ptr, 0, E * K * 8))
        check(lib().pdc_emd_batch_dev(self.device, None, self.d_t.ptr, d_noise.ptr, n, E, *self.params, K,
                                      self.d_modes.ptr, d_res.ptr, self.d_nm.ptr, d_sifts.ptr, d_flags.ptr))
        check(lib().pdc_device_sync(self.device))
        self.n_modes = self.d_nm.to_array(np.int64, E)
        self.sifts = d_sifts.to_array(np.int64, E * K).reshape(E, K)
        self.flags = d_flags.to_array(np.int64, E)

    def _keep(self, buf):
        self._bufs.append(buf)
        return buf

    def noise_mode(self, k):
        """Mode ``k`` of every realisation, ``[E][N]`` (rows without one are zero): one copy of E N values."""
        out = np.zeros((self.E, self.n))
        for e in np.flatnonzero(self.n_modes > k):
            src = self.d_modes.ptr + (int(e) * self.max_modes + int(k)) * self.n * 8
            check(lib().pdc_memcpy_d2h(self.device, _ptr(out[e]), src, self.n * 8))
        return out

    def stage(self, residue, k, beta):
        """``(mu[N], n_modes[E], sifts[E], flags[E])`` of stage ``k``."""
        residue = _f64(residue, "residue")
        beta = _f64(np.broadcast_to(np.asarray(beta, dtype=np.float64), (self.E,)), "beta")
        if residue.size != self.n:
            raise ValueError("the residue and the ensemble differ in length")
        if not (np.all(np.isfinite(residue)) and np.all(np.isfinite(beta))):
            raise ValueError("the residue and beta must be finite")
        dev = self.device
        check(lib().pdc_memcpy_h2d(dev, self.d_residue.ptr, _ptr(residue), residue.nbytes))
        check(lib().pdc_memcpy_h2d(dev, self.d_beta.ptr, _ptr(beta), beta.nbytes))
        check(lib().pdc_ceemdan_stage_dev(dev, None, self.d_t.ptr, self.d_residue.ptr, self.n, self.d_modes.ptr,
                                          self.d_nm.ptr, self.E, self.max_modes, int(k), self.d_beta.ptr, *self.params,
                                          self.d_mu.ptr, self.d_snm.ptr, self.d_ssf.ptr, self.d_sfl.ptr))
        check(lib().pdc_device_sync(dev))
        return (self.d_mu.to_array(np.float64, self.n), self.d_snm.to_array(np.int64, self.E),
                self.d_ssf.to_array(np.int64, self.E), self.d_sfl.to_array(np.int64, self.E))

    def close(self):
        for buf in self._bufs:
            buf.free()
        self._bufs = []


def kepler_scan(t, y, dy, f0, delta, nf, ecc, m0, fit_mean=True, psd=False, want_cube=False, want_bins=True,
                device=None):
    """Keplerian periodogram (``pdc_kepler_scan``): per trial frequency the best weighted least-squares fit of a
    Keplerian orbit over the eccentricities ``ecc`` (each in [0, 0.95]) times the mean anomalies at ``t[0]``, ``m0``
    (cycles, each in [0, 1)).  Returns a dict: ``power`` / ``cell`` (int32) ``[nf]`` (None without ``want_bins``),
    ``cube`` ``[nf][ne][nm]`` (None without ``want_cube``) and ``best`` = ``(value, bin, cell)``."""
    t, y, ecc, m0 = _f64(t, "t"), _f64(y, "y"), _f64(ecc, "ecc"), _f64(m0, "m0")
    dy = None if dy is None else _f64(dy, "dy")
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    nf = int(nf)
    out = {"power": np.empty(max(nf, 0)) if want_bins else None,
           "cell": np.empty(max(nf, 0), dtype=np.int32) if want_bins else None,
           "cube": np.empty((max(nf, 0), ecc.size, m0.size)) if want_cube else None}
    best, best_at = np.full(1, np.nan), np.full(2, -1, dtype=np.int64)
    dev = default_device() if device is None else device
    check(lib().pdc_kepler_scan(_ptr(t), _ptr(y), _ptr(dy), t.size, f0, delta, nf, _ptr(ecc), ecc.size, _ptr(m0), m0.size,
                                int(bool(fit_mean)), int(bool(psd)), _ptr(out["power"]), _ptr(out["cell"]),
                                _ptr(out["cube"]), _ptr(best), _ptr(best_at), dev))
    out["best"] = (float(best[0]), int(best_at[0]), int(best_at[1]))
    return out


def kepler_anomaly(phase, e, device=None):
    """``(cos nu, sin nu)`` of the true anomaly at the mean anomalies ``phase`` (cycles, any finite value) of orbits of
    eccentricity ``e`` (each in [0, 0.95]), by the solver of the Keplerian scan (``pdc_kepler_anomaly``)."""
    phase, e = _f64(phase, "phase"), _f64(e, "e")
    if e.size != phase.size:
        raise ValueError("Input arrays have incompatible lengths.")
    cos_nu, sin_nu = np.empty(phase.size), np.empty(phase.size)
    dev = default_device() if device is None else device
    check(lib().pdc_kepler_anomaly(_ptr(phase), _ptr(e), phase.size, _ptr(cos_nu), _ptr(sin_nu), dev))
    return cos_nu, sin_nu


def kepler_cell_group():
    """Cells per thread of the Keplerian scan; no GPU needed."""
    return int(lib().pdc_kepler_cell_group())


def kepler_tile_bins():
    """Bins per tile of the Keplerian scan; no GPU needed."""
    return int(lib().pdc_kepler_tile_bins())


def kepler_work_bytes(n, nf, ne, nm, want_cube=False):
    """Workspace bytes of a Keplerian scan under the current ``PDC_WORK_BUDGET_GB`` (-1: sizes out of range); no GPU
    needed."""
    return int(lib().pdc_kepler_work_bytes(int(n), int(nf), int(ne), int(nm), int(bool(want_cube))))


def kepler_last_dispatch():
    """``(kc, groups, launches)`` of this thread's last Keplerian scan."""
    kc, groups, launches = C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().pdc_kepler_last_dispatch(C.byref(kc), C.byref(groups), C.byref(launches)))
    return kc.value, groups.value, launches.value


def dcf_scan(ta, a, tb, b, edges, skip_same_index=False, chunk=0, device=None):
    """Discrete correlation function (``pdc_dcf_scan``): every ordered pair of a sample of ``(ta, a)`` and a sample
    of ``(tb, b)`` binned by its lag ``tb[j] - ta[i]`` into ``edges[k] <= lag < edges[k+1]``; times that never decrease.
    Returns ``(pairs, sums)``: the int64 count per bin and the ``[6][nlag]`` sums Sa, Sb, Saa, Sbb, Sab, Sabab.
    ``skip_same_index`` leaves out the pairs ``i == j`` (autocorrelation: pass the same arrays twice); ``chunk``:
    samples of the first curve per partial sum (0: chosen from the shape; every value gives the same counts)."""
    same = ta is tb and a is b
    ta, a, edges = _f64(ta, "ta"), _f64(a, "a"), _f64(edges, "edges")
    tb, b = (ta, a) if same else (_f64(tb, "tb"), _f64(b, "b"))
    if a.size != ta.size or b.size != tb.size:
        raise ValueError("Input arrays have incompatible lengths.")
    nlag = edges.size - 1
    pairs, sums = np.empty(max(nlag, 0), dtype=np.int64), np.empty((6, max(nlag, 0)))
    dev = default_device() if device is None else device
    check(lib().pdc_dcf_scan(_ptr(ta), _ptr(a), ta.size, _ptr(tb), _ptr(b), tb.size, _ptr(edges), nlag,
                             int(bool(skip_same_index)), int(chunk), _ptr(pairs), _ptr(sums), dev))
    return pairs, sums


def dcf_chunk(na, nb, nlag):
    """Samples per chunk a DCF scan would choose under the current ``PDC_WORK_BUDGET_GB`` (-1: sizes out of range); no
    GPU needed."""
    return int(lib().pdc_dcf_chunk(int(na), int(nb), int(nlag)))


def dcf_work_bytes(na, nb, nlag, chunk=0):
    """Workspace bytes of a DCF scan under the current ``PDC_WORK_BUDGET_GB`` (-1: sizes out of range); no GPU needed."""
    return int(lib().pdc_dcf_work_bytes(int(na), int(nb), int(nlag), int(chunk)))


def dcf_last_dispatch():
    """``(chunks, chunk)`` of this thread's last DCF scan."""
    chunks, chunk = C.c_int64(0), C.c_int64(0)
    check(lib().pdc_dcf_last_dispatch(C.byref(chunks), C.byref(chunk)))
    return chunks.value, chunk.value


def _gp_inputs(t_rel, y, var, coeff, jitter, mean):
    """The arrays both GP entries take: ``coeff`` ``[M][J][4]`` of (a, b, c, nu), ``jitter`` and ``mean`` scalars or ``[M]``."""
    t_rel, y, var = _f64(t_rel, "t_rel"), _f64(y, "y"), _f64(var, "var")
    if y.size != t_rel.size or var.size != t_rel.size:
        raise ValueError("Input arrays have incompatible lengths.")
    coeff = np.ascontiguousarray(coeff, dtype=np.float64)
    if coeff.ndim != 3 or coeff.shape[2] != 4:
        raise ValueError("coeff must have the shape [M][J][4]")
    M = coeff.shape[0]
    jitter = np.ascontiguousarray(np.broadcast_to(np.asarray(jitter, dtype=np.float64), (M,)))
    if mean is not None:
        mean = np.ascontiguousarray(np.broadcast_to(np.asarray(mean, dtype=np.float64), (M,)))
    return t_rel, y, var, coeff, jitter, mean


def gp_loglike(t_rel, y, var, coeff, jitter=0.0, mean=None, fit_mean=False, device=None):
    """Celerite log-likelihoods of one curve under ``M`` kernels (``pdc_gp_loglike``): ``t_rel = t - t[0]`` of the sorted
    times, ``var = err ** 2``, ``coeff`` ``[M][J][4]`` of (a, b, c, nu = d / 2 pi).  Returns ``(log_likelihood, mean,
    status)``, each ``[M]``; ``status`` (int32) is 0 or the 1-based sample at which the matrix stopped being positive
    definite (then the likelihood is -inf)."""
    t_rel, y, var, coeff, jitter, mean = _gp_inputs(t_rel, y, var, coeff, jitter, mean)
    M, J = coeff.shape[:2]
    ll, mu, status = np.empty(M), np.empty(M), np.empty(M, dtype=np.int32)
    dev = default_device() if device is None else device
    check(lib().pdc_gp_loglike(_ptr(t_rel), _ptr(y), _ptr(var), t_rel.size, _ptr(coeff), J, _ptr(jitter), _ptr(mean), M,
                               int(bool(fit_mean)), _ptr(ll), _ptr(mu), _ptr(status), dev))
    return ll, mu, status


def gp_scan(t_rel, y, var, coeff, n_periods, jitter=0.0, mean=None, fit_mean=False, want_cube=False, device=None):
    """The same likelihoods for a period-major grid ``[n_periods][nq]`` folded per period (``pdc_gp_scan``).  Returns a
    dict: ``profile``, ``cell`` (int32), ``marginal``, ``mean`` ``[n_periods]``, ``cube`` ``[n_periods][nq]`` (None
    without ``want_cube``) and ``best`` = ``(value, period, cell)``."""
    t_rel, y, var, coeff, jitter, mean = _gp_inputs(t_rel, y, var, coeff, jitter, mean)
    M, J = coeff.shape[:2]
    n_periods = int(n_periods)
    nq = M // n_periods if n_periods > 0 else 0
    rows = max(n_periods, 0)
    out = {"profile": np.empty(rows), "cell": np.empty(rows, dtype=np.int32), "marginal": np.empty(rows),
           "mean": np.empty(rows), "cube": np.empty((rows, nq)) if want_cube else None}
    best, best_at = np.full(1, np.nan), np.full(2, -1, dtype=np.int64)
    dev = default_device() if device is None else device
    check(lib().pdc_gp_scan(_ptr(t_rel), _ptr(y), _ptr(var), t_rel.size, _ptr(coeff), J, _ptr(jitter), _ptr(mean), M,
                            int(bool(fit_mean)), n_periods, nq, _ptr(out["profile"]), _ptr(out["cell"]),
                            _ptr(out["marginal"]), _ptr(out["mean"]), _ptr(out["cube"]), _ptr(best), _ptr(best_at), dev))
    out["best"] = (float(best[0]), int(best_at[0]), int(best_at[1]))
    return out


def gp_work_bytes(n, M, J, want_cube=False):
    """Workspace bytes of a GP call under the current ``PDC_WORK_BUDGET_GB`` (-1: sizes out of range); no GPU needed."""
    return int(lib().pdc_gp_work_bytes(int(n), int(M), int(J), int(bool(want_cube))))


def gp_max_terms():
    """The largest number of celerite terms of a candidate; no GPU needed."""
    return int(lib().pdc_gp_max_terms())


def gp_chunk_samples():
    """Samples the likelihood kernel stages at a time; no GPU needed."""
    return int(lib().pdc_gp_chunk_samples())


def gp_last_dispatch():
    """``(J, fit_mean, launches)`` of this thread's last GP call."""
    J, fit_mean, launches = C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().pdc_gp_last_dispatch(C.byref(J), C.byref(fit_mean), C.byref(launches)))
    return J.value, fit_mean.value, launches.value


def bls_scan(t, y, dy, periods, n_bins, len_min, len_max, min_points=5, dips_only=False, slices=0, device=None):
    """Box least squares at every trial period (``pdc_bls_scan``): ``(power, depth, start_bin, box_bins)`` of the best
    box of ``len_min .. len_max`` of ``n_bins`` phase bins; ``slices``: workgroups that share one period's samples
    (0: chosen from the shape; every value gives the same bits)."""
    t, y, periods = _f64(t, "t"), _f64(y, "y"), _f64(periods, "periods")
    dy = None if dy is None else _f64(dy, "dy")
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    power, depth = np.empty(periods.size, dtype=np.float64), np.empty(periods.size, dtype=np.float64)
    start, box = np.empty(periods.size, dtype=np.int32), np.empty(periods.size, dtype=np.int32)
    dev = default_device() if device is None else device
    check(lib().pdc_bls_scan(_ptr(t), _ptr(y), _ptr(dy), t.size, _ptr(periods), periods.size, int(n_bins), int(len_min),
                             int(len_max), int(min_points), int(bool(dips_only)), int(slices), _ptr(power), _ptr(depth),
                             _ptr(start), _ptr(box), dev))
    return power, depth, start, box


def gls_scan_batch(t, y, dy, offsets, f0, delta, nf, fit_mean=True, psd=False, shared_t=False,
                   want_power=True, want_peaks=False, j_begin=0, device=None, devices=None):
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    nb = offsets.size - 1
    if nb < 1 or offsets[-1] != y.size or (dy is not None and dy.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    if (shared_t and t.size != offsets[1]) or (not shared_t and t.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    power = np.empty((nb, nf), dtype=np.float64) if want_power else None
    amax = np.empty(nb, dtype=np.float64) if want_peaks else None
    argmax = np.empty(nb, dtype=np.int64) if want_peaks else None
    if devices is not None and len(devices) > 1:
        # curves dealt to the device slots in contiguous groups, no exchange (pdc_gls_scan_batch_multi)
        if j_begin:
            raise ValueError("a batch sharded over devices scans the whole grid (j_begin must be 0)")
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        check(lib().pdc_gls_scan_batch_multi(_ptr(t), _ptr(y), _ptr(dy), _ptr(offsets), nb, int(shared_t),
                                             f0, delta, nf, int(bool(fit_mean)), int(bool(psd)),
                                             _ptr(power), _ptr(amax), _ptr(argmax), _ptr(devs), devs.size))
        return power, amax, argmax
    device = pick_device(device, devices)
    dev = default_device() if device is None else device
    check(lib().pdc_gls_scan_batch(_ptr(t), _ptr(y), _ptr(dy), _ptr(offsets), nb, int(shared_t),
                                   f0, delta, j_begin, nf, int(bool(fit_mean)), int(bool(psd)),
                                   _ptr(power), _ptr(amax), _ptr(argmax), dev))
    return power, amax, argmax


def gls_bootstrap(t, y, dy, picks, f0, delta, nf, fit_mean=True, psd=False, method="direct", device=None,
                  devices=None):
    """Maxima (and their bins) of the periodograms of the bootstrap replicates ``(y[picks[b]], dy[picks[b]])``
    on the unchanged time axis (``pdc_gls_bootstrap``): only the curve and the int32 indices are uploaded,
    the resampled arrays are never built.  ``method="fft"``: ``f0`` / ``delta`` are ``fmin`` / ``df``."""
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    picks = np.ascontiguousarray(picks, dtype=np.int32)
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    if picks.ndim != 2 or (picks.shape[0] and picks.shape[1] != t.size):
        raise ValueError("picks must be [n_bootstraps][n_samples]")
    nb = picks.shape[0]
    amax = np.empty(nb, dtype=np.float64)
    argmax = np.empty(nb, dtype=np.int64)
    if devices is not None and len(devices) > 0:
        devs = np.ascontiguousarray(devices, dtype=np.int32)
    else:
        devs = np.array([default_device() if device is None else device], dtype=np.int32)
    check(lib().pdc_gls_bootstrap(_ptr(t), _ptr(y), _ptr(dy), t.size, _ptr(picks), nb, float(f0), float(delta),
                                  int(nf), int(bool(fit_mean)), int(bool(psd)), 1 if method == "fft" else 0,
                                  _ptr(amax), _ptr(argmax), _ptr(devs), devs.size))
    return amax, argmax


GLS_ROUTES = ("none", "general", "parts", "balanced", "shared", "shared2")
_GLS_DISPATCH_FIELDS = ("route", "K", "S", "tiles", "parts", "parts_by_xcd", "bal_slots", "wide_prep", "bpad", "groups",
                        "z_len", "bal_chunks", "lead_swap", "chunk_sums")


def gls_last_dispatch():
    """TEST HOOK (``pdc_test_gls_last_dispatch``): the route the calling thread's last direct-sum GLS scan took and its
    launch shape, as a dict (``route`` by name, see ``GLS_ROUTES``)."""
    out = (C.c_int64 * len(_GLS_DISPATCH_FIELDS))()
    check(lib().pdc_test_gls_last_dispatch(out))
    rec = dict(zip(_GLS_DISPATCH_FIELDS, (int(v) for v in out)))
    rec["route"] = GLS_ROUTES[rec["route"]]
    return rec


def gls_last_pair():
    """TEST HOOK (``pdc_test_gls_last_pair``): ``(ran, table_bytes)`` - whether the calling thread's last direct-sum GLS
    scan ran the mirrored-pair kernel, and the bytes of its per-sample offset table."""
    out = (C.c_int64 * 2)()
    check(lib().pdc_test_gls_last_pair(out))
    return bool(out[0]), int(out[1])


def gls_scan_multi(t, y, dy, f0, delta, nf, fit_mean=True, psd=False, devices=(0,)):
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    devs = np.ascontiguousarray(devices, dtype=np.int32)
    out = np.empty(nf, dtype=np.float64)
    check(lib().pdc_gls_scan_multi(_ptr(t), _ptr(y), _ptr(dy), t.size, f0, delta, nf,
                                   int(bool(fit_mean)), int(bool(psd)), _ptr(out), _ptr(devs),
                                   devs.size))
    return out


class GlsPlan:
    """A persistent multi-GPU GLS plan (``pdc_gls_plan_*``): buffers, streams and RCCL communicators
    are created once; ``scan`` only enqueues (double-buffered), ``download`` waits and copies."""

    def __init__(self, devices, n_max, nf_max, loopback_slots=None):
        """``loopback_slots=k``: k logical slots on the ONE device listed, the all-gather replaced by the
        equivalent device-to-device copies (``pdc_gls_plan_create_loopback``) - how the N > 1 logic runs
        on a single GPU."""
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        self._plan = C.c_void_p()
        if loopback_slots is not None:
            if devs.size != 1:
                raise ValueError("a loopback plan lives on one device")
            self.devices = [int(devs[0])] * int(loopback_slots)
            check(lib().pdc_gls_plan_create_loopback(int(devs[0]), int(loopback_slots), int(n_max),
                                                     int(nf_max), C.byref(self._plan)))
        else:
            self.devices = [int(d) for d in devs]
            check(lib().pdc_gls_plan_create(_ptr(devs), devs.size, int(n_max), int(nf_max),
                                            C.byref(self._plan)))
        self.nf = 0

    def info(self):
        """``{"n_slots", "rccl_ranks", "exchange"}`` - the communicator size as RCCL reports it and which
        exchange the plan performs ("none", "rccl", "copy")."""
        n, r, x = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().pdc_gls_plan_info(self._plan, C.byref(n), C.byref(r), C.byref(x)))
        buf = C.create_string_buffer(512)
        check(lib().pdc_gls_plan_init_error(self._plan, buf, 512))
        return {"n_slots": n.value, "rccl_ranks": r.value, "exchange": ("none", "rccl", "copy")[x.value],
                "init_error": buf.value.decode() or None}

    def upload(self, t, y, dy=None):
        t, y = _f64(t, "t"), _f64(y, "y")
        dy = None if dy is None else _f64(dy, "dy")
        if y.size != t.size or (dy is not None and dy.size != t.size):
            raise ValueError("Input arrays have incompatible lengths.")
        check(lib().pdc_gls_plan_upload(self._plan, _ptr(t), _ptr(y), _ptr(dy), t.size))

    def scan(self, f0, delta, nf, fit_mean=True, psd=False):
        check(lib().pdc_gls_plan_scan(self._plan, float(f0), float(delta), int(nf),
                                      int(bool(fit_mean)), int(bool(psd))))
        self.nf = int(nf)

    def wait(self):
        check(lib().pdc_gls_plan_wait(self._plan))

    def download(self, which=0):
        out = np.empty(self.nf, dtype=np.float64)
        check(lib().pdc_gls_plan_download(self._plan, _ptr(out), self.nf, int(which)))
        return out

    def kernel_ms(self):
        ms = C.c_float()
        check(lib().pdc_gls_plan_kernel_ms(self._plan, C.byref(ms)))
        return ms.value

    def slot_ms(self):
        """HIP-event time of the latest slab scan on every slot."""
        ms = (C.c_float * len(self.devices))()
        check(lib().pdc_gls_plan_slot_ms(self._plan, ms, len(self.devices)))
        return [float(v) for v in ms]

    def close(self):
        if self._plan:
            check(lib().pdc_gls_plan_destroy(self._plan))
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def trig_sums(t, w, f0, delta, nf, device=None):
    t, w = _f64(t, "t"), _f64(w, "w")
    if w.size != t.size:
        raise ValueError("Input arrays have incompatible lengths.")
    S, Cc = np.empty(nf), np.empty(nf)
    dev = default_device() if device is None else device
    check(lib().pdc_trig_sums(_ptr(t), _ptr(w), t.size, f0, delta, nf, _ptr(S), _ptr(Cc), dev))
    return S, Cc


def gls_scan_fft(t, y, dy, fmin, df, nf, fit_mean=True, psd=False, device=None):
    """The reference's own FFT/extirpolation algorithm on the device (Tier F)."""
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    if y.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    out = np.empty(nf, dtype=np.float64)
    dev = default_device() if device is None else device
    check(lib().pdc_gls_scan_fft(_ptr(t), _ptr(y), _ptr(dy), t.size, float(fmin), float(df), nf,
                                 int(bool(fit_mean)), int(bool(psd)), _ptr(out), dev))
    return out


def gls_scan_fft_batch(t, y, dy, offsets, fmin, df, nf, fit_mean=True, psd=False, shared_t=False,
                       want_power=True, want_peaks=False, device=None):
    """Batch of curves through the FFT path (Tier F); same layout/outputs as ``gls_scan_batch``."""
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    nb = offsets.size - 1
    if nb < 1 or offsets[-1] != y.size or (dy is not None and dy.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    if (shared_t and t.size != offsets[1]) or (not shared_t and t.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    power = np.empty((nb, nf), dtype=np.float64) if want_power else None
    amax = np.empty(nb, dtype=np.float64) if want_peaks else None
    argmax = np.empty(nb, dtype=np.int64) if want_peaks else None
    dev = default_device() if device is None else device
    check(lib().pdc_gls_scan_fft_batch(_ptr(t), _ptr(y), _ptr(dy), _ptr(offsets), nb, int(shared_t),
                                       float(fmin), float(df), nf, int(bool(fit_mean)),
                                       int(bool(psd)), _ptr(power), _ptr(amax), _ptr(argmax), dev))
    return power, amax, argmax


def trig_sums_fft(t, h, df, nf, fmin, device=None):
    """``_trig_sum(t, h, df, nf, fmin)`` (spectral.py:11-40) on the device."""
    t, h = _f64(t, "t"), _f64(h, "h")
    if h.size != t.size:
        raise ValueError("Input arrays have incompatible lengths.")
    S, Cc = np.empty(nf), np.empty(nf)
    dev = default_device() if device is None else device
    check(lib().pdc_trig_sums_fft(_ptr(t), _ptr(h), t.size, float(df), nf, float(fmin), _ptr(S),
                                  _ptr(Cc), dev))
    return S, Cc


def highest_peak(power, device=None):
    """(index, value) of the highest ``find_peaks`` local maximum of each row of ``power``."""
    power = np.ascontiguousarray(power, dtype=np.float64)
    rows = power.reshape(1, -1) if power.ndim == 1 else power
    idx = np.empty(rows.shape[0], dtype=np.int64)
    val = np.empty(rows.shape[0], dtype=np.float64)
    dev = default_device() if device is None else device
    check(lib().pdc_highest_peak(_ptr(rows), rows.shape[0], rows.shape[1], _ptr(idx), _ptr(val), dev))
    return (int(idx[0]), float(val[0])) if power.ndim == 1 else (idx, val)


def gls_batch_highest_peak(t, y, dy, offsets, f0, delta, nf, fit_mean=True, psd=False,
                           shared_t=False, device=None):
    """Batched periodograms reduced on the device to each curve's highest peak (index, power)."""
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    nb = offsets.size - 1
    if nb < 1 or offsets[-1] != y.size or (dy is not None and dy.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    if (shared_t and t.size != offsets[1]) or (not shared_t and t.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    idx = np.empty(nb, dtype=np.int64)
    val = np.empty(nb, dtype=np.float64)
    dev = default_device() if device is None else device
    check(lib().pdc_gls_batch_highest_peak(_ptr(t), _ptr(y), _ptr(dy), _ptr(offsets), nb,
                                           int(shared_t), f0, delta, nf, int(bool(fit_mean)),
                                           int(bool(psd)), _ptr(idx), _ptr(val), dev))
    return idx, val


def _topk_outputs(nb, k):
    return {"count": np.empty(nb, dtype=np.int64), "indices": np.empty((nb, k), dtype=np.int64),
            "heights": np.empty((nb, k)), "prominences": np.empty((nb, k)),
            "half_lo": np.empty((nb, k), dtype=np.int64), "half_hi": np.empty((nb, k), dtype=np.int64)}


def _table_ptrs(table):
    """A peak table's six arrays as pointers, in the order every ``pdc_*peaks*`` entry takes them."""
    return tuple(_ptr(table[name]) for name in ("count", "indices", "heights", "prominences", "half_lo", "half_hi"))


def peaks_topk(power, k=1, by_prominence=False, device=None):
    """The ``k`` (<= 1024; beyond 128 in launches of 128 ranks) highest, or most prominent, ``find_peaks`` maxima of each row of ``power`` with
    prominences and half-maximum crossings (``pdc_peaks_topk``); a dict of arrays shaped ``[rows, k]``
    (``count``: ``[rows]``), ranked descending, padded with -1 / NaN."""
    power = np.ascontiguousarray(power, dtype=np.float64)
    rows = power.reshape(1, -1) if power.ndim == 1 else power
    out = _topk_outputs(rows.shape[0], int(k))
    dev = default_device() if device is None else device
    check(lib().pdc_peaks_topk(_ptr(rows), rows.shape[0], rows.shape[1], int(k), int(bool(by_prominence)),
                               *_table_ptrs(out), dev))
    return out


def gls_batch_peaks(t, y, dy, offsets, f0, delta, nf, k=1, by_prominence=False, fit_mean=True,
                    psd=False, shared_t=False, device=None):
    """Batched periodograms reduced on the device to their ``k`` best peaks (see :func:`peaks_topk`)."""
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    nb = offsets.size - 1
    if nb < 1 or offsets[-1] != y.size or (dy is not None and dy.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    if (shared_t and t.size != offsets[1]) or (not shared_t and t.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    out = _topk_outputs(nb, int(k))
    dev = default_device() if device is None else device
    check(lib().pdc_gls_batch_peaks(_ptr(t), _ptr(y), _ptr(dy), _ptr(offsets), nb, int(shared_t), f0,
                                    delta, nf, int(bool(fit_mean)), int(bool(psd)), int(k),
                                    int(bool(by_prominence)), *_table_ptrs(out), dev))
    return out


def _ragged_inputs(t, y, dy, offsets, f0, delta, f_offsets):
    t, y = _f64(t, "t"), _f64(y, "y")
    dy = None if dy is None else _f64(dy, "dy")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    f_offsets = np.ascontiguousarray(f_offsets, dtype=np.int64)
    f0, delta = _f64(f0, "f0"), _f64(delta, "delta")
    nb = offsets.size - 1
    if nb < 1 or f_offsets.size != nb + 1 or f0.size != nb or delta.size != nb:
        raise ValueError("offsets / f_offsets need n_curves + 1 entries, f0 / delta n_curves")
    if offsets[-1] != y.size or t.size != y.size or (dy is not None and dy.size != y.size):
        raise ValueError("Input arrays have incompatible lengths.")
    return t, y, dy, offsets, f0, delta, f_offsets, nb


def _slots(device, devices):
    if devices is not None and len(devices) > 0:
        return np.ascontiguousarray(devices, dtype=np.int32)
    return np.array([default_device() if device is None else device], dtype=np.int32)


def gls_scan_ragged(t, y, dy, offsets, f0, delta, f_offsets, fit_mean=True, psd=False, want_power=True,
                    want_peaks=False, device=None, devices=None):
    """Batch of curves, each on its own grid ``f0[b] + j*delta[b]``, ``j < f_offsets[b+1] - f_offsets[b]``
    (``pdc_gls_scan_ragged``): ``(power [f_offsets[-1]] | None, amax [B] | None, argmax [B] | None)``."""
    t, y, dy, offsets, f0, delta, f_offsets, nb = _ragged_inputs(t, y, dy, offsets, f0, delta, f_offsets)
    power = np.empty(int(f_offsets[-1]), dtype=np.float64) if want_power else None
    amax = np.empty(nb, dtype=np.float64) if want_peaks else None
    argmax = np.empty(nb, dtype=np.int64) if want_peaks else None
    devs = _slots(device, devices)
    check(lib().pdc_gls_scan_ragged(_ptr(t), _ptr(y), _ptr(dy), _ptr(offsets), nb, _ptr(f0), _ptr(delta),
                                    _ptr(f_offsets), int(bool(fit_mean)), int(bool(psd)), _ptr(power), _ptr(amax),
                                    _ptr(argmax), _ptr(devs), devs.size))
    return power, amax, argmax


def gls_ragged_peaks(t, y, dy, offsets, f0, delta, f_offsets, k=1, by_prominence=False, fit_mean=True, psd=False,
                     want_power=False, device=None, devices=None):
    """The peak table of :func:`gls_batch_peaks` on every curve's own grid (``pdc_gls_ragged_peaks``); with
    ``want_power`` also the spectra (``"power"``, ``[f_offsets[-1]]``)."""
    t, y, dy, offsets, f0, delta, f_offsets, nb = _ragged_inputs(t, y, dy, offsets, f0, delta, f_offsets)
    out = _topk_outputs(nb, int(k))
    out["power"] = np.empty(int(f_offsets[-1]), dtype=np.float64) if want_power else None
    devs = _slots(device, devices)
    check(lib().pdc_gls_ragged_peaks(_ptr(t), _ptr(y), _ptr(dy), _ptr(offsets), nb, _ptr(f0), _ptr(delta),
                                     _ptr(f_offsets), int(bool(fit_mean)), int(bool(psd)), int(k),
                                     int(bool(by_prominence)), *_table_ptrs(out), _ptr(out["power"]), _ptr(devs),
                                     devs.size))
    return out


def _linspace_inputs(t, v, dy, offsets, start, step, stop, p_offsets, names):
    """The inputs of a batch whose curves each have a linspace grid, converted and checked: ``(t, v, dy, offsets,
    start, step, stop, p_offsets, n_curves)``; ``names``: what ``t`` and ``v`` are called in a message."""
    t, v = _f64(t, names[0]), _f64(v, names[1])
    dy = None if dy is None else _f64(dy, "dy")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    p_offsets = np.ascontiguousarray(p_offsets, dtype=np.int64)
    start, step, stop = _f64(start, "start"), _f64(step, "step"), _f64(stop, "stop")
    nb = offsets.size - 1
    if nb < 1 or p_offsets.size != nb + 1 or any(a.size != nb for a in (start, step, stop)):
        raise ValueError("offsets / p_offsets need n_curves + 1 entries, start / step / stop n_curves")
    if offsets[-1] != t.size or v.size != t.size or (dy is not None and dy.size != t.size):
        raise ValueError("Input arrays have incompatible lengths.")
    return t, v, dy, offsets, start, step, stop, p_offsets, nb


def phase_scan_ragged(kind, t, x, offsets, start, step, stop, p_offsets, nb, nc, sigma=None, significant=None,
                      k=0, by_prominence=False, want_power=True, device=None, devices=None):
    """PDM (kind 0), AoV (1) or conditional entropy (2) over a batch of curves, each on its own period grid
    ``linspace(start[b], stop[b], p_offsets[b+1] - p_offsets[b])`` (``pdc_phase_scan_ragged``; with ``k > 0``
    ``pdc_phase_ragged_peaks``): ``(out [p_offsets[-1]] | None, peak table dict | None)``."""
    t, x, _, offsets, start, step, stop, p_offsets, nb_ = _linspace_inputs(t, x, None, offsets, start, step, stop,
                                                                           p_offsets, "tx")
    sigma = None if sigma is None else _f64(sigma, "sigma")
    significant = None if significant is None else _f64(significant, "significant")
    out = np.empty(int(p_offsets[-1]), dtype=np.float64) if want_power else None
    devs = _slots(device, devices)
    common = (int(kind), _ptr(t), _ptr(x), _ptr(offsets), nb_, _ptr(start), _ptr(step), _ptr(stop), _ptr(p_offsets),
              _ptr(sigma), _ptr(significant), int(nb), int(nc))
    if not k:
        check(lib().pdc_phase_scan_ragged(*common, _ptr(out), _ptr(devs), devs.size))
        return out, None
    table = _topk_outputs(nb_, int(k))
    check(lib().pdc_phase_ragged_peaks(*common, int(k), int(bool(by_prominence)), *_table_ptrs(table), _ptr(out),
                                       _ptr(devs), devs.size))
    return out, table


def bls_scan_ragged(t, y, dy, offsets, start, step, stop, p_offsets, n_bins, len_min, len_max, min_points=5,
                    dips_only=False, k=0, by_prominence=False, want_power=True, device=None, devices=None):
    """Box least squares over a batch of curves, each on its own period grid ``linspace(start[b], stop[b],
    p_offsets[b+1] - p_offsets[b])`` (``pdc_bls_scan_ragged``; with ``k > 0`` ``pdc_bls_ragged_peaks``):
    ``(rows | None, best, peak table dict | None)``.  ``rows``: the dict ``power, depth, start_bin, box_bins``
    ``[p_offsets[-1]]`` (None without ``want_power``: they stay on the device); ``best``: the dict ``index, power,
    depth, start_bin, box_bins`` ``[n_curves]`` of every row's first maximum, found on the device."""
    t, y, dy, offsets, start, step, stop, p_offsets, nb_ = _linspace_inputs(t, y, dy, offsets, start, step, stop,
                                                                            p_offsets, "ty")
    total = max(int(p_offsets[-1]), 0)
    rows = None
    if want_power:
        rows = {"power": np.empty(total, dtype=np.float64), "depth": np.empty(total, dtype=np.float64),
                "start_bin": np.empty(total, dtype=np.int32), "box_bins": np.empty(total, dtype=np.int32)}
    best = {"index": np.empty(nb_, dtype=np.int64), "power": np.empty(nb_, dtype=np.float64),
            "depth": np.empty(nb_, dtype=np.float64), "start_bin": np.empty(nb_, dtype=np.int32),
            "box_bins": np.empty(nb_, dtype=np.int32)}
    devs = _slots(device, devices)
    common = (_ptr(t), _ptr(y), _ptr(dy), _ptr(offsets), nb_, _ptr(start), _ptr(step), _ptr(stop), _ptr(p_offsets),
              int(n_bins), int(len_min), int(len_max), int(min_points), int(bool(dips_only)))
    outs = tuple(_ptr(rows[name]) if rows else None for name in ("power", "depth", "start_bin", "box_bins")) + \
        tuple(_ptr(best[name]) for name in ("index", "power", "depth", "start_bin", "box_bins"))
    if not k:
        check(lib().pdc_bls_scan_ragged(*common, *outs, _ptr(devs), devs.size))
        return rows, best, None
    table = _topk_outputs(nb_, int(k))
    check(lib().pdc_bls_ragged_peaks(*common, int(k), int(bool(by_prominence)), *_table_ptrs(table), *outs, _ptr(devs),
                                     devs.size))
    return rows, best, table


def bls_ragged_groups():
    """Test hook: groups of curves the last BLS batch call of this process ran."""
    g = C.c_int64()
    check(lib().pdc_test_bls_ragged_groups(C.byref(g)))
    return g.value


def stringlength_scan_ragged(t, m, offsets, start, step, stop, p_offsets, k=0, by_prominence=False,
                             want_power=True, device=None, devices=None):
    """StringLength over a batch of curves, each on its own grid ``1 / linspace(start[b], stop[b], P_b)``
    (``pdc_stringlength_scan_ragged``; with ``k > 0`` ``pdc_stringlength_ragged_peaks``):
    ``(out [p_offsets[-1]] | None, peak table dict | None)``."""
    t, m, _, offsets, start, step, stop, p_offsets, nb_ = _linspace_inputs(t, m, None, offsets, start, step, stop,
                                                                           p_offsets, "tm")
    out = np.empty(int(p_offsets[-1]), dtype=np.float64) if want_power else None
    devs = _slots(device, devices)
    common = (_ptr(t), _ptr(m), _ptr(offsets), nb_, _ptr(start), _ptr(step), _ptr(stop), _ptr(p_offsets))
    if not k:
        check(lib().pdc_stringlength_scan_ragged(*common, _ptr(out), _ptr(devs), devs.size))
        return out, None
    table = _topk_outputs(nb_, int(k))
    check(lib().pdc_stringlength_ragged_peaks(*common, int(k), int(bool(by_prominence)), *_table_ptrs(table), _ptr(out),
                                              _ptr(devs), devs.size))
    return out, table


def sl_ragged_stats():
    """Test hook: ``(groups, marked pairs, long curves)`` of the last StringLength batch call."""
    g, mk, lc = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().pdc_test_sl_ragged_stats(C.byref(g), C.byref(mk), C.byref(lc)))
    return g.value, mk.value, lc.value


def _period_scan(entry, arrays, periods, params, device, devices):
    """Behind the six single-grid scans: ``arrays`` (``(name, values)`` pairs, all of one length) and ``periods``
    converted and checked, then ``pdc_<entry>`` on one device, or ``pdc_<entry>_multi`` when ``devices`` lists more than
    one: one contiguous slab of the period grid per entry."""
    arrays = [_f64(a, name) for name, a in arrays]
    periods = _f64(periods, "periods")
    if any(a.size != arrays[0].size for a in arrays):
        raise ValueError("Input arrays have incompatible lengths.")
    out = np.empty(periods.size, dtype=np.float64)
    args = (*[_ptr(a) for a in arrays], arrays[0].size, _ptr(periods), periods.size, *params, _ptr(out))
    if devices is not None and len(devices) > 1:
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        check(getattr(lib(), f"pdc_{entry}_multi")(*args, _ptr(devs), devs.size))
        return out
    device = pick_device(device, devices)
    check(getattr(lib(), f"pdc_{entry}")(*args, default_device() if device is None else device))
    return out


def pdm_scan(t, x, periods, nb, nc, sigma, device=None, devices=None):
    """theta at every trial period; ``devices`` (a sequence of GPU ordinals) cuts the period grid
    into one contiguous slab per entry (``pdc_pdm_scan_multi``)."""
    return _period_scan("pdm_scan", (("t", t), ("x", x)), periods, (int(nb), int(nc), float(sigma)), device, devices)


def aov_scan(t, x, periods, n_bins, device=None, devices=None):
    """Analysis-of-Variance statistic at every trial period (``pdc_aov_scan``; ``devices`` as in
    :func:`pdm_scan`)."""
    return _period_scan("aov_scan", (("t", t), ("x", x)), periods, (int(n_bins),), device, devices)


def cond_entropy_scan(t, mag_bin, periods, n_phase, n_mag, device=None, devices=None):
    """Conditional entropy at every trial period (``pdc_cond_entropy_scan``); ``mag_bin`` holds the
    magnitude bin (0 .. n_mag-1) of every sample; ``devices`` as in :func:`pdm_scan`."""
    mag_bin = _f64(mag_bin, "mag_bin")
    if mag_bin.size and not (np.all(mag_bin >= 0) and np.all(mag_bin < n_mag)):
        raise ValueError("magnitude bins must lie in 0 .. n_mag-1")
    return _period_scan("cond_entropy_scan", (("t", t), ("mag_bin", mag_bin)), periods, (int(n_phase), int(n_mag)),
                        device, devices)


def gl_scan(t, periods, m, n_offsets, device=None, devices=None):
    """Gregory-Loredo ``ln S_m`` at every trial period for the arrival times ``t`` (``pdc_gl_scan``): ``m``
    phase bins, the bin-offset integral as the mean over ``n_offsets`` shifts; ``devices`` as in
    :func:`pdm_scan`."""
    return _period_scan("gl_scan", (("t", t),), periods, (int(m), int(n_offsets)), device, devices)


def stringlength_scan(t, m, periods, device=None, devices=None):
    """String length at every trial period; ``devices`` as in :func:`pdm_scan`
    (``pdc_stringlength_scan_multi``)."""
    return _period_scan("stringlength_scan", (("t", t), ("m", m)), periods, (), device, devices)


PHASE_KINDS = {"pdm": 0, "aov": 1, "cond_entropy": 2, "stringlength": 3, "gregory_loredo": 4, "supersmoother": 5}
_PHASE_DISPATCH_FIELDS = ("kind", "split", "block", "waves", "periods_per_wg", "workgroups", "n_z", "z_len", "n_stat",
                          "scan_lds", "finish_lds")


def phase_shape(kind, n, n_periods, nb, nc=1):
    """TEST HOOK (``pdc_test_phase_shape``): the route a phase-binning scan of this shape would take in this process,
    as a dict; no device is touched.  ``kind``: a key of ``PHASE_KINDS`` or its number; ``nb``, ``nc`` as
    ``pdc_phase_scan_dev`` takes them (Gregory-Loredo: ``nb = m * n_offsets``, ``nc = m``)."""
    out = (C.c_int64 * len(_PHASE_DISPATCH_FIELDS))()
    check(lib().pdc_test_phase_shape(PHASE_KINDS.get(kind, kind), int(n), int(n_periods), int(nb), int(nc), out))
    return dict(zip(_PHASE_DISPATCH_FIELDS, (int(v) for v in out)))


def phase_last_dispatch():
    """TEST HOOK (``pdc_test_phase_last_dispatch``): the route of the last phase-binning launch in this process, with
    the keys of :func:`phase_shape`; all zeros before the first."""
    out = (C.c_int64 * len(_PHASE_DISPATCH_FIELDS))()
    check(lib().pdc_test_phase_last_dispatch(out))
    return dict(zip(_PHASE_DISPATCH_FIELDS, (int(v) for v in out)))


def supersmoother_scan(t, y, periods, alpha=0.0, device=None, devices=None):
    """Mean absolute residual of the folded curve about its supersmoother fit at every trial period
    (``pdc_supersmoother_scan``; Friedman 1984 + Reimann 1994, a TODO upstream)."""
    return _period_scan("supersmoother_scan", (("t", t), ("y", y)), periods, (float(alpha),), device, devices)


class PhasePlan:
    """A persistent fan-out of the phase scans over device slots (``pdc_phase_plan_*``): streams, buffers
    and page-locked staging are created once; ``upload`` replicates the samples, ``scan`` only enqueues one
    slab of the period grid per slot, ``download`` waits and returns the whole grid."""

    def __init__(self, devices, n_max=0, n_periods_max=0):
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        self.devices = [int(d) for d in devs]
        self._plan = C.c_void_p()
        check(lib().pdc_phase_plan_create(_ptr(devs), devs.size, int(n_max), int(n_periods_max),
                                          C.byref(self._plan)))
        self.n_periods = 0

    def upload(self, t, v):
        t, v = _f64(t, "t"), _f64(v, "v")
        if v.size != t.size:
            raise ValueError("Input arrays have incompatible lengths.")
        check(lib().pdc_phase_plan_upload(self._plan, _ptr(t), _ptr(v), t.size))

    def scan(self, kind, periods, nb=1, nc=1, sigma=1.0):
        periods = _f64(periods, "periods")
        check(lib().pdc_phase_plan_scan(self._plan, PHASE_KINDS[kind], _ptr(periods), periods.size, int(nb),
                                        int(nc), float(sigma)))
        self.n_periods = periods.size

    def wait(self):
        check(lib().pdc_phase_plan_wait(self._plan))

    def download(self):
        out = np.empty(self.n_periods, dtype=np.float64)
        check(lib().pdc_phase_plan_download(self._plan, _ptr(out), self.n_periods))
        return out

    def kernel_ms(self):
        ms = C.c_float()
        check(lib().pdc_phase_plan_kernel_ms(self._plan, C.byref(ms)))
        return ms.value

    def close(self):
        if self._plan:
            check(lib().pdc_phase_plan_destroy(self._plan))
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- device-resident helpers (bench.py, tests) ----------------------------------------------------
class DeviceBuffer:
    """A raw HBM allocation owned by the caller."""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        check(lib().pdc_malloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_array(cls, a, device=0):
        a = np.ascontiguousarray(a)
        buf = cls(a.nbytes, device)
        check(lib().pdc_memcpy_h2d(device, buf.ptr, _ptr(a), a.nbytes))
        return buf

    def to_array(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        check(lib().pdc_memcpy_d2h(self.device, _ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            check(lib().pdc_free(self.device, self.ptr))
            self.ptr = None
