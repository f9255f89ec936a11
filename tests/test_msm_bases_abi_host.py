"""-m "not gpu": the entry points of the commitments against caller-supplied bases exist in the loaded library, and refuse a null
context with PLK_ERR_ARG and a message before they touch a device."""
import ctypes
import subprocess

import numpy as np

import plonkit_amd as pa

SYMBOLS = ("plk_msm_g1_bases", "plk_msm_g1_bases_dev", "plk_msm_g1_bases_batch_dev", "plk_srs_check_points_dev")
PLK_ERR_ARG = 1


def test_the_four_symbols_are_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", pa.lib_path()]).decode()
    L = pa.lib()
    for s in SYMBOLS:
        assert " T %s\n" % s in out, s
        getattr(L, s)


def test_the_python_layer_has_the_four_methods():
    for name in ("msm_bases", "msm_bases_dev", "msm_bases_batch_dev", "srs_check_points_dev"):
        assert callable(getattr(pa.Context, name)), name


def test_null_context_is_err_arg_with_a_message():
    L = pa.lib()
    out = np.full(8, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    keep = out.copy()
    o = out.ctypes.data_as(ctypes.c_void_p)
    bases, scalars = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)
    bad = ctypes.c_uint64(7)
    rc = L.plk_msm_g1_bases(None, bases.ctypes.data_as(ctypes.c_void_p), scalars.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(2), ctypes.c_uint32(0), o,
                            ctypes.byref(bad))
    assert rc == PLK_ERR_ARG and "plk_msm_g1_bases" in pa.last_error() and bad.value == 2**64 - 1
    bad = ctypes.c_uint64(7)
    rc = L.plk_msm_g1_bases_dev(None, ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_uint64(0), ctypes.c_uint32(0), o, ctypes.byref(bad), None)
    assert rc == PLK_ERR_ARG and "plk_msm_g1_bases_dev" in pa.last_error() and bad.value == 2**64 - 1
    ptrs = (ctypes.c_void_p * 2)(None, None)
    rc = L.plk_msm_g1_bases_batch_dev(None, ctypes.c_void_p(0), ptrs, ctypes.c_uint32(2), ctypes.c_uint64(0), ctypes.c_uint32(0), o, None, None)
    assert rc == PLK_ERR_ARG and "plk_msm_g1_bases_batch_dev" in pa.last_error()
    valid, bad = ctypes.c_int32(5), ctypes.c_uint64(7)
    rc = L.plk_srs_check_points_dev(None, ctypes.c_void_p(0), ctypes.c_uint64(0), bytes(256), None, ctypes.c_uint32(0), ctypes.byref(valid), ctypes.byref(bad), None)
    assert rc == PLK_ERR_ARG and "plk_srs_check_points_dev" in pa.last_error() and valid.value == 0 and bad.value == 2**64 - 1
    assert np.array_equal(out, keep)
