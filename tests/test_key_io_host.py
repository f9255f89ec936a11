"""-m "not gpu": the key-file entry points that run on the GPU (keyio.hip) are declared, exported and refuse bad arguments before
they touch a device: plk_srs_load_key / plk_srs_store_key / plk_g1_decode_dev / plk_g1_encode_dev."""
import ctypes
import os
import re

import plonkit_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("plk_srs_load_key", "plk_srs_store_key", "plk_g1_decode_dev", "plk_g1_encode_dev")
ERR_ARG = 1


def test_header_declares_and_library_exports_the_key_io_entry_points():
    header = open(os.path.join(ROOT, "include", "plonkit_amd.h"), encoding="utf-8").read()
    L = pa.lib()
    for name in NAMES + ("plk_key_chunk_points",):
        assert re.search(r"^\s*(?:int32_t|uint64_t)\s+%s\s*\(" % name, header, re.M), "%s is not declared in include/plonkit_amd.h" % name
        assert hasattr(L, name), "%s is not exported by the library" % name
    assert re.search(r"#define\s+PLK_KEY_LAGRANGE\s+1u", header)
    chunk = L.plk_key_chunk_points()
    assert 0 < chunk <= 1 << 21, "a three-chunk key must stay a few hundred MiB of host memory"


def test_bad_arguments_are_refused_without_a_device():
    L = pa.lib()
    raw = open(os.path.join(ROOT, "tests", "golden", "setup_2pow10.key"), "rb").read()
    n, ln, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    g2 = ctypes.create_string_buffer(256)
    fake = ctypes.create_string_buffer(1 << 16)          # stands where a context would: a bad flag is refused before the context is read
    size, zero = ctypes.c_uint64(len(raw)), ctypes.c_uint64(0)
    # null ctx / data / n_out
    assert L.plk_srs_load_key(None, raw, size, zero, zero, ctypes.c_uint32(0), ctypes.byref(n), g2, ctypes.byref(bad)) == ERR_ARG
    assert "plk_srs_load_key" in pa.last_error()
    assert L.plk_srs_load_key(fake, None, size, zero, zero, ctypes.c_uint32(0), ctypes.byref(n), g2, None) == ERR_ARG
    assert L.plk_srs_load_key(fake, raw, size, zero, zero, ctypes.c_uint32(0), None, g2, None) == ERR_ARG
    # unknown flag bits
    for flags in (2, 3, 0x80000000):
        assert L.plk_srs_load_key(fake, raw, size, zero, zero, ctypes.c_uint32(flags), ctypes.byref(n), g2, None) == ERR_ARG
        assert L.plk_srs_store_key(fake, ctypes.c_uint32(flags), g2, None, zero, ctypes.byref(ln)) == ERR_ARG
    assert L.plk_srs_store_key(None, ctypes.c_uint32(0), g2, None, zero, ctypes.byref(ln)) == ERR_ARG
    assert L.plk_srs_store_key(fake, ctypes.c_uint32(0), None, None, zero, ctypes.byref(ln)) == ERR_ARG
    assert L.plk_srs_store_key(fake, ctypes.c_uint32(0), g2, None, zero, None) == ERR_ARG
    # the kernels on device pointers: null context, null or misaligned buffers
    assert L.plk_g1_decode_dev(None, ctypes.c_void_p(256), ctypes.c_uint64(1), ctypes.c_void_p(512), ctypes.byref(bad), None) == ERR_ARG
    assert L.plk_g1_encode_dev(None, ctypes.c_void_p(256), ctypes.c_uint64(1), ctypes.c_void_p(512), None) == ERR_ARG
    assert L.plk_g1_decode_dev(fake, None, ctypes.c_uint64(1), ctypes.c_void_p(512), None, None) == ERR_ARG
    assert L.plk_g1_decode_dev(fake, ctypes.c_void_p(264), ctypes.c_uint64(1), ctypes.c_void_p(512), None, None) == ERR_ARG      # file + 8
    assert L.plk_g1_encode_dev(fake, ctypes.c_void_p(256), ctypes.c_uint64(1), None, None) == ERR_ARG
    assert L.plk_g1_encode_dev(fake, ctypes.c_void_p(256), ctypes.c_uint64(1), ctypes.c_void_p(520), None) == ERR_ARG
