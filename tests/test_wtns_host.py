"""-m "not gpu": the entry points of the witness stream (wtnsio.hip, prover.hip) are declared, exported and refuse bad arguments before
they touch a device, and plk_wtns_decode's container checks (made on the host, before the context is read) give plk_circuit_load's codes
and words on the same bytes."""
import ctypes
import os
import re
import struct

import pytest

import plonkit_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("plk_fr_decode_dev", "plk_fr_encode_dev", "plk_wtns_decode", "plk_prove_witness", "plk_prove_witness_dev", "plk_prove_wtns",
         "plk_validate_witness_dev")
ERR_ARG, ERR_FORMAT = 1, 6
u64, vp = ctypes.c_uint64, ctypes.c_void_p


def _golden_wtns():
    c = pa.Circuit.from_files(os.path.join(GOLD, "circuit.r1cs.json"), os.path.join(GOLD, "witness.json"))
    return c.export("wtns")


def test_header_declares_and_library_exports_the_seven_entry_points():
    header = open(os.path.join(ROOT, "include", "plonkit_amd.h"), encoding="utf-8").read()
    L = pa.lib()
    for name in NAMES:
        assert re.search(r"^\s*int32_t\s+%s\s*\(" % name, header, re.M), "%s is not declared in include/plonkit_amd.h" % name
        assert hasattr(L, name), "%s is not exported by the library" % name
    for method in ("fr_decode_dev", "fr_encode_dev", "wtns_decode"):
        assert callable(getattr(pa.Context, method))
    for method in ("prove_witness", "prove_witness_dev", "prove_wtns", "validate_witness_dev"):
        assert callable(getattr(pa.SetupForProver, method))


def test_bad_arguments_are_refused_without_a_device():
    L = pa.lib()
    wt = _golden_wtns()
    fake = ctypes.create_string_buffer(1 << 16)          # stands where a context (or a setup) would: refused before it is read
    n, bad, ln, valid = u64(0), u64(0), u64(0), ctypes.c_int32(0)
    buf = ctypes.create_string_buffer(1 << 12)
    # the kernels on device pointers: null context, null or misaligned buffers
    assert L.plk_fr_decode_dev(None, vp(256), u64(1), vp(512), ctypes.byref(bad), None) == ERR_ARG
    assert "plk_fr_decode_dev" in pa.last_error()
    assert L.plk_fr_encode_dev(None, vp(256), u64(1), vp(512), None) == ERR_ARG
    assert L.plk_fr_decode_dev(fake, None, u64(1), vp(512), None, None) == ERR_ARG
    assert L.plk_fr_decode_dev(fake, vp(256), u64(1), None, None, None) == ERR_ARG
    assert L.plk_fr_decode_dev(fake, vp(256 + 76), u64(1), vp(512), None, None) == ERR_ARG      # the payload's offset in the file
    assert L.plk_fr_decode_dev(fake, vp(256), u64(1), vp(520), None, None) == ERR_ARG
    assert L.plk_fr_encode_dev(fake, vp(256), u64(1), None, None) == ERR_ARG
    assert L.plk_fr_encode_dev(fake, vp(264), u64(1), vp(512), None) == ERR_ARG
    assert L.plk_fr_encode_dev(fake, vp(256), u64(1), vp(520), None) == ERR_ARG
    # the file decoder: null ctx / data / n_out, a misaligned destination
    assert L.plk_wtns_decode(None, wt, u64(len(wt)), None, u64(0), ctypes.byref(n), ctypes.byref(bad), None) == ERR_ARG
    assert "plk_wtns_decode" in pa.last_error() and bad.value == 2**64 - 1
    assert L.plk_wtns_decode(fake, None, u64(len(wt)), None, u64(0), ctypes.byref(n), None, None) == ERR_ARG
    assert L.plk_wtns_decode(fake, wt, u64(len(wt)), None, u64(0), None, None, None) == ERR_ARG
    assert L.plk_wtns_decode(fake, wt, u64(len(wt)), vp(520), u64(4), ctypes.byref(n), None, None) == ERR_ARG
    # fr_dev == NULL only reports the count, and a buffer that is too small is refused: neither reads the context
    assert L.plk_wtns_decode(fake, wt, u64(len(wt)), None, u64(0), ctypes.byref(n), ctypes.byref(bad), None) == 0 and n.value == 4
    assert L.plk_wtns_decode(fake, wt, u64(len(wt)), vp(512), u64(3), ctypes.byref(n), None, None) == ERR_ARG and n.value == 4
    # the prove and validate calls
    w = (ctypes.c_uint64 * 16)()
    assert L.plk_prove_witness(None, fake, w, u64(4), buf, u64(len(buf)), ctypes.byref(ln)) == ERR_ARG
    assert "plk_prove_witness" in pa.last_error()
    assert L.plk_prove_witness(fake, None, w, u64(4), buf, u64(len(buf)), ctypes.byref(ln)) == ERR_ARG
    assert L.plk_prove_witness(fake, fake, None, u64(4), buf, u64(len(buf)), ctypes.byref(ln)) == ERR_ARG
    assert L.plk_prove_witness(fake, fake, w, u64(4), None, u64(0), ctypes.byref(ln)) == ERR_ARG
    assert L.plk_prove_witness(fake, fake, w, u64(4), buf, u64(len(buf)), None) == ERR_ARG
    assert L.plk_prove_witness_dev(None, fake, vp(256), u64(4), buf, u64(len(buf)), ctypes.byref(ln), None) == ERR_ARG
    assert L.plk_prove_witness_dev(fake, None, vp(256), u64(4), buf, u64(len(buf)), ctypes.byref(ln), None) == ERR_ARG
    assert L.plk_prove_witness_dev(fake, fake, None, u64(4), buf, u64(len(buf)), ctypes.byref(ln), None) == ERR_ARG
    assert L.plk_prove_witness_dev(fake, fake, vp(264), u64(4), buf, u64(len(buf)), ctypes.byref(ln), None) == ERR_ARG
    assert "16-byte aligned" in pa.last_error()
    assert L.plk_prove_wtns(None, fake, wt, u64(len(wt)), buf, u64(len(buf)), ctypes.byref(ln), ctypes.byref(bad)) == ERR_ARG
    assert L.plk_prove_wtns(fake, None, wt, u64(len(wt)), buf, u64(len(buf)), ctypes.byref(ln), None) == ERR_ARG
    assert L.plk_prove_wtns(fake, fake, None, u64(len(wt)), buf, u64(len(buf)), ctypes.byref(ln), None) == ERR_ARG
    assert L.plk_prove_wtns(fake, fake, wt, u64(len(wt)), None, u64(0), ctypes.byref(ln), None) == ERR_ARG
    assert L.plk_prove_wtns(fake, fake, wt[:-1], u64(len(wt) - 1), buf, u64(len(buf)), ctypes.byref(ln), None) == ERR_FORMAT     # container first
    assert L.plk_validate_witness_dev(None, fake, vp(256), u64(4), ctypes.byref(valid), ctypes.byref(bad), None) == ERR_ARG
    assert L.plk_validate_witness_dev(fake, None, vp(256), u64(4), ctypes.byref(valid), None, None) == ERR_ARG
    assert L.plk_validate_witness_dev(fake, fake, None, u64(4), ctypes.byref(valid), None, None) == ERR_ARG
    assert L.plk_validate_witness_dev(fake, fake, vp(256), u64(4), None, None, None) == ERR_ARG
    assert L.plk_validate_witness_dev(fake, fake, vp(264), u64(4), ctypes.byref(valid), None, None) == ERR_ARG


def _corruptions(wt):
    """one field of the container at a time: (name, bytes, the words parse_wtns_bin has for it)"""
    def put(off, fmt, v):
        b = bytearray(wt)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)
    return [("magic", b"wtnx" + wt[4:], "invalid file header"),
            ("short magic", wt[:3], "invalid file header"),
            ("version", put(4, "<I", 3), "unsupported file version"),
            ("num sections", put(8, "<I", 3), "invalid num sections"),
            ("first section type", put(12, "<I", 2), "invalid section type"),
            ("first section len", put(16, "<Q", 41), "invalid section len"),
            ("field byte size", put(24, "<I", 31), "invalid field byte size"),
            ("prime", put(28, "<B", 2), "invalid curve prime"),
            ("truncated in the prime", wt[:40], "invalid curve prime"),
            ("second section type", put(64, "<I", 1), "invalid section type"),
            ("section size", put(68, "<Q", 32 * 4 + 1), "invalid witness section size"),
            ("count", put(60, "<I", 5), "invalid witness section size"),
            ("one byte short", wt[:-1], "read witness failed: truncated"),
            ("no payload", wt[:76], "read witness failed: truncated")]


def test_container_errors_are_plk_circuit_loads():
    L = pa.lib()
    wt = _golden_wtns()
    assert len(wt) == 76 + 4 * 32
    r1cs = open(os.path.join(GOLD, "circuit.r1cs.json"), "rb").read()
    fake = ctypes.create_string_buffer(1 << 16)
    n = u64(0)
    for name, data, words in _corruptions(wt):
        with pytest.raises(pa.PlkError) as e:
            pa.Circuit(r1cs, True, data, False)
        assert e.value.code == ERR_FORMAT and words in str(e.value), name
        want = str(e.value).split(": ", 1)[1]
        assert L.plk_wtns_decode(fake, data, u64(len(data)), None, u64(0), ctypes.byref(n), None, None) == ERR_FORMAT, name
        assert pa.last_error() == want, name
        # (a destination does not change the order: the container is checked before the context is read)
        assert L.plk_wtns_decode(fake, data, u64(len(data)), vp(512), u64(1 << 20), ctypes.byref(n), None, None) == ERR_FORMAT, name
        assert pa.last_error() == want, name
