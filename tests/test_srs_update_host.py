"""-m "not gpu": the host half of a key update (srs_update.hip): plk_srs_update_receipt makes g2_new = {Q_0, s Q_1} and the receipt
S1 = s G1, S2 = s Q_0; plk_srs_update_check_receipt is every rule of plk_srs_update_verify but the key's own structure check.
The reference has no counterpart.  The referees are the trapdoor of the reference's own tests/golden/setup_2pow10.key (tau = 42),
the oracle's G1 arithmetic (oracle_lib.g1_mul) and the twist arithmetic of tests/gen/forged_proofs.py (g2_mul_bytes / g2_pair, which
first reproduces the golden key's 42 G2).  The only arithmetic of this file is the construction of a twist point outside the order-r
subgroup, as in test_gpu_key_check.py: an Fq2 square root and [r]Q != O by double-and-add."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import Q_MOD, R_MOD
from tests.gen import forged_proofs as fp

ERR_ARG = 1
TAU = 42
S254 = 0x2b6f1d3c5a79880716253443526170fedcba98765432100123456789abcdef01 % R_MOD     # a fixed 254-bit value
SCALARS = [1, 2, R_MOD - 1, S254]
NEW_SYMBOLS = ("plk_srs_update", "plk_srs_update_receipt", "plk_srs_update_verify", "plk_srs_update_check_receipt", "plk_srs_update_last_ms")
G1_INF = b"\x40" + b"\x00" * 63


@pytest.fixture(scope="module")
def pa():
    import plonkit_amd
    return plonkit_amd


@pytest.fixture(scope="module")
def key(golden_dir):
    """(points 0 and 1, the G2 section) of the golden key"""
    raw = open(os.path.join(golden_dir, "setup_2pow10.key"), "rb").read()
    pts = po.read_crs(raw).g1
    assert raw[-256:] == fp.g2_pair(TAU)
    return np.ascontiguousarray(pts[:2]), raw[-256:]


def _g1_bytes(pa, p):
    return pa.g1_to_bytes(p)


def _new_p01(p01, s):
    return np.stack([p01[0], ol.g1_mul(p01[1], s)])


def _honest(pa, key, s):
    p01, g2 = key
    g2_new, receipt = pa.srs_update_receipt(ol.fr_mont(s), g2)
    return p01, _new_p01(p01, s), g2, g2_new, receipt


# ------------------------------------------------------------------------------------------------ correct receipts
def test_s254_is_254_bits():
    assert S254.bit_length() == 254 and 0 < S254 < R_MOD


@pytest.mark.parametrize("s", SCALARS, ids=["1", "2", "r-1", "254bit"])
def test_receipt_against_the_trapdoor(pa, key, s):
    p01, g2 = key
    g2_new, receipt = pa.srs_update_receipt(ol.fr_mont(s), g2)
    assert g2_new == fp.g2_pair(TAU * s % R_MOD)
    assert receipt[:64] == _g1_bytes(pa, ol.g1_mul(ol.g1_generator(), s))
    assert receipt[64:] == fp.g2_pair(s)[128:]
    assert len(receipt) == 192
    assert pa.srs_update_check_receipt(p01, _new_p01(p01, s), g2, g2_new, receipt) == (True, "ok")
    # a one-point key: the rule on point 1 is skipped, nothing of the [1] entries is read
    assert pa.srs_update_check_receipt(p01[:1], p01[:1], g2, g2_new, receipt) == (True, "ok")


# ------------------------------------------------------------------------------------------------ refusals, each with its own reason
# (the arithmetic of test_gpu_key_check.py for a twist point outside the subgroup)
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q_MOD, (a[0] * b[1] + a[1] * b[0]) % Q_MOD)


def _f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q_MOD)
    return (a[0] * n % Q_MOD, -a[1] * n % Q_MOD)


def _f2sub(a, b):
    return ((a[0] - b[0]) % Q_MOD, (a[1] - b[1]) % Q_MOD)


def _fq_sqrt(a):
    s = pow(a, (Q_MOD + 1) // 4, Q_MOD)                          # q = 3 mod 4
    return s if s * s % Q_MOD == a % Q_MOD else None


def _f2sqrt(a):
    a0, a1 = a
    if a1 == 0:
        s = _fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = _fq_sqrt(-a0 % Q_MOD)
        return None if s is None else (0, s)
    norm = _fq_sqrt((a0 * a0 + a1 * a1) % Q_MOD)
    if norm is None:
        return None
    half = pow(2, -1, Q_MOD)
    for t in ((a0 + norm) * half % Q_MOD, (a0 - norm) * half % Q_MOD):
        x0 = _fq_sqrt(t)
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, Q_MOD) % Q_MOD)
            if _f2mul(x, x) == (a0 % Q_MOD, a1 % Q_MOD):
                return x
    return None


TWIST_B = _f2mul((3, 0), _f2inv((9, 1)))


def _g2_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == (0, 0):
            return None
        m = _f2mul(_f2mul((3, 0), _f2mul(p[0], p[0])), _f2inv(_f2mul((2, 0), p[1])))
    else:
        m = _f2mul(_f2sub(q[1], p[1]), _f2inv(_f2sub(q[0], p[0])))
    x = _f2sub(_f2sub(_f2mul(m, m), p[0]), q[0])
    return (x, _f2sub(_f2mul(m, _f2sub(p[0], x)), p[1]))


def _g2_mul(p, k):
    acc = None
    for bit in bin(k)[2:]:
        acc = _g2_add(acc, acc)
        if bit == "1":
            acc = _g2_add(acc, p)
    return acc


def _g2_encode(p):
    return b"".join(v.to_bytes(32, "big") for v in (p[0][1], p[0][0], p[1][1], p[1][0]))


def _g2_decode(b):
    c = [int.from_bytes(b[32 * j: 32 * j + 32], "big") for j in range(4)]
    return ((c[1], c[0]), (c[3], c[2]))


@pytest.fixture(scope="module")
def stray(key):
    """128 bytes of a twist point with [r]Q != O; the arithmetic is checked on the generator first"""
    g = _g2_decode(key[1][:128])
    assert _g2_mul(g, R_MOD) is None and _g2_encode(_g2_mul(g, TAU)) == key[1][128:]
    for k in range(1, 200):
        x = (k, 0)
        y = _f2sqrt(tuple((u + v) % Q_MOD for u, v in zip(_f2mul(_f2mul(x, x), x), TWIST_B)))
        if y is not None and _g2_mul((x, y), R_MOD) is not None:
            return _g2_encode((x, y))
    raise AssertionError("no twist point found")


def test_a_receipt_of_s_plus_1(pa, key):
    """the key moved by s, the receipt made with s + 1: S1 and S2 agree with each other and with nothing else"""
    p01, new, g2, g2_new, _ = _honest(pa, key, S254)
    _, other = pa.srs_update_receipt(ol.fr_mont(S254 + 1), g2)
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new, other) == (False, "p1_mismatch")
    # on a one-point key the G2 side is the first to disagree
    assert pa.srs_update_check_receipt(p01[:1], new[:1], g2, g2_new, other) == (False, "q1_mismatch")


def test_s1_and_s2_from_different_secrets(pa, key):
    p01, new, g2, g2_new, receipt = _honest(pa, key, S254)
    _, other = pa.srs_update_receipt(ol.fr_mont(2), g2)
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new, other[:64] + receipt[64:]) == (False, "receipt_split")
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new, receipt[:64] + other[64:]) == (False, "receipt_split")


def test_s1_at_infinity_or_off_the_curve(pa, key):
    p01, new, g2, g2_new, receipt = _honest(pa, key, 2)
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new, G1_INF + receipt[64:]) == (False, "bad_s1")
    bad = bytearray(receipt)
    bad[63] ^= 1
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new, bytes(bad)) == (False, "bad_s1")


def test_s2_outside_the_subgroup_or_at_infinity(pa, key, stray):
    p01, new, g2, g2_new, receipt = _honest(pa, key, 2)
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new, receipt[:64] + stray) == (False, "bad_s2")
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new, receipt[:64] + fp.G2_INF) == (False, "bad_s2")
    bad = bytearray(receipt)
    bad[191] ^= 1                                                # off the twist
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new, bytes(bad)) == (False, "bad_s2")


def test_g2_new_left_as_it_was(pa, key):
    p01, new, g2, _, receipt = _honest(pa, key, 2)
    assert pa.srs_update_check_receipt(p01, new, g2, g2, receipt) == (False, "q1_mismatch")
    _, _, _, g2_one, receipt_one = _honest(pa, key, 1)           # s = 1 is the one secret for which nothing moves
    assert g2_one == g2 and pa.srs_update_check_receipt(p01, p01, g2, g2, receipt_one) == (True, "ok")


def test_q0_changed(pa, key):
    p01, new, g2, g2_new, receipt = _honest(pa, key, 2)
    two_q0 = fp.g2_mul_bytes(g2[:128], 2)
    assert pa.srs_update_check_receipt(p01, new, g2, two_q0 + g2_new[128:], receipt) == (False, "q0_changed")


def test_a_g2_section_outside_the_subgroup(pa, key, stray):
    p01, new, g2, g2_new, receipt = _honest(pa, key, 2)
    assert pa.srs_update_check_receipt(p01, new, g2, g2_new[:128] + stray, receipt) == (False, "bad_g2")
    assert pa.srs_update_check_receipt(p01, new, g2[:128] + fp.G2_INF, g2_new, receipt) == (False, "bad_g2")


def test_point_0_changed(pa, key):
    p01, new, g2, g2_new, receipt = _honest(pa, key, 2)
    moved = new.copy()
    moved[0] = ol.g1_mul(p01[0], 2)
    assert pa.srs_update_check_receipt(p01, moved, g2, g2_new, receipt) == (False, "p0_changed")
    zero = np.zeros_like(p01)
    zero[1] = p01[1]
    gone = new.copy()
    gone[0] = 0
    assert pa.srs_update_check_receipt(zero, gone, g2, g2_new, receipt) == (False, "p0_changed")     # infinity on both sides


def test_point_1_of_another_scalar(pa, key):
    p01, new, g2, g2_new, receipt = _honest(pa, key, S254)
    other = new.copy()
    other[1] = ol.g1_mul(p01[1], S254 - 1)
    assert pa.srs_update_check_receipt(p01, other, g2, g2_new, receipt) == (False, "p1_mismatch")
    other[1] = p01[1]                                            # left as it was
    assert pa.srs_update_check_receipt(p01, other, g2, g2_new, receipt) == (False, "p1_mismatch")


# ------------------------------------------------------------------------------------------------ arguments
def test_arguments(pa, key):
    L = pa.lib()
    p01, new, g2, g2_new, receipt = _honest(pa, key, 2)
    out_g2, out_r = ctypes.create_string_buffer(b"\xaa" * 256, 256), ctypes.create_string_buffer(b"\xbb" * 192, 192)
    s2 = ol.fr_mont(2)
    sp = s2.ctypes.data_as(ctypes.c_void_p)

    def refused(rc, who):
        assert rc == ERR_ARG
        assert who + ":" in pa.last_error(), pa.last_error()

    zero = np.zeros(4, dtype=np.uint64)
    refused(L.plk_srs_update_receipt(zero.ctypes.data_as(ctypes.c_void_p), g2, out_g2, out_r), "plk_srs_update_receipt")
    r_limbs = ol.int_to_limbs(R_MOD)                             # limbs >= r: not a residue
    refused(L.plk_srs_update_receipt(r_limbs.ctypes.data_as(ctypes.c_void_p), g2, out_g2, out_r), "plk_srs_update_receipt")
    refused(L.plk_srs_update_receipt(None, g2, out_g2, out_r), "plk_srs_update_receipt")
    refused(L.plk_srs_update_receipt(sp, None, out_g2, out_r), "plk_srs_update_receipt")
    refused(L.plk_srs_update_receipt(sp, g2, None, out_r), "plk_srs_update_receipt")
    refused(L.plk_srs_update_receipt(sp, g2, out_g2, None), "plk_srs_update_receipt")
    bad = bytearray(g2)
    bad[255] ^= 1                                                # off the twist: plk_srs_check's words
    refused(L.plk_srs_update_receipt(sp, bytes(bad), out_g2, out_r), "plk_srs_update_receipt")
    assert "G2 point not on the twist" in pa.last_error()
    refused(L.plk_srs_update_receipt(sp, g2[:128] + fp.G2_INF, out_g2, out_r), "plk_srs_update_receipt")
    assert out_g2.raw == b"\xaa" * 256 and out_r.raw == b"\xbb" * 192          # a refused call writes nothing
    with pytest.raises(pa.PlkError) as e:
        pa.srs_update_receipt(None, g2)
    assert e.value.code == ERR_ARG

    valid, reason = ctypes.c_int32(7), ctypes.c_uint32(7)
    po_, pn = p01.ctypes.data_as(ctypes.c_void_p), new.ctypes.data_as(ctypes.c_void_p)
    two = ctypes.c_uint32(2)
    name = "plk_srs_update_check_receipt"
    refused(L.plk_srs_update_check_receipt(None, pn, two, g2, g2_new, receipt, ctypes.byref(valid), ctypes.byref(reason)), name)
    assert valid.value == 0
    refused(L.plk_srs_update_check_receipt(po_, None, two, g2, g2_new, receipt, ctypes.byref(valid), ctypes.byref(reason)), name)
    refused(L.plk_srs_update_check_receipt(po_, pn, ctypes.c_uint32(0), g2, g2_new, receipt, ctypes.byref(valid), ctypes.byref(reason)), name)
    refused(L.plk_srs_update_check_receipt(po_, pn, two, None, g2_new, receipt, ctypes.byref(valid), ctypes.byref(reason)), name)
    refused(L.plk_srs_update_check_receipt(po_, pn, two, g2, None, receipt, ctypes.byref(valid), ctypes.byref(reason)), name)
    refused(L.plk_srs_update_check_receipt(po_, pn, two, g2, g2_new, None, ctypes.byref(valid), ctypes.byref(reason)), name)
    refused(L.plk_srs_update_check_receipt(po_, pn, two, g2, g2_new, receipt, None, ctypes.byref(reason)), name)
    refused(L.plk_srs_update_check_receipt(po_, pn, two, bytes(bad), g2_new, receipt, ctypes.byref(valid), ctypes.byref(reason)), name)
    assert "G2 point not on the twist" in pa.last_error()
    assert L.plk_srs_update_check_receipt(po_, pn, two, g2, g2_new, receipt, ctypes.byref(valid), None) == 0 and valid.value == 1   # reason may be NULL
    # the two calls that need a context refuse a null one before they touch a device
    refused(L.plk_srs_update(None, sp, ctypes.c_uint64(0), g2, out_g2, out_r), "plk_srs_update")
    refused(L.plk_srs_update_verify(None, po_, g2, g2_new, receipt, None, ctypes.byref(valid), ctypes.byref(reason)), "plk_srs_update_verify")


# ------------------------------------------------------------------------------------------------ declarations
def test_the_header_declares_what_the_library_exports(pa):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "plonkit_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int32_t %s\(" % name, header, re.M), name
        assert hasattr(pa.lib(), name), name
    names = re.findall(r"PLK_UPDATE_([A-Z0-9_]+) = (\d+)", header)
    assert [n.lower() for n, _ in names] == list(pa.UPDATE_REASONS) and [int(v) for _, v in names] == list(range(len(names)))
