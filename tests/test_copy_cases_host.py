"""-m "not gpu": the model and the cases of the copy-constraint checks (tests/gen/copy_cases.py) before they judge a kernel, and the per-value
decode of plonkit_amd/csrc/sigma_decode_dev.h compiled for the CPU.

1. On every case the model's decode of sigmas_of(nxt) is index_of(nxt): the dictionary inverts the forward rule of perm_cases.py.
2. The cases tell wrong decoders from the right one (as tests/test_perm_cases_host.py does for wrong sorts): one that ignores the coset, one
   that returns the row's bits reversed, one that is wrong at row N - 1 only, one that accepts a value of order 2N.
3. tests/host/sigma_decode_kat.hip runs sigma_decode itself on the host at EVERY log_n from 1 to 26 — labels of all four cosets at rows
   0, 1, N/2, N - 1 and three random ones, and the values it must refuse (0, 2 omega^i, omega_2N, r, a label + r; r - 1 is a label of every
   domain) — against the model's exponentiation.  Only here is log_n > 20 exercised: a 2^26 vector is too slow to make for a test.
The model's reports for the directed circuits are pinned too, so that the GPU tests compare with something a reader can check by hand."""
import os
import random
import shutil
import struct
import subprocess

import pytest

from tests.gen import copy_cases as cc
from tests.gen import perm_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_decode_inverts_sigmas_of_on_every_case():
    cases = cc.decode_cases()
    assert {"copy/log_n=%d" % l for l in cc.DIRECT_LOG_N} <= set(cases)
    assert {"degenerate/all_dummy", "degenerate/all_distinct", "hub/64_distinct_digits", "size/log_n=12"} <= set(cases)
    for name, (log_n, sig, want) in cases.items():
        idx, bad = cc.decode(sig, log_n)
        assert bad is None and idx == want, name
        assert cc.imageless(idx) is None, name
        assert cc.report(sig, log_n) == (cc.OK, None, None), name


def test_decode_value_agrees_with_the_dictionary():
    rng = random.Random(7)
    for log_n in (1, 2, 5, 9):
        lab = cc.labels(log_n)
        for x, p in rng.sample(sorted(lab.items()), min(len(lab), 40)):
            assert cc.decode_value(x, log_n) == p
        for _ in range(40):
            x = rng.randrange(cc.R_MOD)
            assert cc.decode_value(x, log_n) == lab.get(x, cc.NOT_A_LABEL)
        for name, v in cc.non_labels(log_n, rng):
            assert cc.decode([[v] + [1] * ((1 << log_n) - 1)] + [[1] * (1 << log_n)] * 3, log_n)[0][0] == cc.NOT_A_LABEL, name


@pytest.mark.parametrize("wrong", cc.WRONG_DECODERS, ids=[f.__name__ for f in cc.WRONG_DECODERS])
def test_cases_tell_a_wrong_decoder_from_the_right_one(wrong):
    told = []
    for name, (log_n, sig, want) in cc.decode_cases().items():
        if cc.decode_with(wrong, sig, log_n) != want:
            told.append(name)
    for name, log_n, sig, cells in cc.refusal_cases():
        if cc.decode_with(wrong, sig, log_n) != cc.decode(sig, log_n)[0]:
            told.append(name)
    assert told, wrong.__name__
    if wrong is not cc.wrong_accepts_order_2n:                       # the other three are wrong on valid sigmas already, at every size but the smallest
        assert sum(1 for name in told if name in cc.decode_cases()) >= len(cc.decode_cases()) - 2, told


def test_refusal_cases_report_the_lowest_planted_cell():
    cases = cc.refusal_cases()
    assert len(cases) >= 5 * len(cc.refusal_cells())
    for name, log_n, sig, cells in cases:
        idx, bad = cc.decode(sig, log_n)
        n = 1 << log_n
        assert bad == min(cc.key(c, r) for c, r in cells), name
        assert [k for k, p in enumerate(idx) if p == cc.NOT_A_LABEL] == sorted(c * n + r for c, r in cells), name
        assert cc.report(sig, log_n)[:2] == (cc.KIND_NOT_A_LABEL, cc.cell_of_key(bad)), name


def test_model_reports_of_the_directed_circuits():
    q, sig, cols = cc.hand_built()
    assert cc.report(sig, cc.HAND_LOG_N, cols) == (cc.OK, None, None)
    bad = [list(c) for c in cols]
    bad[0][3] = 12345                                                # a[3] is tied to c[2]; c[2] has the lower key (row 2)
    assert cc.report(sig, cc.HAND_LOG_N, bad) == (cc.KIND_BROKEN, (2, 2), (0, 3))
    sig3, cols3 = cc.three_cycle()
    assert cc.report(sig3, cc.HAND_LOG_N, cols3) == (cc.KIND_BROKEN, (2, 4), (1, 6))
    sigb, colsb = cc.beyond_rows()
    assert cc.report(sigb, cc.HAND_LOG_N, colsb) == (cc.KIND_BROKEN, (0, 1), (3, 6))
    for log_n in (3, 8):
        kind, cell, image = cc.report(cc.shared_image_case(log_n), log_n)
        assert kind == cc.KIND_NOT_BIJECTIVE and image is None and cell is not None


# ---------------------------------------------------------------------------------- sigma_decode on the host
def _kat_cases():
    """[(log_n, value, expected packed cell)] for every log_n from 1 to 26"""
    rng = random.Random(2026)
    out = []
    for log_n in range(1, 27):
        w = pc.omega(log_n)
        for row in cc.label_rows(log_n, rng):
            for c in range(4):
                x = pc.NON_RESIDUES[c] * pow(w, row, pc.R_MOD) % pc.R_MOD
                want = cc.decode_value(x, log_n)
                assert want == cc.pack(c, row)
                out.append((log_n, x, want))
        for _, v in cc.non_labels(log_n, rng):
            out.append((log_n, v, cc.NOT_A_LABEL))
        if cc.decode_value(pc.R_MOD - 1, log_n) != cc.NOT_A_LABEL:     # r - 1 = omega^(N / 2): a label, decoded like one
            out.append((log_n, pc.R_MOD - 1, cc.pack(0, 1 << (log_n - 1))))
    return out


def _limbs(v):
    return cc.stored_int(v).to_bytes(32, "little")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_sigma_decode_on_the_host_at_every_log_n(tmp_path):
    exe = str(tmp_path / "sigma_decode_kat")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "plonkit_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "sigma_decode_kat.hip"), "-o", exe], stderr=subprocess.DEVNULL)
    cases = _kat_cases()
    assert {l for l, _, _ in cases} == set(range(1, 27))
    assert sum(1 for _, _, want in cases if want == cc.NOT_A_LABEL) >= 5 * 26
    blob = _limbs(pc.ROOT_2_28) + _limbs(pow(pc.ROOT_2_28, -1, pc.R_MOD)) + struct.pack("<I", len(cases))
    for log_n, v, _ in cases:
        blob += struct.pack("<I", log_n) + _limbs(v)
    (tmp_path / "cases.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d values decoded on the host" % len(cases) in r.stdout
    got = struct.unpack("<%dI" % len(cases), (tmp_path / "results.bin").read_bytes())
    wrong = [(log_n, hex(int(v)), hex(g), hex(want)) for (log_n, v, want), g in zip(cases, got) if g != want]
    assert not wrong, wrong[:5]
