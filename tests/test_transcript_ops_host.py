"""-m "not gpu": the host verifier under a caller-supplied transcript (plk_verify_with, plk_verify_terms_with; include/plonkit_amd.h
"a transcript of the CALLER's").  The independent pin is the oracle with its transcript substituted (tests/gen/alt_transcript.py): an
oracle proof of the golden circuit under the alt transcript, made on the CPU, must be accepted by the library under the same
transcript handed over as callbacks, and by nothing else."""
import os

import numpy as np
import pytest

import plonkit_amd as pa
from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import R_MOD
from tests.gen import alt_transcript as at

CALLBACK_OF = {"fr": "absorb_fr", "g1": "absorb_g1", "ch": "challenge"}


def _g(golden_dir, name):
    return open(os.path.join(golden_dir, name), "rb").read()


@pytest.fixture(scope="module")
def alt_proof(golden_dir, golden_crs):
    """(proof bytes, the oracle prover's call trace) of the golden circuit under the alt transcript; computed once"""
    r1cs = po.load_r1cs_json(os.path.join(golden_dir, "circuit.r1cs.json"))
    w = po.load_witness_json(os.path.join(golden_dir, "witness.json"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(po, "Transcript", at.AltOracle)
        mp.setattr(at.AltOracle, "trace", [])
        proof = po.write_proof(po.prove(r1cs, w, golden_crs))
        trace = list(at.AltOracle.trace)
    return proof, trace


def _tampered(data):
    """every tampering tests/test_oracle_golden.py applies to the golden proof"""
    P = po.read_proof(data)
    P.wire_values_at_z[1] = (P.wire_values_at_z[1] + 1) % R_MOD
    yield po.write_proof(P)
    P = po.read_proof(data)
    P.opening_at_z_proof = ol.g1_add(P.opening_at_z_proof, ol.g1_generator())
    yield po.write_proof(P)
    P = po.read_proof(data)
    P.inputs[0] = 36
    yield po.write_proof(P)


def test_keccak_through_the_callbacks_is_the_builtin_verifier(golden_dir):
    vk, proof = _g(golden_dir, "vk.bin"), _g(golden_dir, "proof.bin")
    ops = at.KeccakOps()
    assert pa.verify(vk, proof, transcript=ops)
    assert at.kinds(ops.trace) == at.VERIFIER_TRACE + ["end"]
    n = 0
    for bad in _tampered(proof):
        assert not pa.verify(vk, bad) and not pa.verify(vk, bad, transcript=at.KeccakOps())
        n += 1
    assert n == 3
    want = pa.verify_terms(vk, proof)
    got = pa.verify_terms(vk, proof, transcript=at.KeccakOps())
    assert want[2] and got[2]
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    for strict in (False, True):
        assert pa.verify(vk, proof, strict_inputs=strict, transcript=at.KeccakOps())


def test_the_oracle_proof_under_the_alt_transcript(golden_dir, alt_proof):
    vk, golden = _g(golden_dir, "vk.bin"), _g(golden_dir, "proof.bin")
    proof, prover_trace = alt_proof
    assert proof != golden and len(proof) == len(golden)
    assert at.kinds(prover_trace) == at.PROVER_TRACE
    with pytest.MonkeyPatch.context() as mp:                          # the oracle agrees with itself first
        mp.setattr(po, "Transcript", at.AltOracle)
        mp.setattr(at.AltOracle, "trace", [])
        assert po.verify(po.read_vk(vk), po.read_proof(proof))
        assert not po.verify(po.read_vk(vk), po.read_proof(golden))
        oracle_trace = list(at.AltOracle.trace[:30])
    assert not po.verify(po.read_vk(vk), po.read_proof(proof))        # Keccak again
    ops = at.AltOps()
    assert pa.verify(vk, proof, transcript=ops)
    # the recorded calls, with their argument values, are the oracle verifier's
    assert at.kinds(ops.trace) == at.VERIFIER_TRACE + ["end"]
    assert ops.trace[:-1] == oracle_trace
    assert ops.trace[:27] == prover_trace
    assert any(t[0] == "ch" and t[1] >> 253 for t in ops.trace[:-1]), "no challenge of this proof exercises the bits above 2^253"
    assert not pa.verify(vk, proof)
    assert not pa.verify(vk, golden, transcript=at.AltOps())
    for bad in _tampered(proof):
        assert not pa.verify(vk, bad, transcript=at.AltOps())
    # the flattened form under the alt transcript: the same two pairing arguments as the nested one accepts
    pts, sc, early = pa.verify_terms(vk, proof, transcript=at.AltOps())
    assert early
    acc = [None, None]
    for k in range(25):
        term = ol.g1_mul(pts[k], ol.fr_ints(sc[k:k + 1])[0])
        acc[k >= 23] = term if acc[k >= 23] is None else ol.g1_add(acc[k >= 23], term)
    raw = _g(golden_dir, "setup_2pow10.key")[-256:]
    assert pa.pairing_check(acc[0], raw[:128], acc[1], raw[128:])
    assert not pa.verify_terms(vk, golden, transcript=at.AltOps())[2]


@pytest.mark.parametrize("position", range(30))
def test_a_callback_that_fails(golden_dir, alt_proof, position):
    """position 0 is begin, 1..29 the absorbs and challenges of the verifier in order: an error that names the callback, the Python
    exception re-raised, end exactly once for a begin that succeeded, and the next call works"""
    vk, proof = _g(golden_dir, "vk.bin"), alt_proof[0]
    ops = at.AltOps(fail_begin=True) if position == 0 else at.AltOps(fail_at=position)
    with pytest.raises(at.TranscriptBoom):
        pa.verify(vk, proof, transcript=ops)
    words = pa.last_error()
    if position == 0:
        assert "the transcript's begin callback returned -1" in words
        assert ops.trace == []
    else:
        name = CALLBACK_OF[at.VERIFIER_TRACE[position]]
        assert "the transcript's %s callback (call %d after begin) returned -1" % (name, position) in words
        assert at.kinds(ops.trace) == at.VERIFIER_TRACE[:position] + ["end"]
    ops = at.AltOps(fail_begin=True) if position == 0 else at.AltOps(fail_at=position)
    with pytest.raises(at.TranscriptBoom):
        pa.verify_terms(vk, proof, transcript=ops)
    assert at.kinds(ops.trace).count("end") == (0 if position == 0 else 1)
    again = at.AltOps()
    assert pa.verify(vk, proof, transcript=again) and at.kinds(again.trace).count("end") == 1


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("value", [R_MOD, 2 ** 256 - 1])
def test_a_challenge_that_is_not_below_r_is_refused(golden_dir, alt_proof, which, value):
    vk, proof = _g(golden_dir, "vk.bin"), alt_proof[0]
    ops = at.AltOps(script={which: value.to_bytes(32, "little")})
    with pytest.raises(pa.PlkError) as e:
        pa.verify(vk, proof, transcript=ops)
    assert e.value.code == 1 and "not a canonical residue (limbs >= r)" in str(e.value)
    position = [i for i, k in enumerate(at.VERIFIER_TRACE) if k == "ch"][which]
    assert at.kinds(ops.trace) == at.VERIFIER_TRACE[:position + 1] + ["end"], "a callback ran after the refused challenge"
    # r - 1 is the largest value that passes: a verdict, not an error.  (The last challenge, u, only batches the two opening checks of
    # the verifier: a valid proof passes under any u.)
    ops = at.AltOps(script={which: R_MOD - 1})
    assert pa.verify(vk, proof, transcript=ops) is (which == 5)
    assert at.kinds(ops.trace).count("end") == 1


def test_challenges_in_the_domain_are_a_verdict(golden_dir, alt_proof):
    """z = 0 passes through the arithmetic, z = 1 and z = omega are z^N = 1: invalid, never an error, end once"""
    vk, proof = _g(golden_dir, "vk.bin"), alt_proof[0]
    for z in (0, 1, ol.omega(3)):
        ops = at.AltOps(script={3: z})
        assert pa.verify(vk, proof, transcript=ops) is False
        assert at.kinds(ops.trace).count("end") == 1
        assert pa.verify_terms(vk, proof, transcript=at.AltOps(script={3: z}))[2] is False


def test_a_malformed_proof_never_reaches_begin(golden_dir, alt_proof):
    vk, proof = _g(golden_dir, "vk.bin"), alt_proof[0]
    for bad_vk, bad_proof, words in ((vk, proof[:-1], "plk_verify: malformed proof"), (vk, proof + b"\x00", "plk_verify: malformed proof"),
                                     (vk[:-1], proof, "plk_verify: malformed verification key")):
        for call in (pa.verify, pa.verify_terms):
            ops = at.AltOps()
            with pytest.raises(pa.PlkError) as e:
                call(bad_vk, bad_proof, transcript=ops)
            assert e.value.code == 1 and words in str(e.value)
            assert ops.trace == []
    # a proof for another input count parses and is settled before the transcript starts
    P = po.read_proof(proof)
    P.inputs = P.inputs + [1]
    ops = at.AltOps()
    assert pa.verify(vk, po.write_proof(P), transcript=ops) is False and ops.trace == []


def test_a_table_with_a_hole_is_refused(golden_dir, alt_proof):
    import ctypes
    from plonkit_amd import _lib
    vk, proof = _g(golden_dir, "vk.bin"), alt_proof[0]
    table = _lib._TranscriptTable(at.AltOps())
    valid = ctypes.c_int32(7)

    def call():
        return pa.lib().plk_verify_with(vk, ctypes.c_uint64(len(vk)), proof, ctypes.c_uint64(len(proof)), ctypes.c_uint32(0),
                                        ctypes.byref(table.struct), ctypes.byref(valid))
    table.struct.flags = 2
    assert call() == 1 and "unknown flag" in pa.last_error()
    table.struct.flags = 1                                            # PLK_TRANSCRIPT_CONCURRENT means nothing to a single proof
    assert call() == 0 and valid.value == 1
    table.struct.flags = 0
    table.struct.end = _lib._TranscriptOpsStruct._END()
    assert call() == 1 and "null callback" in pa.last_error()
    # no table at all: exactly plk_verify_ex
    golden = _g(golden_dir, "proof.bin")
    assert pa.lib().plk_verify_with(vk, ctypes.c_uint64(len(vk)), golden, ctypes.c_uint64(len(golden)), ctypes.c_uint32(0), None,
                                    ctypes.byref(valid)) == 0 and valid.value == 1
