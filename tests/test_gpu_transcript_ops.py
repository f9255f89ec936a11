"""-m gpu: the prover and the batch verifier under a caller-supplied transcript (plk_ctx_set_transcript, plk_verify_many_with;
include/plonkit_amd.h "a transcript of the CALLER's").  The pin is the CPU oracle with its transcript substituted
(tests/gen/alt_transcript.py): under the alt transcript every proving entry point must give the oracle's bytes, with and without a
Lagrange-form key, and under Keccak routed through the callbacks the reference's golden proof."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import R_MOD
from tests.gen import alt_transcript as at

SHAPES = {"golden": 10, "chain5": 10, "chain300": 10, "chain3000": 13}      # log2 of the key each shape is proved against


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def _circuit_json(r1cs, n_pub):
    cons = []
    for A, B, C in r1cs.constraints:
        cons.append([{str(w): str(c) for w, c in lc} for lc in (A, B, C)])
    return json.dumps({"nPubInputs": n_pub, "nOutputs": 0, "nVars": r1cs.num_variables, "constraints": cons}).encode()


@pytest.fixture(scope="module")
def cases(golden_dir):
    """per shape: the circuit as the library loads it, and the ORACLE's proof under the alt transcript (CPU, computed once)"""
    import plonkit_amd as pa
    from tests.test_oracle_golden import _chain_circuit
    g2 = pa.crs42_g2_bytes()
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(po, "Transcript", at.AltOracle)
        for name, log_srs in SHAPES.items():
            if name == "golden":
                js = open(os.path.join(golden_dir, "circuit.r1cs.json"), "rb").read()
                wit = po.load_witness_json(os.path.join(golden_dir, "witness.json"))
            else:
                n_cons = int(name[5:])
                r1cs, wit = _chain_circuit(n_cons, 0x706c6f6e6b6974 + n_cons)
                js = _circuit_json(r1cs, 1)
            r_o = po.load_r1cs_json(json.loads(js))
            srs = ol.crs42(1 << log_srs)
            crs = po.Crs(srs, g2)
            S = po.setup(r_o)
            mp.setattr(at.AltOracle, "trace", [])
            P, dbg = po.prove(r_o, wit, crs, S, return_debug=True)
            trace = list(at.AltOracle.trace)
            mp.setattr(at.AltOracle, "trace", None)
            proof = po.write_proof(P)
            vk = po.write_vk(po.make_verification_key(S, crs))
            assert po.verify(po.read_vk(vk), po.read_proof(proof))                  # the substituted oracle accepts its own proof
            out[name] = dict(js=js, wit=wit, srs=srs, vk=vk, g2=g2, proof=proof, trace=trace, cols=dbg["w_vals"], N=S.N)
    for c in out.values():
        assert not po.verify(po.read_vk(c["vk"]), po.read_proof(c["proof"]))        # ... and Keccak does not
    return out


def _load(ctx, case):
    import plonkit_amd as pa
    ctx.srs_upload(case["srs"])
    ctx.srs_lagrange_clear()
    circ = pa.Circuit(case["js"], True, json.dumps([str(v) for v in case["wit"]]).encode(), True)
    return circ, pa.SetupForProver(ctx, circ)


@pytest.fixture()
def golden_setup(ctx, golden_dir, golden_crs):
    import plonkit_amd as pa
    ctx.set_transcript(None)
    ctx.srs_upload(golden_crs.g1)
    ctx.srs_lagrange_clear()
    circ = pa.Circuit.from_files(os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json"))
    setup = pa.SetupForProver(ctx, circ)
    yield circ, setup, open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    ctx.set_transcript(None)
    setup.close(); circ.close()


def test_keccak_through_the_callbacks_is_the_golden_proof(ctx, golden_setup):
    circ, setup, golden = golden_setup
    ops = at.KeccakOps()
    ctx.set_transcript(ops)
    assert setup.prove(circ) == golden
    assert at.kinds(ops.trace) == at.PROVER_TRACE + ["end"]
    ctx.set_transcript(None)
    assert setup.prove(circ) == golden
    assert len(ops.trace) == 28                                        # the table is no longer called


@pytest.mark.parametrize("lagrange", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_prove_under_the_alt_transcript_is_the_oracles_proof(ctx, cases, shape, lagrange):
    import torch
    import plonkit_amd as pa
    case = cases[shape]
    circ, setup = _load(ctx, case)
    assert setup.domain_size == case["N"]
    assert setup.verification_key_bytes(case["g2"]) == case["vk"]
    if lagrange:                                                       # the `-l` route: a, b, c, d and z are committed from their values
        lag = torch.zeros((case["N"], 8), dtype=torch.int64, device="cuda:0")
        ctx.g1_intt_srs_dev(case["N"].bit_length() - 1, lag.data_ptr())
        ctx.synchronize()
        ctx.srs_lagrange_set_dev(lag.data_ptr(), case["N"])
    ops = at.AltOps()
    ctx.set_transcript(ops)
    try:
        proof = setup.prove(circ)
    finally:
        ctx.set_transcript(None)
        ctx.srs_lagrange_clear()
    assert proof == case["proof"]
    assert ops.trace[:-1] == case["trace"] and ops.trace[-1] == ("end",)        # the calls and their argument values are the oracle's
    assert at.kinds(ops.trace) == at.PROVER_TRACE + ["end"]
    assert pa.verify(case["vk"], proof, transcript=at.AltOps())
    assert not pa.verify(case["vk"], proof)
    setup.close(); circ.close()


def test_every_proving_entry_point_takes_the_table(ctx, cases):
    import torch
    case = cases["chain300"]
    circ, setup = _load(ctx, case)
    w = ol.fr_vec(case["wit"])
    dev = torch.from_numpy(w.view(np.int64)).to("cuda:0")
    cols_dev = [torch.from_numpy(c.view(np.int64)).to("cuda:0") for c in case["cols"]]
    torch.cuda.synchronize()
    ctx.set_transcript(at.AltOps())
    try:
        assert setup.prove_witness(w) == case["proof"]
        assert setup.prove_witness_dev(dev, w.shape[0]) == case["proof"]
        assert setup.prove_wtns(circ.export("wtns")) == case["proof"]
        assert setup.prove_assembled(case["cols"]) == case["proof"]
        assert setup.prove_assembled_dev(cols_dev, case["N"]) == case["proof"]
        assert np.array_equal(ctx.prove_trace(0), ol.ntt(case["cols"][0], case["N"].bit_length() - 1, inverse=True))   # follows the last proof
    finally:
        ctx.set_transcript(None)
    setup.close(); circ.close()


@pytest.mark.parametrize("z,words", [(0, "challenge z = 0"), (1, "challenge z = 1"), ("omega", "challenge z^N = 1")])
def test_a_scripted_z_is_refused_and_the_context_goes_on(ctx, golden_setup, z, words):
    import plonkit_amd as pa
    circ, setup, golden = golden_setup
    ops = at.AltOps(script={3: ol.omega(3) if z == "omega" else z})
    ctx.set_transcript(ops)
    with pytest.raises(pa.PlkError) as e:
        setup.prove(circ)
    assert e.value.code == 5 and words in str(e.value)
    assert at.kinds(ops.trace) == at.PROVER_TRACE[:15] + ["end"]       # nothing after the refused challenge but end
    ctx.set_transcript(None)
    assert setup.prove(circ) == golden


@pytest.mark.parametrize("which", range(5))
def test_a_transcript_that_raises_or_overflows(ctx, golden_setup, which):
    """every challenge of the prover in turn: the Python exception comes back out of prove(), a challenge with limbs >= r is
    PLK_ERR_ARG, end is called once, and a Keccak proof on the same context is golden afterwards"""
    import plonkit_amd as pa
    circ, setup, golden = golden_setup
    position = [i for i, k in enumerate(at.PROVER_TRACE) if k == "ch"][which]
    ops = at.AltOps(script={which: at.TranscriptBoom("third challenge" if which == 2 else "challenge")})
    ctx.set_transcript(ops)
    with pytest.raises(at.TranscriptBoom):
        setup.prove(circ)
    assert at.kinds(ops.trace) == at.PROVER_TRACE[:position] + ["end"]
    assert "plk_prove: the transcript's challenge callback (call %d after begin) returned -1" % position in pa.last_error()
    ops = at.AltOps(script={which: (2 ** 256 - 1).to_bytes(32, "little")})
    ctx.set_transcript(ops)
    with pytest.raises(pa.PlkError) as e:
        setup.prove(circ)
    assert e.value.code == 1 and "limbs >= r" in str(e.value)
    assert at.kinds(ops.trace) == at.PROVER_TRACE[:position + 1] + ["end"]
    ctx.set_transcript(None)
    assert setup.prove(circ) == golden


def test_an_unsatisfied_witness_never_begins(ctx, cases):
    import plonkit_amd as pa
    case = cases["chain5"]
    circ, setup = _load(ctx, case)
    bad = list(case["wit"])
    bad[5] = (bad[5] + 1) % R_MOD
    circ_bad = pa.Circuit(case["js"], True, json.dumps([str(v) for v in bad]).encode(), True)
    ops = at.AltOps()
    ctx.set_transcript(ops)
    try:
        with pytest.raises(pa.PlkError) as e:
            setup.prove(circ_bad)
        assert e.value.code == 5 and at.kinds(ops.trace).count("begin") == at.kinds(ops.trace).count("end")
        assert setup.prove(circ) == case["proof"]
    finally:
        ctx.set_transcript(None)
    setup.close(); circ.close(); circ_bad.close()


def test_two_contexts_each_with_its_own_transcript(ctx, cases, golden_setup):
    import plonkit_amd as pa
    circ, setup, golden = golden_setup
    other = pa.Context(0)
    try:
        other.share_srs_from(ctx)
        other.set_transcript(at.AltOps())
        for _ in range(3):
            assert setup.prove(circ) == golden
            assert setup.prove(circ, ctx=other) == cases["golden"]["proof"]
    finally:
        other.close()


def test_verify_many_under_the_alt_transcript(ctx, cases, golden_setup):
    """a dozen proofs of one circuit: alt proofs, a tampered one, a Keccak proof, a truncated one"""
    import plonkit_amd as pa
    case = cases["chain300"]
    circ, setup = _load(ctx, case)
    ctx.set_transcript(at.AltOps())
    proofs = [case["proof"]]
    try:
        proofs += [setup.prove(circ) for _ in range(8)]
    finally:
        ctx.set_transcript(None)
    assert all(p == case["proof"] for p in proofs)
    keccak = setup.prove(circ)
    P = po.read_proof(case["proof"])
    P.wire_values_at_z[1] = (P.wire_values_at_z[1] + 1) % R_MOD
    batch = proofs[:4] + [po.write_proof(P)] + proofs[4:6] + [keccak] + proofs[6:] + [case["proof"][:-1]]
    assert len(batch) == 12
    want = [2 if k == 11 else int(pa.verify(case["vk"], p, transcript=at.AltOps())) for k, p in enumerate(batch)]
    assert want == [1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 2]
    key = pa.VerificationKey(ctx, case["vk"])
    ops = at.AltOps()
    got = key.verify_many(batch, transcript=ops)
    assert list(got) == want and key.first_bad == 4
    assert at.kinds(ops.trace).count("begin") == at.kinds(ops.trace).count("end") == 11
    got = key.verify_many(batch)                                       # no transcript: the Keccak verdicts of the same batch
    assert list(got) == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 2] and key.first_bad == 0
    with pytest.raises(at.TranscriptBoom):                             # a callback that fails inside the third proof ends the call
        key.verify_many(batch, transcript=_FailInProof(2))
    assert "proof 2: " in pa.last_error()
    assert list(key.verify_many(batch, transcript=at.AltOps())) == want
    key.close(); setup.close(); circ.close()


class _FailInProof(at.AltOps):
    """raises at the first challenge of the k-th begin"""

    def __init__(self, k):
        super().__init__()
        self.k, self.begun = k, 0

    def begin(self):
        self.trace.append(("begin",))
        script = {0: at.TranscriptBoom("scripted")} if self.begun == self.k else None
        self.begun += 1
        return at._State(self.core(), self.trace, script, None)
