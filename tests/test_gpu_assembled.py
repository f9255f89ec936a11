"""-m gpu: proofs from setup polynomials and assembled wire columns (plk_setup_from_polynomials, plk_prove_assembled,
plk_prove_assembled_dev) — the level plonkit itself works at: bellman's SetupPolynomials (src/plonk.rs:50-55,104) and the circuit
bellman has synthesised (prove_by_steps, src/plonk.rs:152-159).  Verification key and proof bytes against the reference's golden
files and the oracle, against plk_prove on the same circuit, and every refusal the header documents."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NON_RESIDUES = (1, 5, 7, 10)


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden(golden_dir, golden_crs):
    """the oracle's setup of the reference's `simple` circuit and its prover assembly (w_vals = the columns a, b, c, d)"""
    r1cs = po.load_r1cs_json(os.path.join(golden_dir, "circuit.r1cs.json"))
    wit = po.load_witness_json(os.path.join(golden_dir, "witness.json"))
    S = po.setup(r1cs)
    P, dbg = po.prove(r1cs, wit, golden_crs, S, return_debug=True)
    vk = open(os.path.join(golden_dir, "vk.bin"), "rb").read()
    proof = open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    assert po.write_proof(P) == proof
    return dict(S=S, cols=dbg["w_vals"], w_coef=dbg["w_coef"], vk=vk, proof=proof, r1cs=r1cs, wit=wit)


def _from_setup(ctx, S, values):
    import plonkit_amd as pa
    sel, sig = (S.selector_values, S.sigma_values) if values else (S.selectors, S.sigmas)
    return pa.SetupForProver.from_polynomials(ctx, S.n, S.num_inputs, sel[:6], sel[6], sig, values=values)


def _expect(code, fn, *args, **kw):
    import plonkit_amd as pa
    with pytest.raises(pa.PlkError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("values", [False, True])
def test_golden_vk_and_proof_from_polynomials(ctx, golden, golden_crs, values):
    ctx.srs_upload(golden_crs.g1)
    ctx.srs_lagrange_clear()
    setup = _from_setup(ctx, golden["S"], values)
    assert setup.domain_size == golden["S"].N
    assert setup.verification_key_bytes(golden_crs.g2_raw) == golden["vk"]
    assert setup.upload(ctx) is setup                                   # a resident setup: upload is a no-op
    assert setup.prove_assembled(golden["cols"]) == golden["proof"]
    # columns shorter than the domain are zero-extended (the oracle's rows beyond the circuit are padding)
    n_real = 1 + max(r for r in range(golden["S"].N) if any(c[r].any() for c in golden["cols"]))
    assert n_real < golden["S"].N
    assert setup.prove_assembled([c[:n_real] for c in golden["cols"]]) == golden["proof"]
    # the tracing hooks describe an assembled proof as any other
    assert set(setup.timings_ms()) >= {"witness", "round1", "round2", "round3", "round4", "round5"}
    for j in range(4):
        assert np.array_equal(ctx.prove_trace(j), golden["w_coef"][j])
    setup.close()


def test_assembled_proof_on_a_prepared_setup_and_verification(ctx, golden, golden_dir, golden_crs):
    import plonkit_amd as pa
    ctx.srs_upload(golden_crs.g1)
    circ = pa.Circuit.from_files(os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json"))
    setup = pa.SetupForProver(ctx, circ)
    assert setup.prove_assembled(golden["cols"]) == golden["proof"] == setup.prove(circ)
    assert pa.verify(golden["vk"], golden["proof"])
    setup.close(); circ.close()


def _chain(n_cons, seed):
    from tests.test_oracle_golden import _chain_circuit
    return _chain_circuit(n_cons, seed)


def _circuit_json(r1cs, n_pub):
    cons = []
    for A, B, C in r1cs.constraints:
        cons.append([{str(w): str(c) for w, c in lc} for lc in (A, B, C)])
    return json.dumps({"nPubInputs": n_pub, "nOutputs": 0, "nVars": r1cs.num_variables, "constraints": cons}).encode()


@pytest.mark.parametrize("n_cons,log_srs", [(5, 10), (300, 10), (3000, 13), (40000, 17)])
def test_synthetic_chain_circuits_match_the_oracle(ctx, n_cons, log_srs):
    """the constraint counts of test_synthetic_prove_matches_oracle (domains 2^3 .. 2^17): vk and proof bytes equal the oracle's,
    from coefficient-form and value-form setups alike"""
    r1cs, wit = _chain(n_cons, 0x706c6f6e6b6974 + n_cons)
    r_o = po.load_r1cs_json(json.loads(_circuit_json(r1cs, 1)))
    srs = ol.crs42(1 << log_srs)
    crs = po.Crs(srs, b"\x00" * 256)
    ctx.srs_upload(srs)
    ctx.srs_lagrange_clear()
    S = po.setup(r_o)
    P, dbg = po.prove(r_o, wit, crs, S, return_debug=True)
    want_vk, want_proof = po.write_vk(po.make_verification_key(S, crs)), po.write_proof(P)
    for values in (False, True):
        setup = _from_setup(ctx, S, values)
        assert setup.verification_key_bytes(b"\x00" * 256) == want_vk
        assert setup.prove_assembled(dbg["w_vals"]) == want_proof
        setup.close()


def _columns_from_trace(ctx, log_n):
    """the wire values of the last proof on ctx: prove_trace(0..3) are the coefficients, one forward NTT each"""
    return [ctx.ntt(ctx.prove_trace(j), log_n) for j in range(4)]


@pytest.mark.parametrize("lc_terms,log_n", [(5, 10), (9, 14), (12, 16)])
def test_dense_circuits_match_plk_prove(ctx, lc_terms, log_n):
    """Poseidon-shaped dense bodies (d, q_d_next and all 11 commitments live): plk_prove_assembled on a plk_setup_prepare setup with
    the columns of plk_prove's own proof gives plk_prove's bytes; up to 2^14 they are also the oracle's"""
    import plonkit_amd as pa
    n = 1 << log_n
    ctx.srs_generate(n, 0, 42)
    ctx.srs_lagrange_clear()
    circ = pa.Circuit.synthetic_ex(n - 2, lc_terms=lc_terms)
    setup = pa.SetupForProver(ctx, circ)
    assert setup.domain_size == n
    want = setup.prove(circ)
    cols = _columns_from_trace(ctx, log_n)
    assert setup.prove_assembled(cols) == want
    if log_n <= 14:
        rf, wf = po.load_r1cs_flat(circ.export("r1cs")), ol.wtns_parse(circ.export("wtns"))
        crs = po.Crs(ctx.srs_download(0, n), pa.crs42_g2_bytes())
        S = po.setup_flat(rf)
        assert want == po.write_proof(po.prove(rf, wf, crs, S))
        poly = _from_setup(ctx, S, values=False)
        assert poly.verification_key_bytes(pa.crs42_g2_bytes()) == setup.verification_key_bytes(pa.crs42_g2_bytes())
        assert poly.prove_assembled(cols) == want
        poly.close()
    setup.close(); circ.close()


def test_lagrange_form_key_gives_the_same_bytes(ctx):
    import torch
    import plonkit_amd as pa
    log_n = 12
    n = 1 << log_n
    ctx.srs_generate(n, 0, 42)
    ctx.srs_lagrange_clear()
    circ = pa.Circuit.synthetic(n - 2)
    setup = pa.SetupForProver(ctx, circ)
    want = setup.prove(circ)
    cols = _columns_from_trace(ctx, log_n)
    assert setup.prove_assembled(cols) == want
    lag = torch.zeros((n, 8), dtype=torch.int64, device="cuda:0")
    ctx.g1_intt_srs_dev(log_n, lag.data_ptr())
    ctx.synchronize()
    ctx.srs_lagrange_set_dev(lag.data_ptr(), n)
    try:
        assert setup.prove_assembled(cols) == want
    finally:
        ctx.srs_lagrange_clear()
    setup.close(); circ.close()


def test_device_columns_on_a_non_default_stream(ctx):
    import torch
    import plonkit_amd as pa
    log_n = 16
    n = 1 << log_n
    ctx.srs_generate(n, 0, 42)
    ctx.srs_lagrange_clear()
    circ = pa.Circuit.synthetic_ex(n - 2, lc_terms=6)
    setup = pa.SetupForProver(ctx, circ)
    want = setup.prove(circ)
    cols = _columns_from_trace(ctx, log_n)
    assert setup.prove_assembled(cols) == want
    rows = n - 1                                                        # the last row is padding: zero-extended by the call
    assert all(not c[rows:].any() for c in cols)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # produced on s: the call must wait for the stream's work (a copy, then an in-place product by one) before it reads
        dev = [torch.from_numpy(np.ascontiguousarray(c[:rows]).view(np.int64)).to("cuda:0", non_blocking=True) for c in cols]
        for t in dev:
            t.mul_(1)
    got = setup.prove_assembled_dev([t for t in dev], rows, stream=s)
    assert got == want
    assert setup.prove_assembled_dev([t.data_ptr() for t in dev], rows) == want    # NULL stream: the context's own (s is idle now)
    setup.close(); circ.close()


def _hand_built():
    """N = 8, one public input.  Rows: 0 public input x (q_a = -1); 1 x * y = xy (q_m = 1, q_c = -1); 2 xy + y = s (q_a = q_b = 1,
    q_c = -1); 3 selectors all zero, a = s; 4..7 empty.  Copy cycles: x (0a, 1a), y (1b, 2b), xy (1c, 2a), s (2c, 3a) — the cell 3a is
    tied to 2c by the permutation alone, no gate looks at it.  sigma from those cycles with k = 1, 5, 7, 10."""
    N, log_n = 8, 3
    x, y = 3, 11
    m1 = R_MOD - 1
    q = [[0] * N for _ in range(7)]                                     # q_a q_b q_c q_d q_m q_const q_d_next
    q[0][0] = m1
    q[4][1], q[2][1] = 1, m1
    q[0][2], q[1][2], q[2][2] = 1, 1, m1
    vals = [[0] * N for _ in range(4)]
    vals[0][0] = x
    vals[0][1], vals[1][1], vals[2][1] = x, y, x * y % R_MOD
    vals[0][2], vals[1][2], vals[2][2] = x * y % R_MOD, y, (x * y + y) % R_MOD
    vals[0][3] = (x * y + y) % R_MOD
    w = ol.omega(log_n)
    dom = [pow(w, i, R_MOD) for i in range(N)]
    sig = [[NON_RESIDUES[j] * dom[r] % R_MOD for r in range(N)] for j in range(4)]
    for (j1, r1), (j2, r2) in [((0, 0), (0, 1)), ((1, 1), (1, 2)), ((2, 1), (0, 2)), ((2, 2), (0, 3))]:
        sig[j1][r1] = NON_RESIDUES[j2] * dom[r2] % R_MOD
        sig[j2][r2] = NON_RESIDUES[j1] * dom[r1] % R_MOD
    return N, [ol.fr_vec(v) for v in q], [ol.fr_vec(v) for v in sig], [ol.fr_vec(v) for v in vals]


def test_copy_constraints_are_enforced(ctx, golden_crs):
    import plonkit_amd as pa
    N, q, sig, cols = _hand_built()
    ctx.srs_upload(golden_crs.g1)
    ctx.srs_lagrange_clear()
    setup = pa.SetupForProver.from_polynomials(ctx, N - 1, 1, q[:6], q[6], sig, values=True)
    vk = setup.verification_key_bytes(golden_crs.g2_raw)
    proof = setup.prove_assembled(cols)
    assert pa.verify(vk, proof)                                          # the hand-built sigma is right
    assert po.verify(po.read_vk(vk), po.read_proof(proof))
    assert po.read_proof(proof).inputs == [3]
    bad = [c.copy() for c in cols]
    bad[0][3] = ol.fr_mont(12345)                                        # the cell only the permutation looks at
    assert ol.check_gates(np.stack(bad), np.stack(q), N, 1)             # every gate still holds ...
    msg = _expect(5, setup.prove_assembled, bad)                        # ... the copy constraint does not
    assert "copy constraints" in msg
    setup.close()


def test_gate_violation_names_the_lowest_failing_row(ctx, golden, golden_crs):
    import plonkit_amd as pa
    N, q, sig, cols = _hand_built()
    ctx.srs_upload(golden_crs.g1)
    ctx.srs_lagrange_clear()
    setup = pa.SetupForProver.from_polynomials(ctx, N - 1, 1, q[:6], q[6], sig, values=True)
    bad = [c.copy() for c in cols]
    bad[2][1] = ol.fr_mont(7)                                            # c of the multiplication gate
    msg = _expect(5, setup.prove_assembled, bad)
    assert "must satisfy" in msg and "row 1 " in msg
    bad[1][2] = ol.fr_mont(8)                                            # and b of the addition gate: row 1 is still the lowest
    assert "row 1 " in _expect(5, setup.prove_assembled, bad)
    setup.close()
    # the golden circuit: flip c of the last gate row whose q_c is non-zero
    S = golden["S"]
    setup = _from_setup(ctx, S, values=False)
    qc = ol.fr_ints(S.selector_values[2])
    r = max(i for i in range(S.num_inputs, S.N) if qc[i])
    bad = [c.copy() for c in golden["cols"]]
    bad[2][r] = ol.fr_mont(ol.fr_ints(bad[2][r:r + 1])[0] + 1)
    assert ("row %d " % r) in _expect(5, setup.prove_assembled, bad)
    assert setup.prove_assembled(golden["cols"]) == golden["proof"]     # and the context is fine afterwards
    setup.close()


def test_argument_errors(ctx, golden, golden_dir, golden_crs):
    import plonkit_amd as pa
    S = golden["S"]
    N = S.N
    ctx.srs_upload(golden_crs.g1)
    ctx.srs_lagrange_clear()
    sel, sig = S.selectors, S.sigmas
    mk = pa.SetupForProver.from_polynomials
    # N = n + 1 not a power of two; a domain whose 4N exceeds 2^28
    assert "setup power of two" in _expect(2, mk, ctx, N - 2, S.num_inputs, sel[:6], sel[6], sig)
    assert "setup power of two" in _expect(2, mk, ctx, (1 << 27) - 1, 1, sel[:6], sel[6], sig)
    # len > N (coefficient form), len < N (value form)
    pad = lambda v: np.concatenate([v, np.zeros((1, 4), dtype=np.uint64)])
    _expect(1, mk, ctx, S.n, S.num_inputs, [pad(v) for v in sel[:6]], pad(sel[6]), [pad(v) for v in sig])
    sv, gv = S.selector_values, S.sigma_values
    _expect(1, mk, ctx, S.n, S.num_inputs, [v[:-1] for v in sv[:6]], sv[6][:-1], [v[:-1] for v in gv], values=True)
    # num_inputs > n
    _expect(1, mk, ctx, S.n, N, sel[:6], sel[6], sig)
    # a non-canonical selector element (r itself, and all ones), in both forms
    for form, base in ((False, (sel, sig)), (True, (sv, gv))):
        for limbs in (ol.int_to_limbs(R_MOD), np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)):
            q = [v.copy() for v in base[0]]
            q[4][1] = limbs
            assert "q_m" in _expect(1, mk, ctx, S.n, S.num_inputs, q[:6], q[6], base[1], values=form)
    s2 = [v.copy() for v in sig]
    s2[3][0] = ol.int_to_limbs(R_MOD)
    assert "sigma_4" in _expect(1, mk, ctx, S.n, S.num_inputs, sel[:6], sel[6], s2)
    setup = _from_setup(ctx, S, values=False)
    cols = golden["cols"]
    # rows < num_inputs, rows > N
    assert S.num_inputs >= 1
    _expect(1, setup.prove_assembled, [c[:S.num_inputs - 1] for c in cols])
    _expect(1, setup.prove_assembled, [pad(c) for c in cols])
    # a non-canonical column element
    bad = [c.copy() for c in cols]
    bad[1][2] = ol.int_to_limbs(R_MOD)
    assert "column b" in _expect(1, setup.prove_assembled, bad)
    # a key that is too small
    ctx.srs_upload(golden_crs.g1[:N // 2])
    _expect(3, setup.prove_assembled, cols)
    ctx.srs_upload(golden_crs.g1)
    # plk_prove on a setup built from polynomials: no gate structure
    circ = pa.Circuit.from_files(os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json"))
    assert "plk_prove_assembled" in _expect(1, setup.prove, circ)
    assert setup.prove_assembled(cols) == golden["proof"]
    setup.close(); circ.close()


def test_a_c_program_proves_through_the_c_abi_alone(golden, golden_crs, tmp_path):
    """tests/host/assembled_prover.c: reads the golden circuit's setup polynomials and columns as raw files, calls only the C ABI
    (plk_setup_from_polynomials, plk_setup_write_vk, plk_prove_assembled) and writes vk and proof: the reference's golden bytes"""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not on PATH")
    S = golden["S"]
    exe = str(tmp_path / "assembled_prover")
    libdir = os.path.join(ROOT, "plonkit_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "assembled_prover.c"), "-o", exe, "-L", libdir, "-lplonkit_amd",
                           "-Wl,-rpath," + libdir])
    d = tmp_path / "in"
    d.mkdir()
    names = ["q_a", "q_b", "q_c", "q_d", "q_m", "q_const", "q_d_next", "sigma_1", "sigma_2", "sigma_3", "sigma_4"]
    for name, v in zip(names, S.selectors + S.sigmas):
        (d / name).write_bytes(np.ascontiguousarray(v, dtype=np.uint64).tobytes())
    for j, c in enumerate(golden["cols"]):
        (d / ("column_" + "abcd"[j])).write_bytes(np.ascontiguousarray(c, dtype=np.uint64).tobytes())
    (d / "key_points").write_bytes(np.ascontiguousarray(golden_crs.g1[:S.N], dtype=np.uint64).tobytes())
    (d / "key_g2").write_bytes(golden_crs.g2_raw)
    r = subprocess.run([exe, str(d), str(S.n), str(S.num_inputs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert (d / "vk.bin").read_bytes() == golden["vk"]
    assert (d / "proof.bin").read_bytes() == golden["proof"]
