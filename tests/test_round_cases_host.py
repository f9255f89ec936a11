"""No GPU: the integer model of tests/gen/round_cases.py against the oracle's vector operations on random inputs, and every constant-column
circuit of its builder through the oracle alone (gate check, proof, verification).  Two independent references agree here before either judges
a kernel in tests/test_gpu_round_edges.py."""
import numpy as np
import pytest

from oracle import oracle_lib as ol, plonk_oracle as po
from tests.gen import round_cases as rc


def test_constants_and_conversions():
    assert rc.R_MOD == ol.R_MOD and rc.NON_RESIDUES == po.NON_RESIDUES and rc.COSET_GEN == po.COSET_GEN
    for log_n in range(rc.TWO_ADICITY + 1):
        assert rc.omega(log_n) == ol.omega(log_n)
    assert pow(rc.ROOT_2_28, 1 << 27, rc.R_MOD) == rc.R_MOD - 1
    xs = rc.uniform(64, 5) + [0, 1, rc.R_MOD - 1, rc.stored(rc.R_MOD - 1)]
    a = rc.to_array(xs)
    assert np.array_equal(a, ol.fr_vec(xs)) and rc.from_array(a) == xs == ol.fr_ints(a)
    assert rc.stored_ints(rc.to_array([rc.stored(rc.R_MOD - 1)])) == [rc.R_MOD - 1]
    with pytest.raises(AssertionError):
        rc.from_array(np.array([ol.int_to_limbs(rc.R_MOD)]))


@pytest.mark.parametrize("log_n", [3, 11])
def test_grand_product_model_against_the_oracle(log_n):
    n = 1 << log_n
    w = [rc.uniform(n, 10 * log_n + j) for j in range(4)]
    sig = [rc.uniform(n, 100 * log_n + j) for j in range(4)]
    beta, gamma = rc.uniform(2, 7 + log_n)
    z, zero_den = rc.grand_product(w, sig, beta, gamma, log_n)
    assert zero_den is None
    wa, sa = [rc.to_array(v) for v in w], [rc.to_array(v) for v in sig]
    dom = ol.vpowers(ol.omega(log_n), n)
    num = den = None
    for j in range(4):
        nj = ol.vadd_scalar(ol.vaxpy(wa[j], beta * rc.NON_RESIDUES[j] % rc.R_MOD, dom), gamma)
        dj = ol.vadd_scalar(ol.vaxpy(wa[j], beta, sa[j]), gamma)
        num = nj if num is None else ol.vmul(num, nj)
        den = dj if den is None else ol.vmul(den, dj)
    assert np.array_equal(rc.to_array(z), ol.vshifted_prefix_product(ol.vmul(num, ol.vbatch_inv(den))))
    # a vanished denominator is reported with its row, the last row included
    for row in (0, n - 1):
        g0 = -(w[0][row] + beta * sig[0][row]) % rc.R_MOD
        assert rc.grand_product(w, sig, beta, g0, log_n) == (None, row)
    # a vanished numerator: zero from the next row on, nothing changes before
    row = n // 2
    g0 = -(w[0][row] + beta * rc.NON_RESIDUES[0] * pow(rc.omega(log_n), row, rc.R_MOD)) % rc.R_MOD
    z0, zero_den = rc.grand_product(w, sig, beta, g0, log_n)
    assert zero_den is None and all(v != 0 for v in z0[:row + 1]) and all(v == 0 for v in z0[row + 1:])


@pytest.mark.parametrize("n", [1, 2, 8, 2048])
def test_evaluation_and_division_model_against_the_oracle(n):
    p = rc.uniform(n, n)
    pa = rc.to_array(p)
    for name, z in rc.eval_points(n, n) + [("0", 0)]:
        assert rc.poly_eval(p, z) == ol.poly_eval(pa, z), name
        q = rc.poly_div_linear(p, z)
        assert len(q) == n and q[-1] == 0
        assert np.array_equal(rc.to_array(q), ol.poly_div_linear(pa, z)), name
    assert rc.poly_eval(p, 0) == p[0]
    names = dict(rc.eval_points(n, n))
    assert pow(names["omega_2048"], 2048, rc.R_MOD) == 1 and pow(names["omega_n"], 1 << max(n - 1, 0).bit_length(), rc.R_MOD) == 1


def test_directed_vectors_and_combinations():
    n = 4096
    vs = dict(rc.directed_vectors(n))
    top = rc.stored(rc.R_MOD - 1)
    assert rc.stored_ints(rc.to_array(vs["stored_r_minus_1"][:2])) == [rc.R_MOD - 1] * 2
    assert vs["minus_one"][0] == rc.R_MOD - 1 and vs["one"][-1] == 1 and not any(vs["zero"])
    assert vs["stored_r_minus_1_alt_zero_stride_1"][:3] == [top, 0, top]
    blk = vs["stored_r_minus_1_alt_zero_stride_2048"]
    assert blk[2047] == top and blk[2048] == 0 and blk[4095] == 0
    assert all(rc.R_MOD - (1 << 16) <= s < rc.R_MOD for s in rc.stored_ints(rc.to_array(vs["near_r"][:64])))
    ones = rc.stored_ints(rc.to_array(vs["stored_limbs_all_ones"][:1]))[0]
    assert ones < rc.R_MOD and all((ones >> (29 * i)) & 0x1fffffff == 0x1fffffff for i in range(8))
    for at in (0, 2047, 2048, 4095):
        v = vs["single_at_%d" % at]
        assert v[at] == top and sum(1 for x in v if x) == 1
    assert max(vs["uniform"]) >> 252                       # beyond what 62-bit limbs with a 60-bit top limb reach
    assert [k for k, _ in rc.directed_vectors(8)].count("single_at_7") == 1 and "single_at_2047" not in dict(rc.directed_vectors(8))
    perm = rc.coset_major_index(4)
    assert perm.tolist() == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
    nat = np.arange(16)
    assert np.array_equal(rc.from_coset_major(rc.to_coset_major(nat, 4), 4), nat)
    # the pruning floor of the grand-product test, checked with the model at the small sizes here (all sizes on the GPU box)
    for log_n in (1, 3):
        combos = rc.grand_product_combinations(log_n)
        kept = [c for c in combos if rc.grand_product(c[1], c[2], c[3], c[4], log_n)[1] is None]
        assert 4 * len(kept) >= 3 * len(combos)
        assert any(c[3] == 0 for c in kept) and any(c[3] == c[4] == rc.R_MOD - 1 for c in kept) and any(c[3] == 1 and c[4] == 0 for c in kept)


@pytest.mark.parametrize("case", rc.CIRCUIT_CASES, ids=rc.circuit_id)
def test_constant_circuits_prove_and_verify_through_the_oracle(case):
    c, S, crs, P, dbg = rc.oracle_setup_and_proof(case)
    n = c["N"]
    assert ol.check_gates(np.stack(dbg["w_vals"]), np.stack(S.selector_values), n, c["num_inputs"])
    assert P.inputs == c["inputs"] and len(P.inputs) == case[2]
    assert po.verify(po.make_verification_key(S, crs), P)
    assert po.verify(po.read_vk(po.write_vk(po.make_verification_key(S, crs))), po.read_proof(po.write_proof(P)))
    z = ol.fr_ints(dbg["z_vals"])
    if any(case[1]):
        assert len(set(z)) > 1, "a constant grand product would leave the permutation half of the quotient trivial"
        assert any(ol.fr_ints(dbg["t_coef"])), "a zero quotient"
    else:
        assert all(ol.g1_is_inf(p) for p in P.wire_commitments)
