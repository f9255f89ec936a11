"""-m gpu: the prover's round kernels (plonkit_amd/csrc/poly.hip) where their call-site bounds are tightest and their scans have seams.

tests/test_gpu_rounds.py draws every input from values below 2^252 and fixes one beta, gamma and z per case.  Here the direct entry points
(plk_permutation_grand_product_dev, plk_poly_evaluate_at_dev, plk_poly_divide_by_linear_dev, plk_lde4_coset_major_dev,
plk_icoset4_coset_major_dev) see the directed vectors and challenges of tests/gen/round_cases.py — stored residues r - 1, zeros that cross the
2048-element blocks of the scans, points z with z^2048 = 1 — bit-exact against that file's Python-integer model (itself held against the oracle
in tests/test_round_cases_host.py).  The grand-product and division entry points run the sequences of rounds 2 and 5 themselves (k_mul3_blocks
beyond one scan block; k_lincomb with one unit term and times_pow).  k_quotient, k_lincomb's products and the batched evaluation have no entry
point of their own: they are reached with
whole proofs of constant-column circuits (every selector and column r - 1, or 0) through plk_setup_from_polynomials and plk_prove_assembled,
with the oracle prover as the reference and plk_prove_trace localising a difference to a round."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol, plonk_oracle as po
from tests.gen import round_cases as rc
from tests.gen.round_cases import R_MOD

PLK_ERR_ARG, PLK_ERR_UNSAT = 1, 5


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


class _Uploads:
    """one conversion and one upload per distinct vector of a test (the combinations share their columns)"""

    def __init__(self):
        self.seen = {}

    def __call__(self, v):
        hit = self.seen.get(id(v))
        if hit is None:
            hit = self.seen[id(v)] = (v, _dev(rc.to_array(v)))
        return hit[1]


def _grand_product(ctx, up, w, sig, beta, gamma, log_n):
    import torch
    out = torch.full((1 << log_n, 4), -1, dtype=torch.int64, device="cuda:0")
    ctx.permutation_grand_product_dev([up(v) for v in w], [up(v) for v in sig], rc.to_limbs(beta), rc.to_limbs(gamma), log_n, out)
    return _host(out)


# -------------------------------------------------------------------------------- round 2: grand product
@pytest.mark.parametrize("log_n", rc.PRODUCT_LOG_N)
def test_grand_product_at_extreme_residues(ctx, log_n):
    """k_perm_terms ("limbs < 3 * 2^29 feed mulw's left side"), the pair of product scans and the closing product on wires and sigmas of stored
    r - 1, of 0, of residues next to r, of r - 1 alternating with 0 block by block and of all-ones 29-bit limbs, under beta, gamma from {0, 1, r - 1,
    r - 2, 2^253, stored r - 1, stored all-ones limbs, random}.  The entry point runs round 2's own sequence (grand_product, prover.hip):
    2^11 is one scan block exactly (the scans are complete, k_mul3), 2^12 two and 2^13 four (k_scan_totals_pair leaves the block prefixes and C_0
    behind, k_mul3_blocks folds the prefixes in).  Combinations with a vanishing denominator
    belong to test_a_vanished_denominator_is_refused; at least three quarters of the list must remain."""
    combos = rc.grand_product_combinations(log_n)
    up = _Uploads()
    kept = 0
    for name, w, sig, beta, gamma in combos:
        want, zero_den = rc.grand_product(w, sig, beta, gamma, log_n)
        if zero_den is not None:
            continue
        kept += 1
        if beta == 0:
            assert want == [1] * (1 << log_n)
        assert np.array_equal(_grand_product(ctx, up, w, sig, beta, gamma, log_n), rc.to_array(want)), name
    assert 4 * kept >= 3 * len(combos), (kept, len(combos))


@pytest.mark.parametrize("log_n", [12, 13])
def test_a_zero_numerator_crosses_the_scan_blocks(ctx, log_n):
    """gamma = -(w_0[i] + beta k_0 omega^i) makes the numerator of row i vanish: z_j = 0 for every j > i and z_j is unchanged up to i — at the
    first row, on both sides of the first block seam and at the last row (where nothing may change), on otherwise uniform inputs"""
    n = 1 << log_n
    w = [rc.uniform(n, 20 * log_n + j) for j in range(4)]
    sig = [rc.uniform(n, 200 * log_n + j) for j in range(4)]
    beta = rc.uniform(1, 3 * log_n)[0]
    up = _Uploads()
    free, _ = rc.grand_product(w, sig, beta, 0, log_n)
    for i in (0, rc.SCAN_BLOCK - 1, rc.SCAN_BLOCK, n - 1):
        gamma = -(w[0][i] + beta * rc.NON_RESIDUES[0] * pow(rc.omega(log_n), i, R_MOD)) % R_MOD
        want, zero_den = rc.grand_product(w, sig, beta, gamma, log_n)
        assert zero_den is None and all(want[:i + 1]) and not any(want[i + 1:]) and want != free
        assert np.array_equal(_grand_product(ctx, up, w, sig, beta, gamma, log_n), rc.to_array(want)), i


def test_grand_product_on_a_caller_stream(ctx):
    """2^12 (two scan blocks: C_0 comes back from the scans' totals in the context's scratch, the block prefixes are folded in by k_mul3_blocks)
    on a stream that is not the context's: the entry point is the only caller of round 2's sequence that brings its own stream"""
    import torch
    log_n = 12
    n = 1 << log_n
    w = [rc.uniform(n, 61 + j) for j in range(4)]
    sig = [rc.uniform(n, 71 + j) for j in range(4)]
    beta, gamma = rc.uniform(2, 81)
    want, zero_den = rc.grand_product(w, sig, beta, gamma, log_n)
    assert zero_den is None
    up = _Uploads()
    d_w, d_sig = [up(v) for v in w], [up(v) for v in sig]
    out = torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    stream.wait_stream(torch.cuda.current_stream())           # the uploads and the fill above
    ctx.permutation_grand_product_dev(d_w, d_sig, rc.to_limbs(beta), rc.to_limbs(gamma), log_n, out, stream=stream)
    stream.synchronize()
    assert np.array_equal(_host(out), rc.to_array(want))


def test_a_vanished_denominator_is_refused(ctx):
    """gamma = -(w_0[i] + beta sigma_0[i]): PLK_ERR_UNSAT naming the denominator (the output is not looked at), and the next call on the same
    context is right"""
    import plonkit_amd as pa
    log_n = 12
    n = 1 << log_n
    w = [rc.uniform(n, 31 + j) for j in range(4)]
    sig = [rc.uniform(n, 41 + j) for j in range(4)]
    beta = rc.uniform(1, 51)[0]
    up = _Uploads()
    for i in (0, rc.SCAN_BLOCK - 1, rc.SCAN_BLOCK, n - 1):
        gamma = -(w[0][i] + beta * sig[0][i]) % R_MOD
        assert rc.grand_product(w, sig, beta, gamma, log_n) == (None, i)
        with pytest.raises(pa.PlkError) as e:
            _grand_product(ctx, up, w, sig, beta, gamma, log_n)
        assert e.value.code == PLK_ERR_UNSAT and "denominator vanished" in str(e.value), str(e.value)
        want, zero_den = rc.grand_product(w, sig, beta, (gamma + 1) % R_MOD, log_n)
        assert zero_den is None
        assert np.array_equal(_grand_product(ctx, up, w, sig, beta, (gamma + 1) % R_MOD, log_n), rc.to_array(want)), i


# ----------------------------------------------------------------- rounds 4 and 5: evaluation, division
def _evaluate(ctx, d, n, z):
    return rc.from_array(ctx.poly_evaluate_at_dev(d, n, rc.to_limbs(z)).reshape(1, 4))[0]


def _divide(ctx, d, n, z):
    import torch
    q = torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0")
    ctx.poly_divide_by_linear_dev(d, n, rc.to_limbs(z), q)
    return _host(q)


@pytest.mark.parametrize("n", [1, 2, 8, 2047, 2048, 2049, 4096, (1 << 17) + 1])
def test_evaluation_and_division_at_directed_coefficients_and_points(ctx, n):
    """k_eval_partial (Horner on raw sums, then x^start per thread and block), and round 5's division chain (divide_by_linear, prover.hip) on one
    polynomial with the coefficient one — k_lincomb with its times_pow branch, the suffix sum scan and k_div_finish: every directed
    vector at every point of {1, r - 1, 2, 1/2, omega_n, omega_2048, a generator of the 2^28 subgroup, r - 2, random} up to 4096 coefficients, one
    point per vector in turn at 2^17 + 1 (65 blocks); z = 0 gives c_0 for the evaluation and PLK_ERR_ARG for the division"""
    import plonkit_amd as pa
    points = rc.eval_points(n, n)
    for k, (vname, p) in enumerate(rc.directed_vectors(n, seed=n)):
        d = _dev(rc.to_array(p))
        chosen = points if n <= 4096 else [points[k % len(points)]]
        for zname, z in chosen:
            assert _evaluate(ctx, d, n, z) == rc.poly_eval(p, z), (vname, zname)
            assert np.array_equal(_divide(ctx, d, n, z), rc.to_array(rc.poly_div_linear(p, z))), (vname, zname)
        assert _evaluate(ctx, d, n, 0) == p[0], vname
        with pytest.raises(pa.PlkError) as e:
            _divide(ctx, d, n, 0)
        assert e.value.code == PLK_ERR_ARG, str(e.value)
    assert n <= 4096 or k + 1 >= len(points)               # every point was used


def test_evaluation_and_division_beyond_one_block_total_per_lane(ctx):
    """n = 2^21 + 2049: 1026 scan blocks, so the 1024 lanes of k_scan_totals take per = 2 totals each and the last lanes are clamped (lo > nb).
    The reference is the oracle here (the Python model would take a minute); the identity (x - z) q(x) + p(z) = p(x) at a second point does not
    depend on the oracle's own division."""
    n = (1 << 21) + 2049
    top = ol.int_to_limbs(R_MOD - 1)
    alt = np.zeros((n, 4), dtype=np.uint64)
    alt[(np.arange(n) // rc.SCAN_BLOCK) % 2 == 0] = top                       # stored r - 1 and 0, block by block
    near = rc.to_array(rc.near_r(1 << 12, 21))
    near = np.ascontiguousarray(np.tile(near, (n // near.shape[0] + 1, 1))[:n])
    y = 0x55aa55aa55aa55aa
    for vname, p, z in (("alternation", alt, rc.omega(11)), ("near r", near, rc.uniform(1, 2121)[0])):
        d = _dev(p)
        pz = ol.poly_eval(p, z)
        assert _evaluate(ctx, d, n, z) == pz, vname
        q = _divide(ctx, d, n, z)
        assert np.array_equal(q, ol.poly_div_linear(p, z)), vname
        assert ((y - z) * ol.poly_eval(q, y) + pz) % R_MOD == ol.poly_eval(p, y), vname


# ------------------------------------------------------------------------- round 3: the coset transforms
LDE_VECTORS = ("stored_r_minus_1", "zero", "stored_r_minus_1_alt_zero_stride_1", "near_r")


@pytest.mark.parametrize("log_n", [1, 3, 10, 11, 12])
def test_coset_major_transforms_at_extreme_residues(ctx, log_n):
    """lde4cm_batch_dev, icoset4cm_dev and k_icoset_combine on stored r - 1, 0, r - 1 alternating with 0 and residues next to r, against the
    oracle's coset NTT at 4n put into / taken out of coset-major order by the model's permutation; the inverse returns canonical residues"""
    import torch
    n = 1 << log_n
    polys = [rc.to_array(rc.directed(n, name, seed=log_n)) for name in LDE_VECTORS]
    d_out = [torch.full((4 * n, 4), -1, dtype=torch.int64, device="cuda:0") for _ in polys]
    ctx.lde4_coset_major_dev([_dev(a) for a in polys], log_n, d_out)
    ctx.synchronize()
    for name, a, d in zip(LDE_VECTORS, polys, d_out):
        ext = np.zeros((4 * n, 4), dtype=np.uint64)
        ext[:n] = a
        assert np.array_equal(_host(d), rc.to_coset_major(ol.ntt(ext, log_n + 2, coset=rc.COSET_GEN), n)), name
    for name in LDE_VECTORS:
        cm = rc.to_array(rc.directed(4 * n, name, seed=log_n))                # 4n values in coset-major order
        d = _dev(cm)
        ctx.icoset4_coset_major_dev(d, log_n)
        ctx.synchronize()
        got = _host(d)
        assert all(s < R_MOD for s in rc.stored_ints(got)), name
        assert np.array_equal(got, ol.ntt(rc.from_coset_major(cm, n), log_n + 2, inverse=True, coset=rc.COSET_GEN)), name


# --------------------------------------------------- rounds 1 to 5: whole proofs from constant columns
_FIRST_OF_SIZE = {case[0]: case for case in reversed(rc.CIRCUIT_CASES)}
TRACE = [("w_coef", 0, "round 1: wire polynomial a"), ("w_coef", 1, "round 1: wire polynomial b"), ("w_coef", 2, "round 1: wire polynomial c"),
         ("w_coef", 3, "round 1: wire polynomial d"), ("z_coef", None, "round 2: grand product polynomial"),
         ("t_coef", None, "round 3: quotient polynomial (4N coefficients)"), ("r", None, "round 4: linearisation polynomial"),
         ("W_z", None, "round 5: opening quotient at z"), ("W_zw", None, "round 5: opening quotient at z * omega")]


@pytest.mark.parametrize("case", rc.CIRCUIT_CASES, ids=rc.circuit_id)
def test_constant_column_circuits_match_the_oracle_prover(ctx, case):
    """A constant column is a constant polynomial, so its extension to the 4N coset is that constant at every point: with every selector and
    column r - 1 (or 0) k_quotient's gate sums, k_lincomb's selector terms and the batched evaluations run on one extreme value throughout,
    and a shuffled sigma keeps the grand product and the permutation half of the quotient non-trivial.  vk and proof bytes and all nine
    vectors between the rounds equal the oracle's; 8 public inputs is the last count of the quotient's in-kernel path, 9 the first extended one."""
    import plonkit_amd as pa
    c, S, crs, P, dbg = rc.oracle_setup_and_proof(case)
    crs = po.Crs(crs.g1, pa.crs42_g2_bytes())               # the G2 pair of the same tau = 42 key: the verifier needs a real one
    want_vk, want_proof = po.write_vk(po.make_verification_key(S, crs)), po.write_proof(P)
    ctx.srs_upload(crs.g1)
    ctx.srs_lagrange_clear()
    for values in (True, False) if _FIRST_OF_SIZE[case[0]] is case else (True,):
        sel, sig = (S.selector_values, S.sigma_values) if values else (S.selectors, S.sigmas)
        setup = pa.SetupForProver.from_polynomials(ctx, S.n, S.num_inputs, sel[:6], sel[6], sig, values=values)
        try:
            assert setup.verification_key_bytes(crs.g2_raw) == want_vk, "values=%s" % values
            proof = setup.prove_assembled(dbg["w_vals"])
            for key, j, what in TRACE:
                want = dbg[key] if j is None else dbg[key][j]
                assert np.array_equal(ctx.prove_trace(TRACE.index((key, j, what))), want), what
            assert proof == want_proof, "values=%s" % values
            assert pa.verify(want_vk, proof)
        finally:
            setup.close()
    if not any(case[1]):                                    # the all-zero circuit: every wire commitment is the point at infinity
        at = 16 + 32 * case[2]
        assert struct.unpack_from(">Q", proof, at)[0] == 4
        assert proof[at + 8:at + 8 + 4 * 64] == (b"\x40" + b"\x00" * 63) * 4
