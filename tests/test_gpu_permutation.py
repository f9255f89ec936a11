"""-m gpu: the copy-constraint permutation of the setup (plonkit_amd/csrc/perm.hip: the hand-written radix sort and k_perm_next; k_sigma_from_index
in poly.hip) against the plain model of tests/gen/perm_cases.py.

A setup with a wrong permutation still yields keys and proofs that agree with each other, so "the proof verifies" cannot see it; only a
comparison with an independent reference does.  plk_setup_permutation_dev runs the helper the setup itself calls, on a variable table of the
test's choosing: every case of perm_cases.py (pass counts 1 to 4 with ids that differ in one digit only, sizes from 8 positions to 16 tiles and
two scan blocks, hub variables across tiles and waves, the degenerate tables) once for the packed index and once for the sigma columns, exact.
Two whole setups through the existing API check that the setup hands the sort the right variable count: a circuit with one wire in thousands of
constraints against the oracle's key bytes, and the smallest domain whose ids need three passes against sigma_j(42) * G from the oracle's setup.
tests/test_perm_cases_host.py shows, without a GPU, that these cases tell a wrong sort or link from the right one."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import R_MOD
from tests.gen import perm_cases as pc
from tests.gen import round_cases as rc

PLK_ERR_ARG = 1


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


_UPLOADED = {}


def _vars(name):
    """the four id columns of a case on the device (uint32 bit patterns in int32 tensors), uploaded once"""
    import torch
    hit = _UPLOADED.get(name)
    if hit is None:
        cols = np.array(pc.case(name).cols, dtype=np.uint32)
        hit = _UPLOADED[name] = [torch.from_numpy(cols[j].view(np.int32).copy()).to("cuda:0") for j in range(4)]
        torch.cuda.synchronize()                                   # the library runs on its own stream
    return hit


def _run(ctx, name, index, sigmas):
    import torch
    c = pc.case(name)
    n = 1 << c.log_n
    d_idx = torch.full((4 * n,), -1, dtype=torch.int32, device="cuda:0") if index else None
    d_sig = [torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0") for _ in range(4)] if sigmas else None
    torch.cuda.synchronize()
    ctx.setup_permutation_dev(_vars(name), c.log_n, c.num_vars, d_idx, d_sig)
    return (d_idx.cpu().numpy().view(np.uint32) if index else None,
            [t.cpu().numpy().view(np.uint64) for t in d_sig] if sigmas else None)


def _check_index(name, got):
    want = np.array(pc.index_of(pc.case(name).nxt), dtype=np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d entries differ, the first at idx[%d]: %#x, want %#x" % (name, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


def _check_sigmas(name, got):
    c = pc.case(name)
    for j, want in enumerate(pc.sigmas_of(c.nxt, c.log_n)):
        assert np.array_equal(got[j], rc.to_array(want)), "%s: sigma column %d" % (name, j)


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_permutation_index(ctx, name):
    """idx[col * n + row] = col' << 30 | row' for every position, uint32 equality"""
    _check_index(name, _run(ctx, name, True, False)[0])


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_permutation_sigmas(ctx, name):
    """sigma_col[row] = k_col' * omega^row' as canonical Montgomery limbs, without the index being asked for"""
    _check_sigmas(name, _run(ctx, name, False, True)[1])


@pytest.mark.parametrize("name", pc.BOTH_OUTPUTS)
def test_permutation_index_and_sigmas_in_one_call(ctx, name):
    idx, sig = _run(ctx, name, True, True)
    _check_index(name, idx)
    _check_sigmas(name, sig)


def test_bad_arguments_are_refused(ctx):
    """null pointers, log_n above the largest setup, num_vars = 0, both outputs NULL: PLK_ERR_ARG, and the next call on the context is right"""
    import torch
    import plonkit_amd as pa
    name = "size/log_n=4"
    c, v = pc.case(name), _vars(name)
    idx = torch.zeros(4 << c.log_n, dtype=torch.int32, device="cuda:0")
    sig = [torch.zeros((1 << c.log_n, 4), dtype=torch.int64, device="cuda:0") for _ in range(4)]
    for what, args in (("a null column", ([v[0], v[1], 0, v[3]], c.log_n, c.num_vars, idx, sig)),
                       ("a null sigma column", (v, c.log_n, c.num_vars, idx, [sig[0], 0, sig[2], sig[3]])),
                       ("both outputs null", (v, c.log_n, c.num_vars, None, None)),
                       ("num_vars = 0", (v, c.log_n, 0, idx, sig)),
                       ("log_n = 27", (v, 27, c.num_vars, idx, sig)),
                       ("log_n = 29", (v, 29, c.num_vars, idx, sig)),
                       ("log_n = 2^32 - 2", (v, 0xFFFFFFFE, c.num_vars, idx, sig))):
        with pytest.raises(pa.PlkError) as e:
            ctx.setup_permutation_dev(*args)
        assert e.value.code == PLK_ERR_ARG, what
    L = pa.lib()
    import ctypes
    assert L.plk_setup_permutation_dev(None, None, ctypes.c_uint32(4), ctypes.c_uint64(2), None, None, None) == PLK_ERR_ARG
    assert L.plk_setup_permutation_dev(ctx._h, None, ctypes.c_uint32(4), ctypes.c_uint64(2), ctypes.c_void_p(idx.data_ptr()), None, None) == PLK_ERR_ARG
    _check_index(name, _run(ctx, name, True, False)[0])


# ------------------------------------------------------------------ whole setups through the existing API
HUB_WIRE, HUB_LINEAR, HUB_SQUARES = 2, 2200, 1000


def _hub_circuit():
    """wire 2 in every constraint: 2200 of hub * w_i = w_{i+1} (one gate each, the hub once) and 1000 of (a hub)(b hub) = c hub (one gate, the
    hub twice) -> 4200 occurrences in 3201 rows, domain 2^12.  Only the key is made: no witness."""
    rng = po.Xoshiro256ss(0x687562)
    cons = []
    for i in range(HUB_LINEAR):
        cons.append([{str(HUB_WIRE): str(rng.fr() or 1)}, {str(3 + i): str(rng.fr() or 1)}, {str(4 + i): str(rng.fr() or 1)}])
    for _ in range(HUB_SQUARES):
        cons.append([{str(HUB_WIRE): str(rng.fr() or 1)}, {str(HUB_WIRE): str(rng.fr() or 1)}, {str(HUB_WIRE): str(rng.fr() or 1)}])
    return {"nPubInputs": 1, "nOutputs": 0, "nVars": 4 + HUB_LINEAR, "constraints": cons}


def test_setup_of_a_hub_circuit_gives_the_oracles_key(ctx):
    """one wire in 3200 constraints: its cycle of more than 4096 occurrences crosses a tile of the sort, inside a whole plk_setup_prepare"""
    import plonkit_amd as pa
    js = _hub_circuit()
    assert sum(1 for con in js["constraints"] if any(str(HUB_WIRE) in lc for lc in con)) > 2048
    r_o = po.load_r1cs_json(js)
    T = po.transpile(r_o)
    rows, _, N = po._assemble(r_o, T)
    counts = {}
    for g in rows:
        for v in g.vars:
            counts[v] = counts.get(v, 0) + 1
    assert N <= 1 << 13 and counts[HUB_WIRE] > 4096, (N, counts[HUB_WIRE])
    S = po.setup(r_o, T)
    srs = ol.crs42(N)
    ctx.srs_upload(srs)
    ctx.srs_lagrange_clear()
    circ = pa.Circuit(json.dumps(js).encode(), True)                            # NULL witness
    setup = pa.SetupForProver(ctx, circ)
    try:
        assert setup.domain_size == N
        assert setup.verification_key_bytes(b"\x00" * 256) == po.write_vk(po.make_verification_key(S, po.Crs(srs, b"\x00" * 256)))
    finally:
        setup.close(); circ.close()


def test_setup_at_the_smallest_three_pass_domain(ctx):
    """Circuit.synthetic(2^17 - 2): more than 65536 variables, so the setup must hand the sort a count that needs three passes.  The four
    permutation commitments of its key equal sigma_j(42) * G with sigma_j from the oracle's setup of the exported .r1cs, evaluated by Horner
    in Python integers: four scalar multiplications on the host, no MSM."""
    import plonkit_amd as pa
    log_n = 17
    circ = pa.Circuit.synthetic((1 << log_n) - 2)
    rf = po.load_r1cs_flat(circ.export("r1cs"))
    V = po._rows_flat(rf)[0]
    assert json.loads(circ.analyse())["num_variables"] > 65536 and int(V.max()) >= 65536 and pc.passes(int(V.max()) + 1) == 3
    S = po.setup_flat(rf)
    assert S.N == 1 << log_n
    ctx.srs_generate(1 << log_n, 0, 42)
    ctx.srs_lagrange_clear()
    setup = pa.SetupForProver(ctx, circ)
    try:
        assert setup.domain_size == S.N
        vk = po.read_vk(setup.verification_key_bytes(pa.crs42_g2_bytes()))
    finally:
        setup.close(); circ.close()
    G = ol.g1_generator()
    for j in range(4):
        at_tau = 0
        for coeff in reversed(ol.fr_ints(S.sigmas[j])):
            at_tau = (at_tau * 42 + coeff) % R_MOD
        assert np.array_equal(vk.permutation_commitments[j], ol.g1_mul(G, at_tau)), "sigma_%d" % j
