"""-m gpu: which copy constraint is broken (plonkit_amd/csrc/copycheck.hip, sigma_decode_dev.h) against the plain model of
tests/gen/copy_cases.py: plk_sigma_decode_dev against the kernel it inverts (plk_setup_permutation_dev) and against planted non-labels,
plk_setup_check_permutation on sigmas that are no bijection, plk_check_copies / _dev on hand-built circuits and on a prepared setup, and the
suffix plk_prove_assembled appends to its "copy constraints" message.  All comparisons are exact integers.
tests/test_copy_cases_host.py shows, without a GPU, that the model inverts the forward rule, that the cases tell wrong decoders from the right
one, and runs the per-value decode on the CPU at every log_n up to 26 (here: up to 16)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol, plonk_oracle as po
from tests.gen import copy_cases as cc
from tests.gen import perm_cases as pc

PLK_ERR_ARG, PLK_ERR_UNSAT = 1, 5
OLD_MESSAGE = ("copy constraints: the permutation argument does not close (prod of numerators != prod of denominators at beta, gamma): "
               "the columns break the copy constraints of the setup's sigma")


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    c.srs_generate(1 << 10, 0, 42)
    c.srs_lagrange_clear()
    yield c
    c.close()


def _dev(arr):
    """a host array on the device, complete before the library's own stream reads it"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _sig_dev(sig):
    return [_dev(cc.to_array(col).view(np.int64)) for col in sig]


def _decode(ctx, sig_tensors, log_n, **kw):
    idx, bad = ctx.sigma_decode_dev(sig_tensors, log_n, **kw)
    return idx.cpu().numpy().view(np.uint32), bad


def _roundtrip(ctx, case):
    """variable table -> index and sigmas (the setup's kernels) -> decode of the sigmas == the index, and == the model's"""
    import torch
    n = 1 << case.log_n
    cols = np.array(case.cols, dtype=np.uint32)
    v = [_dev(cols[j].view(np.int32)) for j in range(4)]
    d_idx = torch.full((4 * n,), -1, dtype=torch.int32, device="cuda:0")
    d_sig = [torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    ctx.setup_permutation_dev(v, case.log_n, case.num_vars, d_idx, d_sig)
    want = d_idx.cpu().numpy().view(np.uint32)
    got, bad = _decode(ctx, d_sig, case.log_n)
    assert bad is None, case.name
    assert np.array_equal(got, want), case.name
    assert np.array_equal(got, np.array(pc.index_of(case.nxt), dtype=np.uint32)), case.name


# ------------------------------------------------------------------ decode against the kernel it inverts
@pytest.mark.parametrize("log_n", cc.DIRECT_LOG_N)
def test_decode_inverts_the_setup_permutation(ctx, log_n):
    _roundtrip(ctx, cc.table(log_n))


ABOVE_2_POW_12 = ("size/log_n=13", "size/log_n=14", "hub/a_and_b_columns")      # (named here so that collecting the tests builds no case)


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n not in ABOVE_2_POW_12])
def test_decode_inverts_the_permutation_cases(ctx, name):
    """every case of perm_cases.py up to 2^12, and the single cycle over all cells at 2^14"""
    c = pc.case(name)
    assert c.log_n <= 12 or name == "hub/one_id_everywhere"
    _roundtrip(ctx, c)


def test_the_cases_left_out_are_the_ones_above_2_pow_12():
    assert tuple(n for n in pc.CASE_NAMES if n not in cc.perm_case_names()) == ABOVE_2_POW_12
    assert all(pc.case(n).log_n > 12 for n in ABOVE_2_POW_12)


def test_decode_at_2_pow_16(ctx):
    _roundtrip(ctx, cc.table(cc.LARGE_LOG_N))


# ------------------------------------------------------------------------------------------------ refusals
def test_planted_non_labels_are_refused_where_they_are(ctx):
    """every non-label of the host list at (a, 0), (d, N - 1), both sides of a block seam and of a wave seam, and two at once: the lowest
    key comes back and idx is 0xFFFFFFFF exactly there"""
    cases = cc.refusal_cases()
    assert {name.split(" at ")[0] for name, _, _, _ in cases} >= {"zero", "omega_2N", "r, not canonical", "a label + r, not canonical"}
    for name, log_n, sig, cells in cases:
        want, want_bad = cc.decode(sig, log_n)
        got, bad = _decode(ctx, _sig_dev(sig), log_n)
        assert bad == want_bad == min(cc.key(c, r) for c, r in cells), name
        assert np.array_equal(got, np.array(want, dtype=np.uint32)), name
        assert sorted(np.nonzero(got == 0xFFFFFFFF)[0]) == sorted(c * (1 << log_n) + r for c, r in cells), name


def test_decode_bad_arguments(ctx):
    import ctypes
    import plonkit_amd as pa
    sig = _sig_dev(cc.decode_cases()["copy/log_n=3"][1])
    for log_n in (0, 27, 28, 0xFFFFFFFF):
        with pytest.raises(pa.PlkError) as e:
            ctx.sigma_decode_dev(sig, log_n)
        assert e.value.code == PLK_ERR_ARG
    L = pa.lib()
    idx = _dev(np.zeros(32, dtype=np.int32))
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in sig])
    holed = (ctypes.c_void_p * 4)(sig[0].data_ptr(), None, sig[2].data_ptr(), sig[3].data_ptr())
    for log_n in (0, 27, 0xFFFFFFFF):
        assert L.plk_sigma_decode_dev(ctx._h, ptrs, ctypes.c_uint32(log_n), ctypes.c_void_p(idx.data_ptr()), None, None) == PLK_ERR_ARG
    assert L.plk_sigma_decode_dev(None, ptrs, ctypes.c_uint32(3), ctypes.c_void_p(idx.data_ptr()), None, None) == PLK_ERR_ARG
    assert L.plk_sigma_decode_dev(ctx._h, None, ctypes.c_uint32(3), ctypes.c_void_p(idx.data_ptr()), None, None) == PLK_ERR_ARG
    assert L.plk_sigma_decode_dev(ctx._h, holed, ctypes.c_uint32(3), ctypes.c_void_p(idx.data_ptr()), None, None) == PLK_ERR_ARG
    assert L.plk_sigma_decode_dev(ctx._h, ptrs, ctypes.c_uint32(3), None, None, None) == PLK_ERR_ARG
    # bad_key may be NULL, and the context is fine afterwards
    assert L.plk_sigma_decode_dev(ctx._h, ptrs, ctypes.c_uint32(3), ctypes.c_void_p(idx.data_ptr()), None, None) == 0
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), np.array(cc.decode_cases()["copy/log_n=3"][2], dtype=np.uint32))


# ----------------------------------------------------------------- setups with a sigma of the test's choosing
def _setup(ctx, sig, log_n, q=None):
    """a resident setup from value-form vectors: sigma as given (canonical integers), selectors all zero unless given; one public input
    (with zero selectors row 0 then reads 0 + a[0] = 0: all-zero columns satisfy every gate)"""
    import plonkit_amd as pa
    n = 1 << log_n
    sel = [ol.fr_vec(v) for v in (q or [[0] * n] * 7)]
    return pa.SetupForProver.from_polynomials(ctx, n - 1, 1, sel[:6], sel[6], [cc.to_array(col) for col in sig], values=True)


def _report(rep):
    return (rep.kind, rep.cell, rep.image)


def _cols(columns):
    return [cc.to_array(c) for c in columns]


@pytest.mark.parametrize("log_n", [3, 8])
def test_two_cells_sharing_an_image_is_not_bijective(ctx, log_n):
    import plonkit_amd as pa
    sig = cc.shared_image_case(log_n)
    want = cc.report(sig, log_n)
    assert want[0] == cc.KIND_NOT_BIJECTIVE == pa.COPY_NOT_BIJECTIVE
    setup = _setup(ctx, sig, log_n)
    try:
        assert _report(setup.check_permutation()) == want
        zeros = [[0] * (1 << log_n)] * 4
        assert _report(setup.check_copies(_cols(zeros))) == want               # kind 2 wins over the copies
        if log_n == 3:                                                          # all-zero columns satisfy the empty gates; sigma does not close
            with pytest.raises(pa.PlkError) as e:
                setup.prove_assembled(_cols(zeros))
            assert e.value.code == PLK_ERR_UNSAT
            assert str(e.value).endswith(OLD_MESSAGE + "; sigma is not a permutation: cell %s[%d] is the image of no cell" % ("abcd"[want[1][0]], want[1][1]))
    finally:
        setup.close()


def test_a_canonical_non_label_in_a_setup(ctx):
    import plonkit_amd as pa
    log_n = 3
    base = cc.decode_cases()["copy/log_n=3"][1]
    for cell, v in (((3, 2), 0), ((0, 7), pc.omega(log_n + 1))):
        sig = [list(col) for col in base]
        sig[cell[0]][cell[1]] = v
        want = cc.report(sig, log_n)
        assert want == (cc.KIND_NOT_A_LABEL, cell, None)
        setup = _setup(ctx, sig, log_n)
        try:
            assert _report(setup.check_permutation()) == want
            with pytest.raises(pa.PlkError) as e:
                setup.prove_assembled(_cols([[0] * 8] * 4))
            assert e.value.code == PLK_ERR_UNSAT
            assert str(e.value).endswith(OLD_MESSAGE + "; sigma is not a permutation: its value at cell %s[%d] is not a cell label" % ("abcd"[cell[0]], cell[1]))
        finally:
            setup.close()


# -------------------------------------------------------------------------------------------------- copies
def test_hand_built_circuit_and_its_broken_cell(ctx):
    import plonkit_amd as pa
    q, sig, cols = cc.hand_built()
    setup = _setup(ctx, sig, cc.HAND_LOG_N, q)
    try:
        assert _report(setup.check_permutation()) == (pa.COPY_OK, None, None)
        assert _report(setup.check_copies(_cols(cols))) == (pa.COPY_OK, None, None)
        proof = setup.prove_assembled(_cols(cols))                               # the rebuilt circuit is the one of the assembled tests
        assert pa.verify(setup.verification_key_bytes(pa.crs42_g2_bytes()), proof)
        bad = [list(c) for c in cols]
        bad[0][3] = 12345                                                        # the cell only the permutation looks at
        want = cc.report(sig, cc.HAND_LOG_N, bad)
        assert want == (cc.KIND_BROKEN, (2, 2), (0, 3))
        rep = setup.check_copies(_cols(bad))
        assert isinstance(rep, pa.CopyReport) and _report(rep) == want
        with pytest.raises(pa.PlkError) as e:
            setup.prove_assembled(_cols(bad))
        assert e.value.code == PLK_ERR_UNSAT
        assert str(e.value).endswith(OLD_MESSAGE + "; first broken copy: cell c[2] and its image a[3] hold different values")
        assert setup.prove_assembled(_cols(cols)) == proof                       # and the context proves on
    finally:
        setup.close()


def test_a_cycle_of_three_names_the_lowest_cell(ctx):
    sig, cols = cc.three_cycle()
    want = cc.report(sig, cc.HAND_LOG_N, cols)
    assert want == (cc.KIND_BROKEN, (2, 4), (1, 6))
    setup = _setup(ctx, sig, cc.HAND_LOG_N)
    try:
        assert _report(setup.check_copies(_cols(cols))) == want
    finally:
        setup.close()


def test_a_break_in_the_zero_extension(ctx):
    sig, cols = cc.beyond_rows()
    assert len(cols[0]) == 3
    want = cc.report(sig, cc.HAND_LOG_N, cols)
    assert want == (cc.KIND_BROKEN, (0, 1), (3, 6))
    setup = _setup(ctx, sig, cc.HAND_LOG_N)
    try:
        assert _report(setup.check_copies(_cols(cols))) == want
        cols[0][1] = 0                                                           # equal to the zeros beyond `rows`
        assert _report(setup.check_copies(_cols(cols))) == (cc.OK, None, None)
    finally:
        setup.close()


def test_check_copies_refuses_what_prove_assembled_refuses(ctx):
    import plonkit_amd as pa
    q, sig, cols = cc.hand_built()
    setup = _setup(ctx, sig, cc.HAND_LOG_N, q)
    try:
        arr = _cols(cols)
        arr[1][2] = ol.int_to_limbs(pc.R_MOD)
        with pytest.raises(pa.PlkError) as e:
            setup.check_copies(arr)
        assert e.value.code == PLK_ERR_ARG and "column b" in str(e.value)
        for rows in (0, 9):                                                      # rows < num_inputs = 1, rows > N
            with pytest.raises(pa.PlkError) as e:
                setup.check_copies([np.zeros((rows, 4), dtype=np.uint64)] * 4)
            assert e.value.code == PLK_ERR_ARG
        assert _report(setup.check_copies(_cols(cols))) == (pa.COPY_OK, None, None)
    finally:
        setup.close()


@pytest.fixture(scope="module")
def prepared(ctx):
    """a plk_setup_prepare setup of a synthetic circuit at 2^10, the columns of its own proof, and the oracle's sigma of the same circuit"""
    import plonkit_amd as pa
    log_n = 10
    circ = pa.Circuit.synthetic((1 << log_n) - 2)
    setup = pa.SetupForProver(ctx, circ)
    assert setup.domain_size == 1 << log_n
    setup.prove(circ)
    cols = [ctx.ntt(ctx.prove_trace(j), log_n) for j in range(4)]
    S = po.setup_flat(po.load_r1cs_flat(circ.export("r1cs")))
    sig = [ol.fr_ints(v) for v in S.sigma_values]
    yield dict(log_n=log_n, setup=setup, cols=cols, sig=sig, values=[ol.fr_ints(c) for c in cols])
    setup.close(); circ.close()


def _flip_last_tied_cell(prepared):
    """the columns with one cell changed: the tied cell (sigma moves it) of the highest row"""
    log_n, n = prepared["log_n"], 1 << prepared["log_n"]
    idx, bad = cc.decode(prepared["sig"], log_n)
    assert bad is None
    col, row = max(((c, r) for c in range(4) for r in range(n) if idx[c * n + r] != cc.pack(c, r)), key=lambda cr: (cr[1], cr[0]))
    values = [list(v) for v in prepared["values"]]
    values[col][row] = (values[col][row] + 1) % pc.R_MOD
    want = cc.report(prepared["sig"], log_n, values)
    assert want[0] == cc.KIND_BROKEN and (col, row) in (want[1], want[2])
    cols = [c.copy() for c in prepared["cols"]]
    cols[col][row] = ol.fr_mont(values[col][row])
    return cols, want


def test_prepared_setup_with_its_own_columns(ctx, prepared):
    import plonkit_amd as pa
    setup = prepared["setup"]
    assert cc.report(prepared["sig"], prepared["log_n"], prepared["values"]) == (cc.OK, None, None)
    assert _report(setup.check_permutation()) == (pa.COPY_OK, None, None)
    assert _report(setup.check_copies(prepared["cols"])) == (pa.COPY_OK, None, None)
    cols, want = _flip_last_tied_cell(prepared)
    assert _report(setup.check_copies(cols)) == want


def test_device_columns_on_a_non_default_stream(ctx, prepared):
    import torch
    import plonkit_amd as pa
    setup = prepared["setup"]
    bad_cols, want = _flip_last_tied_cell(prepared)
    rows = (1 << prepared["log_n"]) - 1                                          # the last row is padding: zero-extended by the call
    assert all(not c[rows:].any() for c in prepared["cols"])
    s = torch.cuda.Stream()
    for cols, verdict in ((prepared["cols"], (pa.COPY_OK, None, None)), (bad_cols, want)):
        with torch.cuda.stream(s):
            # produced on s: the call must be ordered behind the stream's work (a copy, then an in-place product by one)
            dev = [torch.from_numpy(np.ascontiguousarray(c[:rows]).view(np.int64)).to("cuda:0", non_blocking=True) for c in cols]
            for t in dev:
                t.mul_(1)
        assert _report(setup.check_copies_dev(dev, stream=s)) == verdict
        assert _report(setup.check_copies_dev(dev)) == verdict                   # NULL stream: the context's own (s is idle now)
    with pytest.raises(ValueError):
        setup.check_copies_dev(dev[:3])
