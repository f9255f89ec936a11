"""-m gpu: one setup, a stream of witnesses.  The .wtns payload is decoded and range-checked by a kernel (wtnsio.hip), and
plk_prove_witness / _witness_dev / _wtns prove a witness that arrives without its circuit.  Referees: Python integers for the kernels
(v * 2^256 mod r), the reference's golden proof.bin, and plk_prove on a circuit object that holds the same witness."""
import ctypes
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import R_MOD

ERR_ARG, ERR_UNSAT, ERR_FORMAT = 1, 5, 6
HEAD = 76                                                # bytes of a .wtns file in front of its elements
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def mont(values):
    """Python integers -> the (n, 4) uint64 Montgomery limbs the library must produce: v * 2^256 mod r"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = v * (1 << 256) % R_MOD
        out[i] = [(m >> (64 * k)) & MASK for k in range(4)]
    return out


def le_bytes(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def wtns_file(values):
    return (b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, 40) + struct.pack("<I", 32) + po.BN254_PRIME_LE
            + struct.pack("<I", len(values)) + struct.pack("<IQ", 2, 32 * len(values)) + le_bytes(values))


def to_dev_bytes(raw):
    import torch
    return torch.from_numpy(np.frombuffer(bytearray(raw), dtype=np.uint8)).to("cuda:0")


def to_dev_fr(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def known_values(n, seed):
    special = [0, 1, 2, R_MOD - 1, (1 << 256) % R_MOD, (R_MOD - 1) // 2]
    rng = po.Xoshiro256ss(seed)
    return (special + [rng.fr() for _ in range(n)])[:n] if n >= len(special) else [special[(seed + i) % len(special)] for i in range(n)]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_decode_and_encode_known_answers(ctx, n):
    """one lane per element, 256 lanes per block, no grid-stride loop: the sizes straddle a wave and a block"""
    import torch
    vals = known_values(n, 100 + n)
    if n == 1:
        vals = [R_MOD - 1]
    raw = le_bytes(vals)
    src = to_dev_bytes(raw)
    out = torch.full((n + 1, 4), -1, dtype=torch.int64, device="cuda:0")           # one element of guard behind the output
    ctx.fr_decode_dev(src, n, out)
    got = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:n], mont(vals))
    assert (got[n] == MASK).all(), "the kernel wrote behind its output"
    back = torch.full((32 * n + 32,), 0x55, dtype=torch.uint8, device="cuda:0")
    ctx.fr_encode_dev(out, n, back)
    ctx.synchronize()
    b = back.cpu().numpy().tobytes()
    assert b[:32 * n] == raw and b[32 * n:] == b"\x55" * 32
    # the file decoder gives the same elements from the payload's unaligned place in the file
    out2 = torch.zeros((n, 4), dtype=torch.int64, device="cuda:0")
    assert ctx.wtns_decode(wtns_file(vals), out2, n) == (n, None)
    assert np.array_equal(out2.cpu().numpy().view(np.uint64), mont(vals))


def test_alignment_and_capacity_are_checked(ctx):
    import torch
    import plonkit_amd as pa
    src = torch.zeros(32 * 4 + 64, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros((6, 4), dtype=torch.int64, device="cuda:0")
    for a, b in ((src.data_ptr() + 8, out.data_ptr()), (src.data_ptr(), out.data_ptr() + 8), (src.data_ptr() + 76, out.data_ptr())):
        with pytest.raises(pa.PlkError) as e:
            ctx.fr_decode_dev(a, 4, b)
        assert e.value.code == ERR_ARG
        with pytest.raises(pa.PlkError) as e:
            ctx.fr_encode_dev(b, 4, a)
        assert e.value.code == ERR_ARG
    vals = known_values(6, 3)
    assert ctx.wtns_decode(wtns_file(vals), None, 0) == (6, None)
    with pytest.raises(pa.PlkError) as e:
        ctx.wtns_decode(wtns_file(vals), out, 5)
    assert e.value.code == ERR_ARG
    with pytest.raises(pa.PlkError) as e:
        ctx.wtns_decode(wtns_file(vals), out.data_ptr() + 8, 6)
    assert e.value.code == ERR_ARG
    # non-canonical Montgomery limbs are encoded after one reduction: r + 5 (as limbs) is the Montgomery form of 5 / R
    v = R_MOD + 5
    limbs = np.array([[(v >> (64 * k)) & MASK for k in range(4)]], dtype=np.uint64)
    back = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    ctx.fr_encode_dev(to_dev_fr(limbs), 1, back)
    ctx.synchronize()
    assert int.from_bytes(back.cpu().numpy().tobytes(), "little") == 5 * pow(1 << 256, -1, R_MOD) % R_MOD


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("where", [(130,), (40, 200), (0,), (299,), (0, 299), (63, 64, 256)])
def test_refused_elements(ctx, where):
    import torch
    import plonkit_amd as pa
    n = 300
    refused = [R_MOD, R_MOD + 1, (1 << 256) - 1, 1 << 254]
    vals = known_values(n, 7)
    for k, i in enumerate(where):
        vals[i] = refused[(k + len(where)) % 4]
    want = mont([0 if i in where else v for i, v in enumerate(vals)])
    for through_file in (False, True):
        out = torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0")
        with pytest.raises(pa.PlkError) as e:
            if through_file:
                ctx.wtns_decode(wtns_file(vals), out, n)
            else:
                ctx.fr_decode_dev(to_dev_bytes(le_bytes(vals)), n, out)
        assert e.value.code == ERR_FORMAT and "read witness failed: not in field" in str(e.value)
        assert e.value.bad_index == min(where)
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want), "zero at the refused indices, every other element right"
    for bad in refused:                                  # each refused value on its own, and its neighbour r - 1 accepted
        out = torch.zeros((2, 4), dtype=torch.int64, device="cuda:0")
        with pytest.raises(pa.PlkError) as e:
            ctx.fr_decode_dev(to_dev_bytes(le_bytes([R_MOD - 1, bad])), 2, out)
        assert e.value.code == ERR_FORMAT and e.value.bad_index == 1
        assert np.array_equal(out.cpu().numpy().view(np.uint64), mont([R_MOD - 1, 0]))


# ------------------------------------------------------------------------------------------------ 3
def test_golden_proof_three_ways(ctx, golden_dir, golden_crs):
    import plonkit_amd as pa
    ctx.srs_load_key(open(os.path.join(golden_dir, "setup_2pow10.key"), "rb").read())
    ctx.srs_lagrange_clear()
    circ = pa.Circuit.from_files(os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json"))
    wt = circ.export("wtns")
    setup = pa.SetupForProver(ctx, circ)
    circ.close()                                         # nothing of the circuit object is needed from here on
    want = open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    assert setup.prove_wtns(wt) == want
    t = setup.timings_ms()
    assert list(t) == ["witness", "round1", "round2", "round3", "round4", "round5", "serialise"]
    assert ctx.prove_trace(0).shape == (8, 4) and ctx.prove_trace(5).shape == (32, 4)
    w = ol.fr_vec(po.parse_wtns(wt))
    assert setup.prove_witness(w) == want
    dev = to_dev_fr(w)
    assert setup.prove_witness_dev(dev, w.shape[0]) == want
    assert setup.validate_witness_dev(dev, w.shape[0]) == (True, None)
    extra = np.concatenate([w, ol.fr_vec([5, 6])])       # extra elements are ignored
    assert setup.prove_witness(extra) == want and setup.prove_wtns(wtns_file(po.parse_wtns(wt) + [5, 6])) == want
    setup.close()


# ------------------------------------------------------------------------------------------------ 4
class Stream:
    """one R1CS, three witnesses: the setup, the .wtns bytes and the proofs plk_prove makes of the circuit objects"""

    def __init__(self, ctx, gates, lc_terms, seed, lagrange):
        import torch
        import plonkit_amd as pa
        self.circs = [pa.Circuit.synthetic_ex(gates, seed, ws, lc_terms) for ws in (1, 2, 3)]
        self.r1cs = self.circs[0].export("r1cs")
        assert all(c.export("r1cs") == self.r1cs for c in self.circs)
        self.n = self.circs[0].domain_size()
        ctx.srs_generate(self.n, 0, 42)
        ctx.srs_lagrange_clear()
        self.lag = None
        if lagrange:
            self.lag = torch.zeros((self.n, 8), dtype=torch.int64, device="cuda:0")
            ctx.g1_intt_srs_dev(self.n.bit_length() - 1, self.lag.data_ptr())
            ctx.synchronize()
            ctx.srs_lagrange_set_dev(self.lag.data_ptr(), self.n)
        self.setup = pa.SetupForProver(ctx, self.circs[0])
        self.wtns = [c.export("wtns") for c in self.circs]
        self.want = [self.setup.prove(c) for c in self.circs]
        assert len(set(self.want)) == 3
        self.num_variables = po.load_r1cs_bin(self.r1cs).num_variables

    def close(self, ctx):
        ctx.srs_lagrange_clear()
        self.setup.close()
        for c in self.circs:
            c.close()


@pytest.mark.parametrize("log_gates,lc_terms,lagrange", [(10, 0, False), (10, 8, False), (12, 0, True), (12, 8, True)])
def test_stream_of_witnesses(ctx, log_gates, lc_terms, lagrange):
    """lc_terms = 0: the pinned-subset body, independent temporaries (eval_witness_ops); 8: chained linear forms (eval_witness_runs)"""
    import plonkit_amd as pa
    S = Stream(ctx, 1 << log_gates, lc_terms, 77 + lc_terms, lagrange)
    vk = S.setup.verification_key_bytes(pa.crs42_g2_bytes())
    for k in (2, 0, 1):
        got = S.setup.prove_wtns(S.wtns[k])
        assert got == S.want[k], "witness %d" % k
        assert pa.verify(vk, got)
    w = ol.fr_vec(po.parse_wtns(S.wtns[1]))
    assert S.setup.prove_witness(w) == S.want[1]
    assert S.setup.prove_witness_dev(to_dev_fr(w), w.shape[0]) == S.want[1]
    S.close(ctx)


# ------------------------------------------------------------------------------------------------ 5
@pytest.fixture(scope="module")
def stream10(ctx):
    S = Stream(ctx, 1 << 10, 0, 5, False)
    yield S
    S.close(ctx)


def _fresh_key(ctx, S):
    ctx.srs_generate(S.n, 0, 42)
    ctx.srs_lagrange_clear()


def test_recovery_after_each_refusal(ctx, stream10):
    import plonkit_amd as pa
    S = stream10
    _fresh_key(ctx, S)
    L = pa.lib()
    ints = po.parse_wtns(S.wtns[0])
    nv = S.num_variables
    assert len(ints) >= nv
    good = lambda k: S.setup.prove_wtns(S.wtns[k]) == S.want[k]
    # one wire changed: PLK_ERR_UNSAT and no bytes; the device verdict names the row the circuit object's verdict names
    k = nv // 2
    wrong = list(ints)
    wrong[k] = (wrong[k] + 1) % R_MOD
    buf, ln, bad = ctypes.create_string_buffer(1 << 16), ctypes.c_uint64(7), ctypes.c_uint64(0)
    raw = wtns_file(wrong)
    assert L.plk_prove_wtns(ctx._h, S.setup._h, raw, ctypes.c_uint64(len(raw)), buf, ctypes.c_uint64(len(buf)), ctypes.byref(ln), ctypes.byref(bad)) == ERR_UNSAT
    assert ln.value == 0 and buf.raw[:64] == b"\x00" * 64 and bad.value == MASK and "must satisfy" in pa.last_error()
    assert good(1)
    for call in (lambda: S.setup.prove_witness(ol.fr_vec(wrong)), lambda: S.setup.prove_witness_dev(to_dev_fr(ol.fr_vec(wrong)), len(wrong))):
        with pytest.raises(pa.PlkError) as e:
            call()
        assert e.value.code == ERR_UNSAT
    tampered = pa.Circuit(S.r1cs, False, raw, False)
    verdict = S.setup.validate_witness(tampered)
    tampered.close()
    assert verdict[0] is False and verdict[1] is not None
    assert S.setup.validate_witness_dev(to_dev_fr(ol.fr_vec(wrong)), len(wrong)) == verdict
    assert S.setup.validate_witness_dev(to_dev_fr(ol.fr_vec(ints)), len(ints)) == (True, None)
    assert good(2)
    # a file with an element >= r
    notin = list(ints)
    notin[k] = R_MOD + 3
    notin[k + 9] = R_MOD
    with pytest.raises(pa.PlkError) as e:
        S.setup.prove_wtns(wtns_file(notin))
    assert e.value.code == ERR_FORMAT and e.value.bad_index == k and "read witness failed: not in field" in str(e.value)
    assert good(0)
    beyond = list(ints) + [1, R_MOD]                     # every element of the file is checked, also those no wire reads
    with pytest.raises(pa.PlkError) as e:
        S.setup.prove_wtns(wtns_file(beyond))
    assert e.value.code == ERR_FORMAT and e.value.bad_index == len(ints) + 1
    assert good(1)
    # one element short
    w = ol.fr_vec(ints)
    for call in (lambda: S.setup.prove_witness(w[:nv - 1]), lambda: S.setup.prove_wtns(wtns_file(ints[:nv - 1])),
                 lambda: S.setup.prove_witness_dev(to_dev_fr(w), nv - 1), lambda: S.setup.validate_witness_dev(to_dev_fr(w), nv - 1)):
        with pytest.raises(pa.PlkError) as e:
            call()
        assert e.value.code == ERR_ARG and "does not match the prepared setup" in str(e.value)
    assert good(2)
    # Montgomery limbs >= r at wire k (and at a later one): PLK_ERR_ARG naming k; garbage in wire 0 is not read
    noncanon = w.copy()
    noncanon[k] = [MASK, MASK, MASK, MASK]
    noncanon[nv - 1] = [(R_MOD >> (64 * j)) & MASK for j in range(4)]
    for call in (lambda: S.setup.prove_witness(noncanon), lambda: S.setup.prove_witness_dev(to_dev_fr(noncanon), len(ints)),
                 lambda: S.setup.validate_witness_dev(to_dev_fr(noncanon), len(ints))):
        with pytest.raises(pa.PlkError) as e:
            call()
        assert e.value.code == ERR_ARG and ("wire %d holds an element that is not a canonical residue (limbs >= r)" % k) in str(e.value)
        assert good(0)
    garbage0 = w.copy()
    garbage0[0] = [MASK, MASK, MASK, MASK]
    assert S.setup.prove_witness(garbage0) == S.want[0]
    assert S.setup.prove_witness_dev(to_dev_fr(garbage0), len(ints)) == S.want[0]


# ------------------------------------------------------------------------------------------------ 6
def test_device_witness_is_read_after_the_callers_stream(ctx, stream10):
    import torch
    S = stream10
    _fresh_key(ctx, S)
    w = ol.fr_vec(po.parse_wtns(S.wtns[2]))
    host = torch.from_numpy(w.view(np.int64)).pin_memory()
    dev = torch.full(host.shape, -1, dtype=torch.int64, device="cuda:0")            # garbage until the copy below has run
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev.copy_(host, non_blocking=True)
    assert S.setup.prove_witness_dev(dev, w.shape[0], stream=side) == S.want[2]     # no synchronisation in between
    side.synchronize()


# ------------------------------------------------------------------------------------------------ 7
def test_two_contexts_one_setup(ctx, stream10):
    import plonkit_amd as pa
    S = stream10
    _fresh_key(ctx, S)
    other = pa.Context(0)
    other.share_srs_from(ctx)
    ctxs, jobs = [ctx, other], [(0, 1), (2, 0)]
    got, errs = [[], []], []
    gate = threading.Barrier(2)

    def worker(t):
        try:
            gate.wait()
            for k in jobs[t]:
                got[t].append(S.setup.prove_wtns(S.wtns[k], ctx=ctxs[t]))
        except Exception as exc:                                       # noqa: BLE001
            errs.append(repr(exc))
    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    other.close()
    assert not errs, errs
    for t in range(2):
        assert got[t] == [S.want[k] for k in jobs[t]], "thread %d" % t


# ------------------------------------------------------------------------------------------------ 8
def _run_cli(args):
    import plonkit_amd as pa
    cli = os.path.join(os.path.dirname(pa.lib_path()), "plonkit")
    return subprocess.run(["timeout", "-k", "10", "120", cli] + args, capture_output=True, text=True, timeout=150)


def test_cli_prove_many(ctx, stream10, golden_dir, tmp_path):
    import plonkit_amd as pa
    S = stream10
    _fresh_key(ctx, S)
    key, circ = str(tmp_path / "k.key"), str(tmp_path / "c.r1cs")
    open(key, "wb").write(ctx.srs_store_key(pa.crs42_g2_bytes()))
    open(circ, "wb").write(S.r1cs)
    ints = po.parse_wtns(S.wtns[1])
    ints[S.num_variables // 2] = (ints[S.num_variables // 2] + 1) % R_MOD
    files = {"w0.wtns": S.wtns[0], "w1.wtns": S.wtns[1], "w2.wtns": S.wtns[2], "wrong.wtns": wtns_file(ints)}
    for name, data in files.items():
        open(str(tmp_path / name), "wb").write(data)
    out = tmp_path / "proofs"
    r = _run_cli(["prove-many", "-m", key, "-c", circ, "-o", str(out), str(tmp_path / "w0.wtns"), str(tmp_path / "wrong.wtns"), str(tmp_path / "w2.wtns")])
    assert r.returncode == 2, r.stderr
    assert sorted(os.listdir(str(out))) == ["w0.wtns.proof.bin", "w2.wtns.proof.bin"]
    assert (out / "w0.wtns.proof.bin").read_bytes() == S.want[0] and (out / "w2.wtns.proof.bin").read_bytes() == S.want[2]
    bad_lines = [ln for ln in r.stderr.splitlines() if "wrong.wtns" in ln]
    assert bad_lines and "must satisfy" in bad_lines[0]
    out2 = tmp_path / "proofs2"
    r = _run_cli(["prove-many", "-m", key, "-c", circ, "-o", str(out2)] + [str(tmp_path / ("w%d.wtns" % k)) for k in range(3)])
    assert r.returncode == 0, r.stderr
    for k in range(3):
        assert (out2 / ("w%d.wtns.proof.bin" % k)).read_bytes() == S.want[k]
    # a *.json witness goes through the host parser: the reference's simple circuit and its golden proof
    out3 = tmp_path / "proofs3"
    r = _run_cli(["prove-many", "-m", os.path.join(golden_dir, "setup_2pow10.key"), "-c", os.path.join(golden_dir, "circuit.r1cs.json"), "-o", str(out3),
                  os.path.join(golden_dir, "witness.json")])
    assert r.returncode == 0, r.stderr
    assert (out3 / "witness.json.proof.bin").read_bytes() == open(os.path.join(golden_dir, "proof.bin"), "rb").read()
