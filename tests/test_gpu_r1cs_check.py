"""-m gpu: a witness against its R1CS on the device (plk_r1cs_*, r1cs_check.hip) and SetupForProver::validate_witness
(plk_validate_witness).  The circuits are written here as circom JSON text and loaded with plk_circuit_load(.., r1cs_is_json=1); every
expected verdict — valid or not, and the lowest failing constraint — comes from the Python-integer loop `py_check` below, which reads
wire 0 as the constant 1.  All comparisons are exact."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ circuits as Python integers
def lc_value(lc, wit):
    return sum(c * (1 if w == 0 else wit[w]) for w, c in lc) % R_MOD


def py_check(cons, wit):
    """the lowest constraint with <A,w> * <B,w> != <C,w> (wire 0 = 1 whatever wit[0] holds), None when all hold"""
    for i, (A, B, C) in enumerate(cons):
        if lc_value(A, wit) * lc_value(B, wit) % R_MOD != lc_value(C, wit):
            return i
    return None


def circuit_json(cons, num_vars, n_pub=1):
    """circom JSON TEXT written by hand: a wire may appear twice in one LC (duplicate keys), which json.dumps of a dict cannot say"""
    body = ",".join("[%s]" % ",".join("{%s}" % ",".join('"%d":"%d"' % (w, c) for w, c in lc) for lc in con) for con in cons)
    return ('{"n8":32,"prime":"%d","nVars":%d,"nOutputs":0,"nPubInputs":%d,"nPrvInputs":0,"nLabels":%d,"nConstraints":%d,"constraints":[%s]}'
            % (R_MOD, num_vars, n_pub, num_vars, len(cons), body)).encode()


def mont(wit):
    return ol.fr_vec(wit)


def load(cons, num_vars, wit=None):
    import plonkit_amd as pa
    w = json.dumps([str(x) for x in wit]).encode() if wit is not None else None
    return pa.Circuit(circuit_json(cons, num_vars), True, w, w is not None)


def shapes_circuit(m, seed, L):
    """m constraints whose LC lengths run through LENS on every side; terms on wire 0, the same wire twice in one LC, coefficients 1,
    r - 1, 2 and random, values 0, 1, r - 1 and random.  Satisfying by construction: C closes through a fresh wire (coefficient from the
    same set), or C is empty beside an empty A or B.  The very long lengths are kept to the first and last constraints of a large circuit
    (the JSON of 4097 constraints of 1025-term LCs would be 100 MB); every length still appears on every side."""
    rng = random.Random(seed)
    lens = [0, 1, 2, 3, L - 1, L, L + 1, 63, 64, 65, 129, 1025]
    small = [0, 1, 2, 3, L - 1, L, L + 1]
    wit = [1, rng.randrange(R_MOD), 0, 1, R_MOD - 1] + [rng.randrange(R_MOD) for _ in range(5)]

    def coeff():
        return [1, R_MOD - 1, 2, rng.randrange(1, R_MOD)][rng.randrange(4)]

    def free_lc(n):
        lc = [(rng.randrange(len(wit)), coeff()) for _ in range(n)]
        if n >= 2 and rng.randrange(2):
            lc[1] = (lc[0][0], lc[1][1])                     # the same wire twice
        if n >= 1 and rng.randrange(3) == 0:
            lc[-1] = (0, lc[-1][1])                          # a term on wire 0
        return lc

    cons = []
    for i in range(m):
        pool = lens if (i < 12 or i >= m - 12 or m <= 65) else small
        la, lb, lcc = (pool[(i + 5 * s) % len(pool)] for s in range(3))
        if lcc == 0:                                         # empty A or B beside an empty C: holds by arithmetic, the reference skips it
            if (i // len(pool)) % 2 == 0:                    # (alternating, so that the length given up on one side comes back in the next cycle)
                la = 0
            else:
                lb = 0
        A, B = free_lc(la), free_lc(lb)
        if lcc == 0:
            C = []
        else:
            C = free_lc(lcc - 1)
            k = coeff()
            fresh = len(wit)
            wit.append((lc_value(A, wit) * lc_value(B, wit) - lc_value(C, wit)) * pow(k, -1, R_MOD) % R_MOD)
            C.insert(rng.randrange(len(C) + 1), (fresh, k))
        cons.append((A, B, C))
    assert py_check(cons, wit) is None
    return cons, wit


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    import plonkit_amd as pa
    return pa.r1cs_long_lc_terms()


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 4097])
def test_shapes(ctx, L, m):
    import plonkit_amd as pa
    cons, wit = shapes_circuit(m, 1000 + m, L)
    sides = [set(len(con[s]) for con in cons) for s in range(3)]
    if m >= 65:
        for s in range(3):
            assert sides[s] >= {0, 1, 2, 3, L - 1, L, L + 1, 63, 64, 65, 129, 1025}, (s, sorted(sides[s]))
    circ = load(cons, len(wit))
    r = pa.R1cs(ctx, circ)
    assert r.num_constraints == m and r.num_variables == len(wit)
    assert r.check(mont(wit)) == (True, None)
    # 4. wire 0 is the constant 1 whatever witness[0] holds
    for w0 in (0, random.Random(m).randrange(R_MOD)):
        assert r.check(mont([w0] + wit[1:])) == (True, None)
    # one broken element: the verdict of the integer loop
    rng = random.Random(m)
    for _ in range(3):
        bad = list(wit)
        k = rng.randrange(1, len(bad))
        bad[k] = (bad[k] + 1 + rng.randrange(R_MOD - 1)) % R_MOD
        want = py_check(cons, bad)
        assert r.check(mont(bad)) == (want is None, want), k
        assert r.check(mont([0] + bad[1:])) == (want is None, want), k
    r.close(); circ.close()


# ------------------------------------------------------------------ 2. top of the ranges
@pytest.mark.parametrize("side", [0, 1, 2])
def test_longest_lc_of_largest_terms(ctx, side):
    """one LC of 1025 terms, every coefficient r - 1, every value r - 1: 1025 (r-1)^2 = 1025 mod r.  An accumulation that left its
    layer's contract would show here"""
    import plonkit_amd as pa
    n = 1025
    wit = [1] + [R_MOD - 1] * n + [n % R_MOD]
    long_lc, total, one = [(1 + k, R_MOD - 1) for k in range(n)], [(n + 1, 1)], [(0, 1)]
    con = [(long_lc, one, total), (one, long_lc, total), (total, one, long_lc)][side]
    assert py_check([con], wit) is None
    circ = load([con], len(wit))
    r = pa.R1cs(ctx, circ)
    assert r.check(mont(wit)) == (True, None)
    for k in (1, n // 2, n, n + 1):
        bad = list(wit)
        bad[k] = (bad[k] + 1) % R_MOD
        assert py_check([con], bad) == 0 and r.check(mont(bad)) == (False, 0)
    r.close(); circ.close()


# ------------------------------------------------------------------ 3. the lowest failing constraint
@pytest.mark.parametrize("where", ["short A", "long A", "short C", "long C"])
def test_lowest_failing_constraint(ctx, L, where):
    import plonkit_amd as pa
    m, ks = 4097, (5, 64, 4096)
    rng = random.Random(["short A", "long A", "short C", "long C"].index(where))
    base = 16
    wit = [1] + [rng.randrange(1, R_MOD) for _ in range(base - 1)]
    s_all, s_last = 1, 2                                     # wire 1 sits in constraints 5, 64, 4096; wire 2 in 4096 only
    cons = []
    side, long_ = (0 if "A" in where else 2), "long" in where
    for i in range(m):
        A = [(rng.randrange(3, base), 1)]
        B = [(rng.randrange(3, base), 1)]
        C = []
        planted = []
        if i in ks:
            planted = [(s_all, 3)] + ([(s_last, 5)] if i == ks[2] else [])
            if long_:
                planted += [(rng.randrange(3, base), rng.randrange(1, R_MOD)) for _ in range(L + 5)]
                rng.shuffle(planted)
        if side == 0:
            A = A + planted
        else:
            C = planted
        fresh = len(wit)
        wit.append((lc_value(A, wit) * lc_value(B, wit) - lc_value(C, wit)) % R_MOD)
        cons.append((A, B, C + [(fresh, 1)]))
    assert py_check(cons, wit) is None
    circ = load(cons, len(wit))
    r = pa.R1cs(ctx, circ)
    assert r.check(mont(wit)) == (True, None)
    for wire, want in ((s_all, ks[0]), (s_last, ks[2])):
        bad = list(wit)
        bad[wire] = (bad[wire] + 1) % R_MOD
        assert py_check(cons, bad) == want
        assert r.check(mont(bad)) == (False, want)
    r.close(); circ.close()


# ------------------------------------------------------------------ 5. witnesses on the device
def test_device_witness(ctx, L):
    import torch
    import plonkit_amd as pa
    cons, wit = shapes_circuit(65, 7, L)
    unread = len(wit)                                        # one more variable that no term reads
    wit = wit + [12345]
    circ = load(cons, len(wit))
    r = pa.R1cs(ctx, circ)
    n = len(wit)
    bad = list(wit)
    bad[len(bad) // 2] = (bad[len(bad) // 2] + 1) % R_MOD
    want_bad = py_check(cons, bad)
    assert want_bad is not None
    side = torch.cuda.Stream()

    def on_stream(values_mont):
        """the tensor the call reads is written by a torch op on `side`, and `side` is what the call is given"""
        src = torch.from_numpy(np.ascontiguousarray(values_mont).view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t = src + 0
        return t

    t = on_stream(mont(wit))
    assert r.check_dev(t, n, stream=side) == (True, None)
    tb = on_stream(mont(bad))
    assert r.check_dev(tb, n, stream=side) == (False, want_bad)
    # extra elements are ignored, fewer are refused
    longer = on_stream(np.concatenate([mont(wit), mont([5, 6, 7])]))
    assert r.check_dev(longer, n + 3, stream=side) == (True, None)
    with pytest.raises(pa.PlkError) as e:
        r.check_dev(t, n - 1, stream=side)
    assert e.value.code == 1
    with pytest.raises(pa.PlkError) as e:
        r.check(mont(wit)[:n - 1])
    assert e.value.code == 1
    # an element that is not a canonical residue: refused on a wire some term reads (the lowest such wire is named), ignored elsewhere
    read = sorted(set(w for con in cons for lc in con for w, _ in lc) - {0})
    raw = mont(wit)
    for k in (read[-1], read[3]):
        raw[k] = ol.int_to_limbs(R_MOD)                      # r itself: the smallest value that is not canonical
    with pytest.raises(pa.PlkError) as e:
        r.check_dev(on_stream(raw), n, stream=side)
    assert e.value.code == 1 and "wire %d holds" % read[3] in str(e.value) and "not a canonical residue" in str(e.value)
    with pytest.raises(pa.PlkError) as e:
        r.check(raw)
    assert e.value.code == 1 and "wire %d holds" % read[3] in str(e.value)
    raw = mont(wit)
    raw[unread] = ol.int_to_limbs(R_MOD)
    raw[0] = ol.int_to_limbs((1 << 256) - 1)                 # wire 0 is never read either
    assert r.check_dev(on_stream(raw), n, stream=side) == (True, None)
    # the same R1cs from a second context of the device
    other = pa.Context(0)
    assert r.check_dev(t, n, stream=side, ctx=other) == (True, None)
    assert r.check_dev(tb, n, stream=side, ctx=other) == (False, want_bad)
    assert r.check(mont(bad), ctx=other) == (False, want_bad)
    other.close()
    r.close(); circ.close()


# ------------------------------------------------------------------ 6. the three judges agree, with no key resident
JUDGED = [("synthetic", 8, 0), ("synthetic", 8, 7), ("synthetic", 1000, 0), ("synthetic", 1000, 7), ("synthetic", 5000, 0), ("synthetic", 5000, 7),
          ("poseidon", 1, 0)]


def _judged_circuit(kind, t, lc_terms):
    """(r1cs bytes, wtns bytes, cons, wit, num_inputs) of one of the JUDGED circuits, the R1CS read back from the library's own export"""
    import plonkit_amd as pa
    if kind == "synthetic":
        circ = pa.Circuit.synthetic_ex(t, lc_terms=lc_terms)
    else:
        from tests.gen import poseidon_like as pl
        ni, nv, pcons, pwit = pl.build(t, 77 + t)
        circ = pa.Circuit(json.dumps(pl.as_circom_json(ni, nv, pcons)).encode(), True, json.dumps([str(x) for x in pwit]).encode(), True)
    r1cs, wtns = circ.export("r1cs"), circ.export("wtns")
    circ.close()
    hdr, off, wires, coeffs = ol.r1cs_parse(r1cs)
    cf = ol.fr_ints(coeffs)
    cons = []
    for i in range(hdr["n_constraints"]):
        cons.append(tuple([(int(wires[k]), cf[k]) for k in range(int(off[3 * i + s]), int(off[3 * i + s + 1]))] for s in range(3)))
    wit = ol.fr_ints(ol.wtns_parse(wtns))
    return r1cs, wtns, cons, wit, hdr["n_pub_out"] + hdr["n_pub_in"] + 1


def _changed_witnesses(cons, wit, num_inputs):
    """the circuit's own witness and copies with one element changed: an input, an aux wire of the first constraint, one used only in the
    last, a wire feeding a long LC (>= 5 terms, where the circuit has one)"""
    def wires_of(con):
        return [w for lc in con for w, _ in lc if w >= num_inputs]
    picks = [("own", None), ("input", 1)]
    first = wires_of(cons[0])
    if first:
        picks.append(("first constraint", first[0]))
    earlier = set(w for con in cons[:-1] for w in wires_of(con))
    only_last = [w for w in wires_of(cons[-1]) if w not in earlier]
    if only_last:
        picks.append(("only the last constraint", only_last[0]))
    long_lcs = [lc for con in cons for lc in con if len(lc) >= 5]
    if long_lcs:
        lc = long_lcs[len(long_lcs) // 2]
        picks.append(("a long LC", [w for w, _ in lc if w != 0][-1]))
    out = []
    for name, wire in picks:
        w = list(wit)
        if wire is not None:
            w[wire] = (w[wire] + 1) % R_MOD
        out.append((name, wire, w))
    return out


def _wtns_bytes(template, wit):
    """the library's .wtns export with other values: a 76-byte head, then 32 little-endian canonical bytes per element"""
    assert len(template) == 76 + 32 * len(wit)
    return template[:76] + b"".join(int(x).to_bytes(32, "little") for x in wit)


def _judge(ctx, spec):
    """[(name, R1cs.check verdict, validate_witness verdict)] for one circuit; no key is touched"""
    import plonkit_amd as pa
    r1cs, wtns, cons, wit, num_inputs = _judged_circuit(*spec)
    out = []
    base = pa.Circuit(r1cs, False, wtns, False)
    setup = pa.SetupForProver(ctx, base)
    r = pa.R1cs(ctx, base)
    for name, wire, w in _changed_witnesses(cons, wit, num_inputs):
        circ = pa.Circuit(r1cs, False, _wtns_bytes(wtns, w), False)
        out.append([name, list(r.check(mont(w))), list(setup.validate_witness(circ))])
        circ.close()
    r.close(); setup.close(); base.close()
    return out


def _judge_all_to_stdout():
    """child-process entry of test_judges_agree_with_host_temporaries"""
    import plonkit_amd as pa
    ctx = pa.Context(0)
    print("VERDICTS " + json.dumps([_judge(ctx, spec) for spec in JUDGED]))
    ctx.close()


@pytest.mark.parametrize("spec", JUDGED, ids=["%s-%d-lc%d" % s for s in JUDGED])
def test_three_judges_agree(spec):
    import plonkit_amd as pa
    ctx = pa.Context(0)                                      # a fresh context: no key resident while the judges run
    assert ctx.srs_size() == 0
    r1cs, wtns, cons, wit, num_inputs = _judged_circuit(*spec)
    base = pa.Circuit(r1cs, False, wtns, False)
    stats = json.loads(base.analyse())["constraint_stats"]
    first_row, row = {}, num_inputs - 1                      # the public-input rows come first, then the gates of every non-trivial constraint
    for st in stats:
        first_row[int(st["name"])] = (row, row + st["num_gates"])
        row += st["num_gates"]
    setup = pa.SetupForProver(ctx, base)
    r = pa.R1cs(ctx, base)
    judged = []
    for name, wire, w in _changed_witnesses(cons, wit, num_inputs):
        want = py_check(cons, w)
        circ = pa.Circuit(r1cs, False, _wtns_bytes(wtns, w), False)
        got = r.check(mont(w))
        assert got == (want is None, want), (name, wire)
        valid, bad_row = setup.validate_witness(circ)
        assert valid == (want is None), (name, wire, bad_row)
        if want is not None:
            lo, hi = first_row[want]
            assert lo <= bad_row < hi, (name, wire, want, bad_row, lo, hi)
        else:
            assert bad_row is None
        judged.append((name, circ, want))
    assert judged[0][2] is None and any(w is not None for _, _, w in judged)
    # with a key generated afterwards: prove refuses exactly the witnesses judged invalid
    ctx.srs_generate(1 << 13, 0, 42)
    vk = setup.verification_key_bytes(pa.crs42_g2_bytes())
    for name, circ, want in judged:
        if want is None:
            assert pa.verify(vk, setup.prove(circ)), name
        else:
            with pytest.raises(pa.PlkError) as e:
                setup.prove(circ)
            assert e.value.code == 5, name
        circ.close()
    r.close(); setup.close(); base.close(); ctx.close()


def test_judges_agree_with_host_temporaries(ctx):
    """PLK_WITNESS_TMP_HOST=1 (read once per process, hence the child): the transpiler's temporaries come from the host loop instead of
    the device kernels, and no verdict changes"""
    here = [_judge(ctx, spec) for spec in JUDGED]
    code = "import sys; sys.path.insert(0, %r); import tests.test_gpu_r1cs_check as t; t._judge_all_to_stdout()" % ROOT
    got = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PLK_WITNESS_TMP_HOST="1"), capture_output=True, text=True, timeout=600)
    assert got.returncode == 0, (got.stdout + got.stderr)[-3000:]
    line = [ln for ln in got.stdout.splitlines() if ln.startswith("VERDICTS ")][0]
    assert json.loads(line[len("VERDICTS "):]) == json.loads(json.dumps(here))
    assert any(not v[1][0] for circuit in here for v in circuit) and all(v[1][0] == v[2][0] for circuit in here for v in circuit)


# ------------------------------------------------------------------ 7. refusals of validate_witness
def test_validate_witness_refusals(ctx, golden_dir):
    import torch
    import plonkit_amd as pa
    gold = pa.Circuit.from_files(os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json"))
    no_wit = pa.Circuit.from_files(os.path.join(golden_dir, "circuit.r1cs.json"))
    other = pa.Circuit.synthetic(100)
    ctx.srs_generate(1 << 10, 0, 42)
    ctx.srs_lagrange_clear()
    setup = pa.SetupForProver(ctx, gold)
    assert setup.validate_witness(gold) == (True, None)

    def codes(s, c):
        got = []
        for call in (lambda: s.validate_witness(c), lambda: s.prove(c)):
            with pytest.raises(pa.PlkError) as e:
                call()
            got.append(e.value.code)
        return got
    zeros = [np.zeros((8, 4), dtype=np.uint64) for _ in range(11)]
    polys = pa.SetupForProver.from_polynomials(ctx, 7, 1, zeros[:6], zeros[6], zeros[7:])
    assert codes(polys, gold) == [1, 1]                      # no gate structure
    assert codes(setup, no_wit) == [1, 1]                    # no witness
    assert codes(setup, other) == [1, 1]                     # another circuit
    # a commitment in flight on the context
    r = pa.R1cs(ctx, gold)
    limbs = np.random.default_rng(3).integers(0, 1 << 62, size=(1024, 4), dtype=np.uint64)
    limbs[:, 3] &= np.uint64((1 << 60) - 1)
    scalars = torch.from_numpy(limbs.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    ctx.msm_enqueue_dev(scalars, 1024)
    try:
        assert codes(setup, gold) == [1, 1]
        with pytest.raises(pa.PlkError) as e:
            r.check(mont([1, 35, 3, 9]))
        assert e.value.code == 1
    finally:
        ctx.msm_finish()
    assert setup.validate_witness(gold) == (True, None)
    assert setup.prove(gold) == open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    r.close(); polys.close(); setup.close()
    for c in (gold, no_wit, other):
        c.close()


# ------------------------------------------------------------------ 8. the binary
def test_cli_check_witness(golden_dir, tmp_path):
    import plonkit_amd as pa
    cli = os.path.join(os.path.dirname(pa.lib_path()), "plonkit")
    circ, wit_path = os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json")
    ok = subprocess.run([cli, "check-witness", "-c", circ, "-w", wit_path], capture_output=True, text=True, timeout=120)
    assert ok.returncode == 0, ok.stderr
    js = json.load(open(circ))
    cons = [tuple([(int(w), int(c)) for w, c in lc.items()] for lc in con) for con in js["constraints"]]
    wit = [int(x) for x in json.load(open(wit_path))]
    assert py_check(cons, wit) is None
    for k in range(1, len(wit)):
        bad = list(wit)
        bad[k] = (bad[k] + 1) % R_MOD
        want = py_check(cons, bad)
        assert want is not None
        path = str(tmp_path / ("bad%d.json" % k))
        json.dump([str(x) for x in bad], open(path, "w"))
        got = subprocess.run([cli, "check-witness", "-c", circ, "-w", path], capture_output=True, text=True, timeout=120)
        assert got.returncode == 2 and "constraint %d fails" % want in got.stderr, (k, got.returncode, got.stderr)
    usage = subprocess.run([cli], capture_output=True, text=True)
    assert "check-witness" in usage.stderr and "the reference has no such command" in usage.stderr
