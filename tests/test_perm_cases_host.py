"""-m "not gpu": tests/gen/perm_cases.py before it judges a kernel.

The model (a dict of lists) gives the sigma values of the oracle's two setups, which reach them by other routes (po.setup: its own dict over
the transpiled gates; po.setup_flat: the C transpiler and one stable numpy sort).  The vectorised form used for the one 2^24 case equals the
dict form on every small case.  And the cases discriminate: for each way a sort or a link can be wrong — listed in perm_cases.py as a wrong
model — the test names the cases whose answer differs from the true one.  That replaces running broken kernels."""
import json

import numpy as np
import pytest

from oracle import plonk_oracle as po
from tests.gen import perm_cases as pc
from tests.gen import round_cases as rc


def test_constants_are_the_projects():
    assert (pc.R_MOD, pc.NON_RESIDUES, pc.ROOT_2_28) == (rc.R_MOD, rc.NON_RESIDUES, rc.ROOT_2_28) and pc.NON_RESIDUES == tuple(po.NON_RESIDUES)
    assert [pc.passes(m) for m in pc.PASS_NUM_VARS] == [1, 1, 2, 2, 3, 3, 4, 4] and pc.passes(pc.THREE_PASS) == 3 and pc.passes(pc.LARGE_NUM_VARS) == 4


def test_model_gives_the_oracles_sigma_values():
    """a chain circuit of 300 constraints (domain 2^9): rows from the Python transpiler against po.setup, rows from the C transpiler against
    po.setup_flat on the binary form of the same circuit"""
    import plonkit_amd as pa
    from tests.test_oracle_golden import _chain_circuit
    r1cs, wit = _chain_circuit(300, 0x706c6f6e6b6974 + 300)
    cons = [[{str(w): str(c) for w, c in lc} for lc in con] for con in r1cs.constraints]
    js = {"nPubInputs": 1, "nOutputs": 0, "nVars": r1cs.num_variables, "constraints": cons}
    r_o = po.load_r1cs_json(js)
    T = po.transpile(r_o)
    rows, n_in, N = po._assemble(r_o, T)
    S = po.setup(r_o, T)
    assert S.N == N == 512
    cols = [[g.vars[j] for g in rows] + [0] * (N - len(rows)) for j in range(4)]
    nxt = pc.successors(cols)
    assert sum(1 for p, q in enumerate(nxt) if p != q) > N                       # a real permutation, not the identity
    for j, want in enumerate(pc.sigmas_of(nxt, S.log_n)):
        assert np.array_equal(rc.to_array(want), S.sigma_values[j]), j
    circ = pa.Circuit(json.dumps(js).encode(), True)
    rf = po.load_r1cs_flat(circ.export("r1cs"))
    V = po._rows_flat(rf)[0]
    S2 = po.setup_flat(rf)
    nxt2 = pc.successors([[int(v) for v in V[j]] for j in range(4)])
    for j, want in enumerate(pc.sigmas_of(nxt2, S2.log_n)):
        assert np.array_equal(rc.to_array(want), S2.sigma_values[j]), j
    circ.close()


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_vectorised_form_equals_the_model(name):
    c = pc.case(name)
    V = np.array(c.cols, dtype=np.uint32)
    nxt = pc.successors_vectorised(V)
    assert nxt.tolist() == c.nxt
    assert pc.index_of_vectorised(nxt).tolist() == pc.index_of(c.nxt)


def test_cases_are_what_their_names_say():
    """the properties the shapes were chosen for, checked on the data"""
    for m in pc.PASS_NUM_VARS:
        c = pc.case("passes/num_vars=%d" % m)
        ids = {v for col in c.cols for v in col}
        P = pc.passes(m)
        shift = 8 * (P - 1)
        assert c.log_n == 10 and m - 1 in ids and len(ids) >= 2
        if m > 2:
            assert any(a != b and a ^ b < 256 for a in ids for b in ids if a and b), m                      # differ in the lowest digit only
        if P > 1:
            assert any(a != b and (a ^ b) >> shift and not (a ^ b) & ((1 << shift) - 1) for a in ids for b in ids), m   # in the top digit only
    assert {0xFFFFFFFF, 0x80000000, 0x01000000} <= {v for col in pc.case("passes/num_vars=4294967296").cols for v in col}
    for log_n in pc.SIZE_LOG_N:
        c = pc.case("size/log_n=%d" % log_n)
        assert c.log_n == log_n and pc.passes(c.num_vars) == 3
        assert log_n < 3 or sum(1 for p, q in enumerate(c.nxt) if p != q) >= len(c.nxt) // 2
    hub = pc.case("hub/a_and_b_columns")
    assert sum(col.count(0x12345) for col in hub.cols) == 32768
    one = pc.case("hub/one_id_everywhere")
    assert one.nxt == [(p + 1) % (1 << 16) for p in range(1 << 16)]
    pos = lambda c: [c.cols[p & 3][p >> 2] for p in range(4 << c.log_n)]
    w = pos(pc.case("hub/wave_of_64_and_65"))
    assert w.count(0x0a0b0c) == 64 and len(set(w[320:384])) == 1 and w.count(0x0a0b0d) == 65 and len(set(w[576:641])) == 1
    assert w.count(0x1f0001) == 64 and len(set(w[4032:4096])) == 1 and w.count(0x1f0002) == 65 and len(set(w[4096:4161])) == 1
    a = pos(pc.case("hub/two_ids_alternating"))
    assert len(set(a[0::2])) == 1 and len(set(a[1::2])) == 1 and a[0] != a[1]
    d = pos(pc.case("hub/64_distinct_digits"))
    assert len({v & 255 for v in d[192:256]}) == 64 and len({(v >> 8) & 255 for v in d[448:512]}) == 64 and len({v & 255 for v in d[448:512]}) == 1
    for name in ("degenerate/all_dummy", "degenerate/all_distinct"):
        assert pc.case(name).nxt == list(range(1 << 14)), name
    assert 0 not in pos(pc.case("degenerate/no_dummy"))
    last = pos(pc.case("degenerate/largest_id_last"))
    assert last[-1] == max(last) == pc.THREE_PASS - 1 and pc.case("degenerate/largest_id_last").nxt[-1] == 17


def _caught(wrong, names):
    return [name for name in names if wrong(pc.case(name).cols) != pc.case(name).nxt]


def test_cases_tell_a_short_sort_from_the_right_one():
    """a sort that keeps 8, 16 or 24 bits of the key, on each case whose num_vars needs one more pass than that: every pass-count case of that
    pass count catches it, and so do the random sizes and the hub cases named below"""
    by_passes = {}
    for name in pc.CASE_NAMES:
        by_passes.setdefault(pc.passes(pc.case(name).num_vars), []).append(name)
    for bits, must in ((8, ["passes/num_vars=257", "passes/num_vars=65536"]),
                       (16, ["passes/num_vars=65537", "passes/num_vars=16777216", "size/log_n=3", "size/log_n=10", "size/log_n=14",
                             "hub/wave_of_64_and_65", "hub/two_ids_alternating", "hub/a_and_b_columns", "degenerate/largest_id_last"]),
                       (24, ["passes/num_vars=16777217", "passes/num_vars=4294967296"])):
        caught = _caught(lambda cols: pc.wrong_truncated_sort(cols, bits), by_passes[bits // 8 + 1])
        print("sort of %d bits only: caught by %s" % (bits, caught))
        assert set(must) <= set(caught), (bits, caught)
    # and the full sort of the same wrong model is the true one: what the cases catch is the missing pass, not the model's form
    for name in ("passes/num_vars=4294967296", "size/log_n=11", "hub/wave_of_64_and_65"):
        assert pc.wrong_truncated_sort(pc.case(name).cols, 32) == pc.case(name).nxt, name


@pytest.mark.parametrize("wrong,must", [
    (pc.wrong_reversed, ["passes/num_vars=2", "passes/num_vars=4294967296", "size/log_n=3", "size/log_n=14", "hub/a_and_b_columns",
                         "hub/wave_of_64_and_65", "hub/64_distinct_digits", "hub/one_id_everywhere", "degenerate/no_dummy"]),
    (pc.wrong_no_wrap, ["passes/num_vars=2", "passes/num_vars=256", "size/log_n=1", "size/log_n=4", "size/log_n=13", "hub/a_and_b_columns",
                        "hub/two_ids_alternating", "hub/one_id_everywhere", "degenerate/largest_id_last"]),
    (pc.wrong_dummy_linked, ["passes/num_vars=2", "passes/num_vars=65537", "size/log_n=2", "size/log_n=12", "degenerate/all_dummy",
                             "degenerate/largest_id_last"]),
    (pc.wrong_tile_local_wrap, ["size/log_n=12", "size/log_n=14", "hub/a_and_b_columns", "hub/wave_of_64_and_65", "hub/one_id_everywhere"]),
], ids=["reversed_cycle", "no_wrap", "dummy_linked", "tile_local_wrap"])
def test_cases_tell_a_wrong_link_from_the_right_one(wrong, must):
    caught = _caught(wrong, pc.CASE_NAMES)
    print("%s: caught by %s" % (wrong.__name__, caught))
    assert set(must) <= set(caught), caught
    if wrong is pc.wrong_tile_local_wrap:                      # a one-tile case cannot see it: that is what the larger sizes are for
        assert not any(pc.case(name).log_n <= 10 for name in caught)
