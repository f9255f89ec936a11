"""-m gpu: plk_kzg_verify_multi_many_dev and plk_kzg_verify_multi_front_dev (kzg_multi_verify.hip): many multi-point openings of one shape,
each verified on its own on the device, against plk_kzg_verify_multi per opening.

Every opening is made by construction with tau = 42 and no prover call: commitments are horner(f_i, 42) G, W and W' are h(42) G and
Q(42) G with h and Q from the Python-integer model (tests/gen/kzg_multi_cases.py), polynomials have 5 coefficients.  The expected column
is pa.kzg_verify_multi per opening (PlkError of code ERR_ARG = 2) AND the literal list the construction implies.  The front's scalars are
the model's (c_values, r_at, z_at), bit for bit after Montgomery conversion.  Exact arithmetic: no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol
from oracle.oracle_lib import Q_MOD, R_MOD
from tests.gen import kzg_multi_cases as km

ERR_ARG = 1
TAU = km.TAU
GAMMA = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80919 % R_MOD
U_RANDOM = 0x1f2e3d4c5b6a79880706050403020100fedcba98765432100123456789abcdef % R_MOD
G = ol.g1_generator()
INF = np.zeros(8, dtype=np.uint64)
R_LIMBS = ol.int_to_limbs(R_MOD)
PASS_MAX, PASS_BYTES = 1 << 16, 64 << 20


@pytest.fixture(scope="module")
def pa():
    import plonkit_amd
    return plonkit_amd


@pytest.fixture(scope="module")
def ctx(pa):
    c = pa.Context(0)
    c.srs_generate(1 << 10, 0, TAU)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _g(k):
    return ol.g1_mul(G, k % R_MOD) if k % R_MOD else INF.copy()


def _polys(m, seed, coeffs=5):
    rng = np.random.default_rng(seed)
    return [[int(x) * 0x9e3779b97f4a7c15f39cc0605cedc835 % R_MOD for x in rng.integers(1, 1 << 62, size=coeffs)] for _ in range(m)]


class Opening:
    """one opening: the arrays the library reads, and the integers behind the scalars (None where a word is no residue)"""

    def __init__(self, polys, points, sets, gamma, u):
        o = km.opening(polys, points, sets, gamma, u)
        self.sets = list(sets)
        self.cm = np.stack([_g(km.horner(f, TAU)) for f in polys])
        self.pts = np.stack([ol.fr_mont(t) for t in points])
        self.ev = np.stack([np.stack([ol.fr_mont(y) for y in row]) for row in o["evals"]])
        self.gamma, self.u = ol.fr_mont(gamma), ol.fr_mont(u)
        self.proof = np.stack([_g(o["w"]), _g(o["w2"])])
        self.ints = {"points": list(points), "evals": [list(r) for r in o["evals"]], "gamma": gamma, "u": u}
        self.w, self.malformed = o["w"], False

    def copy(self):
        import copy
        return copy.deepcopy(self)

    def scalars(self):
        """[count + 3, 4]: the model's c_i, -sum c_i r_i(u), -Z_T(u), u as Montgomery words; zero for a malformed opening"""
        m = len(self.sets)
        if self.malformed:
            return np.zeros((m + 3, 4), dtype=np.uint64)
        i = self.ints
        c, z_t = km.c_values(i["points"], self.sets, i["gamma"], i["u"])
        total = sum(ci * km.r_at(i["points"], mask, row, i["u"]) for ci, mask, row in zip(c, self.sets, i["evals"])) % R_MOD
        return np.stack([ol.fr_mont(x) for x in c + [-total, -z_t, i["u"]]])

    # ---- single changes; each returns a new opening
    def with_eval(self, i, j, delta=1, raw=None):
        o = self.copy()
        if raw is not None:
            o.ev[i, j] = raw
            o.malformed = o.malformed or bool((self.sets[i] >> j) & 1)
        else:
            o.ints["evals"][i][j] = (o.ints["evals"][i][j] + delta) % R_MOD
            o.ev[i, j] = ol.fr_mont(o.ints["evals"][i][j])
        return o

    def with_proof(self, k, point):
        o = self.copy()
        o.proof[k] = point
        return o

    def with_commitment(self, i, point):
        o = self.copy()
        o.cm[i] = point
        return o

    def with_gamma(self, gamma):
        o = self.copy()
        o.ints["gamma"], o.gamma = gamma, ol.fr_mont(gamma)
        return o

    def with_u(self, u):
        o = self.copy()
        o.ints["u"], o.u = u, ol.fr_mont(u)
        return o

    def broken(self, **arrays):
        o = self.copy()
        for k, v in arrays.items():
            setattr(o, k, v)
        o.malformed = True
        return o


def _cpu(pa, o):
    try:
        return 1 if pa.kzg_verify_multi(o.cm, o.pts, o.sets, o.ev, o.gamma, o.u, o.proof, pa.crs42_g2_bytes()) else 0
    except pa.PlkError as e:
        assert e.code == ERR_ARG
        return 2


def _pack(rows, m, p):
    """the six device arrays of a batch"""
    n = len(rows)
    if n == 0:
        return [0] * 6
    return [_dev(np.stack([getattr(o, k) for o in rows]).reshape(n * w, -1)) for k, w in (("cm", m), ("pts", p), ("ev", m * p), ("gamma", 1), ("u", 1), ("proof", 2))]


def _verdicts(ctx, pa, rows, m, p, sets):
    import torch
    n = len(rows)
    d = _pack(rows, m, p)
    verdict = torch.full((n + 48,), 0xAA, dtype=torch.uint8, device="cuda:0")
    ctx.kzg_verify_multi_many_dev(m, p, sets, d[0], d[1], d[2], d[3], d[4], d[5], n, pa.crs42_g2_bytes(), verdict.data_ptr() + 17 if n else 0)
    torch.cuda.synchronize()
    ctx.synchronize()
    got = verdict.cpu().numpy()
    assert (got[:17] == 0xAA).all() and (got[17 + n:] == 0xAA).all()                  # canaries on both sides of an unaligned pointer
    return list(got[17:17 + n])


def _front(ctx, rows, m, p, sets):
    import torch
    n = len(rows)
    d = _pack(rows, m, p)
    scalars = torch.full((n * (m + 3) * 4 + 8,), -1, dtype=torch.int64, device="cuda:0")
    state = torch.full((n + 48,), 0xAA, dtype=torch.uint8, device="cuda:0")
    ctx.kzg_verify_multi_front_dev(m, p, sets, d[0], d[1], d[2], d[3], d[4], d[5], n, scalars, state.data_ptr() + 17)
    torch.cuda.synchronize()
    ctx.synchronize()
    st, sc = state.cpu().numpy(), scalars.cpu().numpy().view(np.uint64)
    assert (st[:17] == 0xAA).all() and (st[17 + n:] == 0xAA).all() and (sc[n * (m + 3) * 4:] == np.uint64(2 ** 64 - 1)).all()
    return list(st[17:17 + n]), sc[:n * (m + 3) * 4].reshape(n, m + 3, 4)


# ------------------------------------------------------------------------------------------------ 1. the kinds table
KIND_SETS = km.plonk_like_masks(3)                                   # [5, 3, 3]: f_0 at t_0 and t_2, f_1 and f_2 at t_0 and t_1
KIND_POINTS = [9, 0, TAU]
KIND_WANT = [1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2]


def _opening_kinds():
    polys, pts, sets = _polys(3, 99), KIND_POINTS, KIND_SETS
    v = Opening(polys, pts, sets, GAMMA, U_RANDOM)
    assert v.w != 0
    out = [v,                                                                          # 0 valid
           v.with_eval(1, 1),                                                          # 1 an evaluation inside a set + 1
           v.with_eval(1, 2),                                                          # 2 an evaluation outside a set + 1
           v.with_eval(0, 1, raw=R_LIMBS),                                             # 3 a non-residue outside a set
           v.with_proof(0, ol.g1_add(v.proof[0], G)),                                  # 4 W + G
           v.with_proof(1, ol.g1_add(v.proof[1], G)),                                  # 5 W' + G
           v.with_commitment(2, ol.g1_add(v.cm[2], G)),                                # 6 a commitment + G
           v.with_gamma((GAMMA + 1) % R_MOD),                                          # 7 gamma + 1
           v.with_u((U_RANDOM + 1) % R_MOD)]                                           # 8 u + 1
    zero = Opening([[0] * 5] * 3, pts, sets, GAMMA, U_RANDOM)                          # 9 all polynomials zero: infinity everywhere
    assert not zero.cm.any() and not zero.proof.any()
    low = Opening([f[:2] + [0, 0, 0] for f in polys], pts, sets, GAMMA, U_RANDOM)      # 10 degree < |S_i| = 2: f_i = r_i, h = 0, W = infinity
    assert low.w == 0 and not low.proof[0].any() and low.proof[1].any()
    at_t1 = Opening(polys, pts, sets, GAMMA, pts[1])                                   # 11 u = t_1: c_0 = 0 (f_0 is not opened there), Z_T(u) = 0
    c, z_t = km.c_values(pts, sets, GAMMA, pts[1])
    assert c[0] == 0 and c[1] != 0 and z_t == 0
    # 12, 13: f_1 = f_2 with equal sets under gamma = 1 / r - 1, so c_1 C_1 = +- c_2 C_2; f_0 = 0 makes the first product the identity, so
    # the running sum IS c_1 C_1 when c_2 C_2 arrives: the sum doubles, or passes through infinity
    twins = [[0] * 5, polys[1], polys[1]]
    dbl, opp = Opening(twins, pts, sets, 1, U_RANDOM), Opening(twins, pts, sets, R_MOD - 1, U_RANDOM)
    for o, sign in ((dbl, 1), (opp, -1)):
        c, _ = km.c_values(pts, sets, o.ints["gamma"], U_RANDOM)
        assert c[1] == sign * c[2] % R_MOD and c[1] != 0 and np.array_equal(o.cm[1], o.cm[2]) and not o.cm[0].any()
    off = v.cm.copy(); off[1][4] ^= np.uint64(1)                                       # 14 a commitment off the curve
    big = v.proof.copy(); big[1][:4] = ol.int_to_limbs(Q_MOD + 1)                      # 15 a coordinate >= q in W'
    pts_eq = v.pts.copy(); pts_eq[2] = pts_eq[0]                                       # 18 two equal points
    out += [zero, low, at_t1, dbl, opp,
            v.broken(cm=off), v.broken(proof=big), v.broken(gamma=R_LIMBS),            # 16 gamma = r
            v.with_eval(2, 0, raw=R_LIMBS),                                            # 17 an evaluation inside a set = r
            v.broken(pts=pts_eq)]
    return out


@pytest.fixture(scope="module")
def kinds(pa):
    ks = _opening_kinds()
    want = [_cpu(pa, o) for o in ks]
    assert want == KIND_WANT                                                           # what the construction says
    assert [o.malformed for o in ks] == [w == 2 for w in want]
    return ks, want


def test_the_kinds_table(ctx, pa, kinds):
    ks, want = kinds
    assert _verdicts(ctx, pa, ks, 3, 3, KIND_SETS) == want == KIND_WANT


# ------------------------------------------------------------------------------------------------ 2. per opening, at the sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_verify_multi_many_is_kzg_verify_multi_per_opening(ctx, pa, kinds, n):
    """(65 openings x 6 terms: the term lanes cross a workgroup at a boundary that is no multiple of the term count)"""
    ks, want = kinds
    order = [(7 * i + i // 19) % 19 for i in range(n)]                                 # malformed entries between valid and invalid ones
    if n == 1:
        order = [0]
    assert _verdicts(ctx, pa, [ks[k] for k in order], 3, 3, KIND_SETS) == [want[k] for k in order]


# ------------------------------------------------------------------------------------------------ 3. shapes
SHAPE_WANT = [1, 0, 0, 0, 0]


def _shape_rows(m, p, name, sets):
    """valid, and one change each: an evaluation inside a set, W, W', the last commitment"""
    v = Opening(_polys(m, 1000 * m + p), km.point_cases(5, p, seed=m), sets, GAMMA, U_RANDOM)
    i = m - 1
    j = km.members(sets[i], p)[0]
    return [v, v.with_eval(i, j), v.with_proof(0, ol.g1_add(v.proof[0], G)), v.with_proof(1, ol.g1_add(v.proof[1], G)), v.with_commitment(i, ol.g1_add(v.cm[i], G))]


_rows_cache = {}


@pytest.fixture(scope="module")
def shape_rows(pa):
    def get(m, p):
        if (m, p) not in _rows_cache:
            fam = {}
            for name, sets in sorted(km.mask_families(m, p, seed=m + p).items()):
                rows = _shape_rows(m, p, name, sets)
                want = [_cpu(pa, o) for o in rows]
                assert want == SHAPE_WANT, (m, p, name)
                fam[name] = (sets, rows, want)
            _rows_cache[(m, p)] = fam
        return _rows_cache[(m, p)]
    return get


@pytest.mark.parametrize("shape", km.HOST_SHAPES)
def test_shapes_and_mask_families(ctx, pa, shape_rows, shape):
    m, p = shape
    fam = shape_rows(m, p)
    assert set(fam) == set(km.mask_families(m, p))
    for name, (sets, rows, want) in fam.items():
        assert p < 8 or {0, 1, R_MOD - 1, TAU} <= set(rows[0].ints["points"])           # eight points: the whole pool, domain points included
        assert _verdicts(ctx, pa, rows, m, p, sets) == want == SHAPE_WANT, (shape, name)


# ------------------------------------------------------------------------------------------------ 4. the front on its own
def test_the_front_gives_the_models_scalars(ctx, pa, kinds, shape_rows):
    ks, want = kinds
    batches = [(3, 3, KIND_SETS, ks)]
    for m, p in km.HOST_SHAPES:
        batches += [(m, p, sets, rows) for sets, rows, _ in shape_rows(m, p).values()]
    for m, p, sets, rows in batches:
        state, sc = _front(ctx, rows, m, p, sets)
        assert state == [2 if o.malformed else 1 for o in rows], (m, p)
        for k, o in enumerate(rows):
            assert np.array_equal(sc[k], o.scalars()), (m, p, k)
            assert o.malformed == (not sc[k].any())


# ------------------------------------------------------------------------------------------------ 5. the pass seam
def test_the_pass_seam(ctx, pa, shape_rows):
    """shape (32, 8): one opening more than a pass holds, so the second pass has a single lane-group; then the last opening alone is tampered"""
    import torch
    m, p = 32, 8
    per = (m + 3) * (32 + 144) + p * (p - 1) // 2 * 32 + 64 + 64 + 2
    n = min(PASS_MAX, PASS_BYTES // per // 256 * 256) + 1
    assert n == 9217
    sets, rows, want = shape_rows(m, p)["random"]
    order = np.array([(i + 4) % 5 for i in range(n)])                                  # the last opening is the valid one
    assert order[-1] == 0
    d = [_dev(np.stack([getattr(o, k) for o in rows]).reshape(5, -1)[order].reshape(n * w, -1)) for k, w in (("cm", m), ("pts", p), ("ev", m * p), ("gamma", 1), ("u", 1), ("proof", 2))]
    verdict = torch.full((n + 48,), 0xAA, dtype=torch.uint8, device="cuda:0")
    expect = np.array(want, dtype=np.uint8)[order]

    def run():
        ctx.kzg_verify_multi_many_dev(m, p, sets, d[0], d[1], d[2], d[3], d[4], d[5], n, pa.crs42_g2_bytes(), verdict.data_ptr() + 17)
        torch.cuda.synchronize()
        ctx.synchronize()
        got = verdict.cpu().numpy()
        assert (got[:17] == 0xAA).all() and (got[17 + n:] == 0xAA).all()
        return got[17:17 + n]

    assert np.array_equal(run(), expect) and expect[-1] == 1
    d[5][2 * (n - 1)] = _dev(rows[2].proof[0])                                         # W + G in the last opening
    expect[-1] = 0
    assert np.array_equal(run(), expect)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(ctx, pa, kinds):
    import torch
    ks, want = kinds
    n = len(ks)
    d = _pack(ks, 3, 3)
    out = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    sc = torch.zeros(n * 6 * 4, dtype=torch.int64, device="cuda:0")
    g2 = pa.crs42_g2_bytes()

    def refused(words, count, npoints, sets, ptrs=d, nn=n, verdict=out):
        """both calls refuse alike"""
        for call in (lambda: ctx.kzg_verify_multi_many_dev(count, npoints, sets, *ptrs, nn, g2, verdict),
                     lambda: ctx.kzg_verify_multi_front_dev(count, npoints, sets, *ptrs, nn, sc, verdict)):
            with pytest.raises(pa.PlkError) as e:
                call()
            assert e.value.code == ERR_ARG and words in str(e.value), e.value

    refused("empty set", 3, 3, [5, 0, 3])
    refused("a set names a point that does not exist", 3, 3, [5, 3, 11])
    refused("a point belongs to no set", 3, 3, [1, 3, 3])
    refused("out of range", 0, 3, [])
    refused("out of range", 33, 3, [1] * 33)
    refused("out of range", 3, 0, KIND_SETS)
    refused("out of range", 3, 9, KIND_SETS)
    for k in range(6):
        refused("null argument", 3, 3, KIND_SETS, ptrs=d[:k] + [0] + d[k + 1:])
        refused("16-byte aligned", 3, 3, KIND_SETS, ptrs=d[:k] + [d[k].data_ptr() + 8] + d[k + 1:], nn=n - 1)
    refused("null argument", 3, 3, KIND_SETS, verdict=0)
    bad = bytearray(g2); bad[255] ^= 1
    with pytest.raises(pa.PlkError) as e:
        ctx.kzg_verify_multi_many_dev(3, 3, KIND_SETS, *d, n, bytes(bad), out)
    assert e.value.code == ERR_ARG and "plk_pairing_check: G2 point not on the twist" in str(e.value)
    with pytest.raises(pa.PlkError) as e:                                              # misaligned scalars of the front
        ctx.kzg_verify_multi_front_dev(3, 3, KIND_SETS, *d, n, sc.data_ptr() + 8, out)
    assert e.value.code == ERR_ARG and "16-byte aligned" in str(e.value)
    ctx.msm_enqueue_dev(_dev(np.zeros((16, 4), dtype=np.uint64)), 16)                  # a commitment in flight
    try:
        refused("a commitment is still in flight on this context", 3, 3, KIND_SETS)
    finally:
        ctx.msm_finish()
    assert _verdicts(ctx, pa, ks, 3, 3, KIND_SETS) == want                              # and the context still works
