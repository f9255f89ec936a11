"""-m gpu: the two resident keys of a context (ctx.h: ResidentKey, ctx->key[monomial | Lagrange]) are independent of each other: each has
its own fixed-base table, replacing one leaves the other alone, every change of the monomial key voids the context's transform of it
(kzg_all.hip), and a borrower of both keys commits against both.

Referee of every commitment: plk_msm_g1_bases_dev over the same points and scalars, which reads nothing resident and builds no table; the
points are the monomial key as plk_srs_download returns it and its G1 iNTT (plk_g1_intt_srs_dev), which is what
plk_srs_lagrange_from_powers installs.  Affine coordinates are unique: every comparison is an equality of bytes.

What the values route allows: plk_kzg_commit_dev with PLK_KZG_VALUES takes exactly as many terms as the Lagrange-form key has points, so at
the 2^12 key of the first test every commitment against it has 4096 terms; its short commitment (2048 terms) is the one against the 2^11
key of the second test.  At keys this small msm_plan_pass asks for all 15 copies of the table for a short commitment as well
(MSM_SMALL_CHEAP_KEY): the two tables are built by the first commitment against each key and are never the same size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol

TOP = 0x30644e72e131a029                                        # top limb of r: four limbs with a smaller top one are a residue
MONO_LOG, LAG_LOG = 13, 12
SHORT = 1000                                                    # fewer than 4096 terms, no multiple of anything


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _host(t, width):
    return t.cpu().numpy().view(np.uint64).reshape(-1, width)


def _rand_fr(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, size=n, dtype=np.uint64)
    return a


def _lagrange_points(ctx, log_n):
    """the G1 iNTT of the first 2^log_n resident monomial points, in device memory"""
    d = _dev(np.zeros((1 << log_n, 8), dtype=np.uint64))
    ctx.g1_intt_srs_dev(log_n, d)
    ctx.synchronize()
    return d


class TwoKeys:
    """a context with a monomial key of 2^13 points and a Lagrange-form key of 2^12, and both keys' points as plain device arrays"""

    def __init__(self, pa):
        self.ctx = pa.Context(0)
        self.ctx.srs_generate(1 << MONO_LOG, 0, 42)
        self.ctx.srs_lagrange_from_powers(LAG_LOG)
        self.mono = _dev(self.ctx.srs_download(0, 1 << MONO_LOG))
        self.lag = _lagrange_points(self.ctx, LAG_LOG)
        self.seed = 100

    def check_monomial(self, terms):
        self.seed += 1
        s = _dev(_rand_fr(terms, self.seed))
        got = self.ctx.msm_dev(s, terms)
        assert np.array_equal(got, self.ctx.msm_bases_dev(self.mono, s, terms)), ("monomial", terms)
        assert got.any()

    def check_lagrange(self, points):
        self.seed += 1
        terms = self.ctx.srs_lagrange_size()
        s = _dev(_rand_fr(terms, self.seed))
        got = self.ctx.kzg_commit_dev([s], terms, values=True)[0]
        assert np.array_equal(got, self.ctx.msm_bases_dev(points, s, terms)), ("lagrange", terms)
        assert got.any()

    def alternate(self):
        """monomial, Lagrange, monomial, Lagrange: the short commitment first, then 4096 terms"""
        self.check_monomial(SHORT)
        self.check_lagrange(self.lag)
        self.check_monomial(4096)
        self.check_lagrange(self.lag)


@pytest.fixture()
def two_keys():
    import plonkit_amd as pa
    k = TwoKeys(pa)
    yield k
    k.ctx.close()


def test_each_key_keeps_its_own_table(two_keys):
    k = two_keys
    assert (k.ctx.srs_size(), k.ctx.srs_lagrange_size()) == (1 << MONO_LOG, 1 << LAG_LOG)
    assert not np.array_equal(_host(k.lag, 8), _host(k.mono, 8)[: 1 << LAG_LOG])           # the keys differ in size and in points
    k.alternate()
    k.alternate()                                                                          # and again with both tables built


def test_replacing_one_key_leaves_the_other_alone(two_keys):
    import plonkit_amd as pa
    k = two_keys
    k.alternate()
    k.ctx.srs_lagrange_from_powers(LAG_LOG - 1)                                            # a new Lagrange-form key, half the size
    assert (k.ctx.srs_size(), k.ctx.srs_lagrange_size()) == (1 << MONO_LOG, 1 << (LAG_LOG - 1))
    k.check_monomial(4096)
    k.check_lagrange(_lagrange_points(k.ctx, LAG_LOG - 1))                                 # 2048 terms: the short commitment against this form
    k.check_monomial(SHORT)
    k.ctx.srs_update(pa.crs42_g2_bytes(), ol.fr_mont(5))                                   # a new monomial key: the Lagrange-form key no longer belongs
    assert (k.ctx.srs_size(), k.ctx.srs_lagrange_size()) == (1 << MONO_LOG, 0)
    k.mono = _dev(k.ctx.srs_download(0, 1 << MONO_LOG))
    k.check_monomial(4096)


def _open_all(ctx, d_poly, log_n):
    d_proofs = _dev(np.full((1 << log_n, 8), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64))
    ctx.kzg_open_all_dev(d_poly, log_n, d_proofs)
    return _host(d_proofs, 8)


def test_both_loan_paths_void_the_transform_of_the_monomial_key():
    """a context that has its key's transform cached borrows another key, then gets its own back: the openings follow the key each time"""
    import plonkit_amd as pa
    log_n, n = 3, 8
    a, b = pa.Context(0), pa.Context(0)
    try:
        b.srs_generate(n, 0, 42)                                                           # K1
        k1 = b.srs_download(0, n)
        a.srs_generate(n, 0, 43)                                                           # K2
        assert not np.array_equal(k1, a.srs_download(0, n))
        d = _dev(_rand_fr(n, 7))
        first = _open_all(b, d, log_n)                                                     # b's transform of K1 is cached now
        assert np.array_equal(first, _open_all(b, d, log_n))
        b.share_srs_from(a)                                                                # the loan is made: K2
        under_k2 = _open_all(b, d, log_n)
        assert np.array_equal(under_k2, _open_all(a, d, log_n))
        w = ol.omega(log_n)
        for i in range(n):
            _, pi = b.kzg_open_dev([d], n, ol.fr_mont(pow(w, i, ol.R_MOD)))
            assert np.array_equal(under_k2[i], pi), i
        assert not np.array_equal(under_k2, first)
        b.srs_upload(k1)                                                                   # the loan is returned: K1 again
        assert np.array_equal(_open_all(b, d, log_n), first)
        a.srs_generate(n, 0, 42)                                                           # (nobody borrows from a any more)
    finally:
        b.close(); a.close()


def test_a_borrower_of_both_keys_commits_against_both():
    import plonkit_amd as pa
    log_n = 12
    n = 1 << log_n
    a, b = pa.Context(0), pa.Context(0)
    try:
        a.srs_generate(n, 0, 42)
        a.srs_lagrange_from_powers(log_n)
        b.share_srs_from(a)
        assert (b.srs_size(), b.srs_lagrange_size()) == (n, n)
        s, v = _dev(_rand_fr(n, 21)), _dev(_rand_fr(n, 22))
        by_a = a.msm_dev(s, n)
        assert np.array_equal(b.msm_dev(s, n), by_a) and by_a.any()
        assert np.array_equal(b.kzg_commit_dev([v], n, values=True), a.kzg_commit_dev([v], n, values=True))
        with pytest.raises(pa.PlkError):
            a.srs_lagrange_from_powers(log_n - 1)                                          # on loan
        # the borrower installs a Lagrange-form key of its own (other points: the second half of the lender's): the monomial loan stays
        own = _host(_lagrange_points(a, log_n), 8)[n // 2:].copy()
        b.srs_lagrange_upload(own)
        assert (b.srs_size(), b.srs_lagrange_size()) == (n, n // 2)
        assert np.array_equal(b.msm_dev(s, n), by_a)
        assert np.array_equal(b.kzg_commit_dev([v], n // 2, values=True)[0], b.msm_bases_dev(_dev(own), v, n // 2))
        a.srs_lagrange_from_powers(log_n - 1)                                              # ... and the lender's Lagrange-form key is free again
        assert a.srs_lagrange_size() == n // 2
        assert np.array_equal(a.kzg_commit_dev([v], n // 2, values=True)[0], a.msm_bases_dev(_lagrange_points(a, log_n - 1), v, n // 2))
        assert np.array_equal(b.msm_dev(s, n), by_a)
        with pytest.raises(pa.PlkError):
            a.srs_generate(n, 0, 42)                                                       # the monomial key is still on loan
    finally:
        b.close(); a.close()
