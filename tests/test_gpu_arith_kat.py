"""-m gpu: known answers for the header-level primitives, DEVICE run.  The same program and the same cases as tests/test_arith_kat_host.py, run by
one kernel instantiation per primitive (one case per lane, or per quad for the four-lane addition), plus the primitives that exist on the device
only: xyzzw_export, a store_xyzzw / load_xyzzw round trip through global memory (and the memory image it leaves), xyzzw_add_dist on the cases of the
lane-wise addition, quad_distribute + quad_gather from each lane of the quad, and the three scalar multiplications of the G1 inverse NTT
(g1_mul_dev.h: g1_mul_scalar, g1_mul_scalar_iso, g1_mul_scalar_iso8, with the dynamic LDS their production kernel launches with) on bases as the
transform's load and its earlier stages leave them and on directed scalars (tests/gen/arith_cases.py: mul_scalars).  Every device result is compared with the integer model of
tests/gen/arith_cases.py, and with the host build's result LIMB FOR LIMB: the lazy results are not unique as residues, but they are deterministic
functions of their inputs, so the two builds of one function must agree exactly (PLK_CHAIN, the out-of-line product of ec_dev.h and the AMDGPU
backend's multiply-add and carry sequences are device-only code).  All comparisons are exact."""
import shutil

import pytest

from tests.gen import arith_cases as ac
from tests.test_arith_kat_host import COVERAGE as HOST_COVERAGE, DEVICE_ONLY

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")]

COVERAGE = sorted(HOST_COVERAGE + [(n, 1) for n in DEVICE_ONLY])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("arith_kat_gpu"))
    exe = ac.build_program(work)
    groups = ac.generate(device=True)
    dev, summary = ac.run_program(exe, groups, work, host=False)
    host_groups = [g for g in groups if not g.device_only]
    host, _ = ac.run_program(exe, host_groups, work, host=True)
    return groups, dev, dict(((g.name, g.field), o) for g, o in zip(host_groups, host)), summary


def test_every_primitive_has_cases(runs):
    groups, dev, host, summary = runs
    assert sorted((g.name, g.field) for g in groups) == COVERAGE == ac.expected_coverage(device=True)
    assert sorted(host) == HOST_COVERAGE
    for g in groups:                                                         # (a chain case is 32 dependent operations)
        assert len(g.cases) * (ac.CHAIN_STEPS if g.name == "E_XYZZW_CHAIN" else 1) >= ac.RANDOM_CASES, (g.name, len(g.cases))
    assert "%d groups, %d cases on the device" % (len(groups), sum(len(g.cases) for g in groups)) in summary, summary


@pytest.mark.parametrize("name,field", COVERAGE, ids=["%s-%s" % (n, ac.FIELD_NAME[f]) for n, f in COVERAGE])
def test_device_results_equal_the_integer_model_and_the_host_build(runs, name, field):
    groups, dev, host, _ = runs
    (g, o), = [(g, o) for g, o in zip(groups, dev) if (g.name, g.field) == (name, field)]
    assert len(o) == len(g.cases)                                            # generated == run ...
    assert ac.check_group(g, o) == len(g.cases)                              # ... == checked
    if name in DEVICE_ONLY:
        return
    h = host[(name, field)]
    assert len(h) == len(o)
    for idx, (a, b) in enumerate(zip(o, h)):
        assert a == b, "%s<%s> case %d: device %s != host %s\n  operands: %s" % (name, ac.FIELD_NAME[field], idx, ac.hexw(a), ac.hexw(b), ac.describe_inputs(g, g.cases[idx]))


def test_the_three_scalar_multiplications_agree_as_points(runs):
    """same cases, three window tables (XYZZ; four and eight effectively affine entries on the isomorphic curve): the same point from each"""
    groups, dev, _, _ = runs
    by_name = dict((g.name, (g, o)) for g, o in zip(groups, dev))
    ref_g, ref_o = by_name[ac.MUL_OPS[0]]
    ref_pts = [ac.decode_xyzz(o, ac.R261) for o in ref_o]
    for name in ac.MUL_OPS[1:]:
        g, outs = by_name[name]
        assert g.cases == ref_g.cases
        for idx, o in enumerate(outs):
            got = ac.decode_xyzz(o, ac.R261)
            assert got[1] is None and got == ref_pts[idx], "%s case %d: %s, %s gives %s\n  operands: %s" % (
                name, idx, got, ac.MUL_OPS[0], ref_pts[idx], ac.describe_inputs(g, g.cases[idx]))
