"""-m gpu: key files decoded, curve-checked and encoded by kernels (keyio.hip): Crs::read straight into HBM (plk_srs_load_key),
Crs::write straight out of it (plk_srs_store_key) and the two kernels on device pointers.  Referees: for well-formed keys the
reference's own file tests/golden/setup_2pow10.key and the oracle's read_crs / write_crs; for refused encodings the host
plk_key_parse (pairing_ce's into_affine rules)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import Q_MOD

ERR_ARG, ERR_FORMAT = 1, 6


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def _chunk():
    import plonkit_amd as pa
    return int(pa.lib().plk_key_chunk_points())


def host_parse(raw):
    """the host referee: (status, points or None, n, g2)"""
    import plonkit_amd as pa
    L = pa.lib()
    buf = np.frombuffer(raw, dtype=np.uint8)
    n, g2 = ctypes.c_uint64(0), ctypes.create_string_buffer(256)
    rc = L.plk_key_parse(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(buf.size), None, ctypes.c_uint64(0), ctypes.byref(n), g2)
    if rc != 0:
        return rc, None, n.value, g2.raw
    pts = np.zeros((n.value, 8), dtype=np.uint64)
    rc = L.plk_key_parse(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(buf.size), pts.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n.value), ctypes.byref(n), g2)
    return rc, (pts if rc == 0 else None), n.value, g2.raw


def host_serialize(pts, g2):
    import plonkit_amd as pa
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    ln = ctypes.c_uint64(8 + 64 * pts.shape[0] + 8 + 256)
    out = np.empty(ln.value, dtype=np.uint8)
    assert pa.lib().plk_key_serialize(pts.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(pts.shape[0]), g2, out.ctypes.data_as(ctypes.c_void_p), ln, ctypes.byref(ln)) == 0
    return bytearray(out.tobytes())


def device_status(ctx, raw, **kw):
    """(status, lowest refused index or None) of srs_load_key"""
    import plonkit_amd as pa
    try:
        ctx.srs_load_key(raw, **kw)
        return 0, None
    except pa.PlkError as e:
        return e.code, e.bad_index


@pytest.fixture(scope="module")
def big_points(ctx):
    """2 * chunk + 5 points of crs_42 (a prefix of a key is a key), made and downloaded once"""
    n = 2 * _chunk() + 5
    ctx.srs_generate(n, 0, 42)
    return ctx.srs_download(0, n)


def _golden_raw(golden_dir):
    return open(os.path.join(golden_dir, "setup_2pow10.key"), "rb").read()


# ------------------------------------------------------------------------------------------------ 1
def test_golden_key_loads_stores_and_proves(ctx, golden_dir, golden_crs):
    import plonkit_amd as pa
    raw = _golden_raw(golden_dir)
    n, g2 = ctx.srs_load_key(raw)
    assert n == 1024 and ctx.srs_size() == 1024
    assert g2 == raw[-256:] == golden_crs.g2_raw
    assert np.array_equal(ctx.srs_download(0, 1024), golden_crs.g1)
    assert ctx.srs_store_key(g2) == raw
    circ = pa.Circuit.from_files(os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json"))
    setup = pa.SetupForProver(ctx, circ)
    assert setup.verification_key_bytes(g2) == open(os.path.join(golden_dir, "vk.bin"), "rb").read()
    assert setup.prove(circ) == open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    setup.close(); circ.close()


# ------------------------------------------------------------------------------------------------ 2
def _sizes():
    c = 1 << 20                     # (ids only; the test reads the library's chunk size)
    return [1, 2, 63, 64, 65, 1000, (1 << 16) + 3, "chunk-1", "chunk", "chunk+1", "2*chunk+5"]


@pytest.mark.parametrize("size", _sizes())
def test_sizes_device_load_equals_host_parse_and_store_equals_serialize(ctx, big_points, golden_crs, size):
    c = _chunk()
    assert c <= 1 << 21
    n = {"chunk-1": c - 1, "chunk": c, "chunk+1": c + 1, "2*chunk+5": 2 * c + 5}.get(size, size)
    raw = host_serialize(big_points[:n], golden_crs.g2_raw)
    rc, want, hn, hg2 = host_parse(raw)
    assert rc == 0 and hn == n
    got_n, g2 = ctx.srs_load_key(raw)
    assert got_n == n and ctx.srs_size() == n and g2 == hg2
    assert np.array_equal(ctx.srs_download(0, n), want)
    assert np.array_equal(want, big_points[:n])
    assert ctx.srs_store_key(g2) == bytes(raw)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("where", ["first", "middle", "last", "adjacent"])
def test_infinity_entries_survive_both_directions(ctx, golden_crs, where):
    n = 1000
    pts = golden_crs.g1[:n].copy()
    idx = {"first": [0], "middle": [n // 2], "last": [n - 1], "adjacent": [417, 418]}[where]
    pts[idx] = 0
    raw = bytes(po.write_crs(po.Crs(pts, golden_crs.g2_raw)))
    for i in idx:
        assert raw[8 + 64 * i: 8 + 64 * i + 64] == b"\x40" + b"\x00" * 63
    assert host_parse(raw)[0] == 0
    ctx.srs_load_key(raw)
    assert np.array_equal(ctx.srs_download(0, n), pts)
    assert ctx.srs_store_key(golden_crs.g2_raw) == raw


# ------------------------------------------------------------------------------------------------ 4
def _be(v):
    return int(v).to_bytes(32, "big")


def _refusal_cases(valid):
    """name -> 64 bytes, from a valid point's 64 bytes"""
    x, y = int.from_bytes(valid[:32], "big"), int.from_bytes(valid[32:], "big")
    return {
        "x=q": _be(Q_MOD) + valid[32:],
        "x=q+1": _be(Q_MOD + 1) + valid[32:],
        "y=q": valid[:32] + _be(Q_MOD),
        "x=2^254-1": _be((1 << 254) - 1) + valid[32:],
        "0x80|valid": bytes([valid[0] | 0x80]) + valid[1:],
        "0xC0 00..": b"\xc0" + b"\x00" * 63,
        "0x40 byte63=1": b"\x40" + b"\x00" * 62 + b"\x01",
        "0x41 00..": b"\x41" + b"\x00" * 63,
        "64 zero bytes": b"\x00" * 64,
        "y+1": valid[:32] + _be(y + 1),
        "x<->y": valid[32:] + valid[:32],
        "-y (control: loads)": valid[:32] + _be(Q_MOD - y),
    }


CASES = ["x=q", "x=q+1", "y=q", "x=2^254-1", "0x80|valid", "0xC0 00..", "0x40 byte63=1", "0x41 00..", "64 zero bytes", "y+1", "x<->y", "-y (control: loads)"]


@pytest.fixture(scope="module")
def resident(ctx, golden_dir, golden_crs):
    """what must survive every refusal: the golden key resident, and a commitment against it"""
    rng = np.random.default_rng(11)
    s = rng.integers(0, 1 << 62, size=(64, 4), dtype=np.uint64)
    s[:, 3] &= np.uint64((1 << 60) - 1)
    return s, ol.msm(golden_crs.g1[:64], s)


def _check_resident_untouched(ctx, golden_crs, resident):
    s, want = resident
    assert ctx.srs_size() == 1024
    assert np.array_equal(ctx.srs_download(0, 1024), golden_crs.g1)
    assert np.array_equal(ctx.msm(s), want)


@pytest.mark.parametrize("case", CASES)
def test_refusals_small_key(ctx, golden_dir, golden_crs, resident, case):
    n = 1000
    clean = bytearray(_golden_raw(golden_dir))
    clean = bytearray(struct.pack(">Q", n) + clean[8:8 + 64 * n] + clean[8 + 64 * 1024:])
    assert host_parse(clean)[0] == 0
    ctx.srs_load_key(_golden_raw(golden_dir))
    for at in (0, n // 2, n - 1):
        raw = bytearray(clean)
        raw[8 + 64 * at: 8 + 64 * at + 64] = _refusal_cases(bytes(clean[8 + 64 * at: 8 + 64 * at + 64]))[case]
        want = host_parse(raw)[0]
        assert want == (0 if case.startswith("-y") else ERR_FORMAT), "the referee's verdict (CPU check of the issue)"
        rc, bad = device_status(ctx, raw)
        print("case %-22s at %4d: host %d device %d bad %s" % (case, at, want, rc, bad))
        assert rc == want
        if want:
            assert bad == at
            _check_resident_untouched(ctx, golden_crs, resident)
        else:
            assert ctx.srs_size() == n
            ctx.srs_load_key(_golden_raw(golden_dir))


@pytest.mark.parametrize("case", CASES)
def test_refusals_in_the_second_chunk(ctx, big_points, golden_dir, golden_crs, resident, case):
    c = _chunk()
    n, at = c + 1000, c + 7
    raw = host_serialize(big_points[:n], golden_crs.g2_raw)
    ctx.srs_load_key(_golden_raw(golden_dir))
    raw[8 + 64 * at: 8 + 64 * at + 64] = _refusal_cases(bytes(raw[8 + 64 * at: 8 + 64 * at + 64]))[case]
    want = host_parse(raw)[0]
    assert want == (0 if case.startswith("-y") else ERR_FORMAT)
    rc, bad = device_status(ctx, raw)
    print("case %-22s at %d: host %d device %d bad %s" % (case, at, want, rc, bad))
    assert rc == want
    if want:
        assert bad == at
        _check_resident_untouched(ctx, golden_crs, resident)
    else:
        assert ctx.srs_size() == n


def test_two_refused_points_report_the_lower_index(ctx, big_points, golden_dir, golden_crs, resident):
    c = _chunk()
    n = c + 1000
    ctx.srs_load_key(_golden_raw(golden_dir))
    for lo, hi in ((3, 900), (511, 512), (c - 1, c), (100, c + 500), (c + 1, c + 999)):
        raw = host_serialize(big_points[:n], golden_crs.g2_raw)
        for at, case in ((hi, "y+1"), (lo, "x=q")):
            raw[8 + 64 * at: 8 + 64 * at + 64] = _refusal_cases(bytes(raw[8 + 64 * at: 8 + 64 * at + 64]))[case]
        assert host_parse(raw)[0] == ERR_FORMAT
        assert device_status(ctx, raw) == (ERR_FORMAT, lo)
        _check_resident_untouched(ctx, golden_crs, resident)


# ------------------------------------------------------------------------------------------------ 5
def test_container_errors_match_the_host_parser(ctx, golden_dir, golden_crs, resident):
    raw = _golden_raw(golden_dir)
    ctx.srs_load_key(raw)
    wrong_g2 = bytearray(raw); wrong_g2[8 + 64 * 1024 + 7] = 3
    huge = struct.pack(">Q", (1 << 28) + 1) + raw[8:]
    for name, data in (("7 bytes", raw[:7]), ("truncated body", raw[:30000]), ("truncated G2", raw[:-1]), ("G2 count != 2", bytes(wrong_g2)), ("n = 2^28 + 1", huge)):
        want = host_parse(data)[0]
        assert want == ERR_FORMAT, name
        rc, bad = device_status(ctx, data)
        assert rc == want and bad is None, name
        _check_resident_untouched(ctx, golden_crs, resident)


# ------------------------------------------------------------------------------------------------ 6
def test_slices(ctx, golden_dir, golden_crs):
    import plonkit_amd as pa
    raw = _golden_raw(golden_dir)
    for first, count in ((0, 1), (0, 256), (300, 424), (768, 256), (1023, 1), (1000, 0), (0, 0), (0, 1024)):
        n, _ = ctx.srs_load_key(raw, first=first, count=count)
        kept = count if count else 1024 - first
        assert n == 1024 and ctx.srs_size() == kept
        assert np.array_equal(ctx.srs_download(0, kept), golden_crs.g1[first:first + kept])
    for first, count in ((1025, 0), (1000, 25), (0, 1025), (1024, 1), (1 << 63, 1 << 63)):
        with pytest.raises(pa.PlkError) as e:
            ctx.srs_load_key(raw, first=first, count=count)
        assert e.value.code == ERR_ARG
    # a bad point outside the kept slice is refused all the same: Crs::read checks every point
    ctx.srs_load_key(raw, first=0, count=256)
    bad = bytearray(raw)
    bad[8 + 64 * 900 + 63] ^= 1
    assert host_parse(bad)[0] == ERR_FORMAT
    assert device_status(ctx, bad, first=0, count=256) == (ERR_FORMAT, 900)
    assert device_status(ctx, bad, first=950, count=10) == (ERR_FORMAT, 900)
    assert ctx.srs_size() == 256 and np.array_equal(ctx.srs_download(0, 256), golden_crs.g1[:256])


# ------------------------------------------------------------------------------------------------ 7
def test_lagrange_slot_through_encode_and_load_key(ctx, golden_dir, golden_crs):
    import torch
    import plonkit_amd as pa
    raw = _golden_raw(golden_dir)
    ctx.srs_load_key(raw)
    ctx.srs_lagrange_clear()
    circ = pa.Circuit.from_files(os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json"))
    setup = pa.SetupForProver(ctx, circ)
    N = setup.domain_size
    log_n = N.bit_length() - 1
    lag = torch.zeros((N, 8), dtype=torch.int64, device="cuda:0")
    body = torch.zeros(64 * N, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.g1_intt_srs_dev(log_n, lag.data_ptr())
    ctx.g1_encode_dev(lag.data_ptr(), N, body.data_ptr())
    ctx.synchronize()
    file_bytes = struct.pack(">Q", N) + body.cpu().numpy().tobytes() + struct.pack(">Q", 2) + raw[-256:]
    assert np.array_equal(po.read_crs(file_bytes).g1, ol.g1_intt(golden_crs.g1[:N], log_n))
    n, _ = ctx.srs_load_key(file_bytes, lagrange=True)
    assert n == N and ctx.srs_lagrange_size() == N and ctx.srs_size() == 1024
    assert ctx.srs_store_key(raw[-256:], lagrange=True) == file_bytes
    assert setup.prove(circ) == open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    # the same key made resident without leaving the device (what `dump-lagrange` does)
    ctx.srs_lagrange_clear()
    ctx.srs_lagrange_from_powers(log_n)
    assert ctx.srs_store_key(raw[-256:], lagrange=True) == file_bytes
    assert setup.prove(circ) == open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    ctx.srs_lagrange_clear()
    setup.close(); circ.close()


# ------------------------------------------------------------------------------------------------ 8
def test_a_lender_refuses_to_replace_its_key(golden_dir, golden_crs):
    import plonkit_amd as pa
    raw = _golden_raw(golden_dir)
    owner, guest = pa.Context(0), pa.Context(0)
    try:
        owner.srs_load_key(raw)
        guest.share_srs_from(owner)
        with pytest.raises(pa.PlkError) as e:
            owner.srs_upload(golden_crs.g1)
        assert e.value.code == ERR_ARG
        with pytest.raises(pa.PlkError) as e:
            owner.srs_load_key(raw)
        assert e.value.code == ERR_ARG
        assert np.array_equal(owner.srs_download(0, 1024), golden_crs.g1)
        # a borrower that is refused a bad key keeps its loan; one that loads a good key owns it
        bad = bytearray(raw); bad[8 + 63] ^= 1
        assert device_status(guest, bad) == (ERR_FORMAT, 0)
        assert guest.srs_size() == 1024 and np.array_equal(guest.srs_download(0, 1024), golden_crs.g1)
        with pytest.raises(pa.PlkError):
            owner.srs_load_key(raw)
        guest.srs_load_key(raw, first=0, count=512)
        assert guest.srs_size() == 512
        owner.srs_load_key(raw)                             # the loan is returned: the lender may replace its key again
    finally:
        guest.close(); owner.close()


# ------------------------------------------------------------------------------------------------ 9
def test_decode_and_encode_on_torch_streams(ctx, big_points, golden_crs):
    import torch
    import plonkit_amd as pa
    n = 1 << 18
    rng = np.random.default_rng(5)
    pick = rng.choice(big_points.shape[0], size=n, replace=False)
    pts = np.ascontiguousarray(big_points[pick])
    want_body = po.write_crs(po.Crs(pts, golden_crs.g2_raw))[8:8 + 64 * n]
    stream = torch.cuda.Stream(device="cuda:0")
    host = torch.from_numpy(pts.view(np.int64)).pin_memory()
    with torch.cuda.stream(stream):
        d_pts = host.to("cuda:0", non_blocking=True)
        d_bytes = torch.empty(64 * n, dtype=torch.uint8, device="cuda:0")
        d_back = torch.empty((n, 8), dtype=torch.int64, device="cuda:0")
        ctx.g1_encode_dev(d_pts, n, d_bytes, stream=stream)
        ctx.g1_decode_dev(d_bytes, n, d_back, stream=stream)
        same = bool(torch.equal(d_back, d_pts))
        body = d_bytes.cpu().numpy().tobytes()
    assert same, "decode(encode(points)) is not the identity"
    assert body == want_body
    # a refused point through the device entry: the lowest index, whatever the launch geometry
    with torch.cuda.stream(stream):
        d_bytes[64 * 70001 + 63] ^= 1
        d_bytes[64 * 1234 + 5] ^= 1
        with pytest.raises(pa.PlkError) as e:
            ctx.g1_decode_dev(d_bytes, n, d_back, stream=stream)
    stream.synchronize()
    assert e.value.code == ERR_FORMAT and e.value.bad_index == 1234


# ------------------------------------------------------------------------------------------------ 10
def test_binary_refuses_a_key_with_an_off_curve_point(golden_dir, tmp_path):
    """`plonkit prove` on a key file with one off-curve point exits 101 (the Rust panic status) and reports it in the words of
    the build before this feature.  Recorded from that build on the same file (stderr, first line after the progress line
    "Loading circuit from ..." that the main thread prints while the key is being read):
        read key_monomial_form err: read key err: point not on curve (status 6)"""
    import plonkit_amd as pa
    cli = os.path.join(os.path.dirname(pa.lib_path()), "plonkit")
    bad = bytearray(_golden_raw(golden_dir))
    bad[8 + 64 * 700 + 40] ^= 0x10
    key = tmp_path / "bad.key"
    key.write_bytes(bytes(bad))
    circ, wit = os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json")
    r = subprocess.run([cli, "prove", "-m", str(key), "-c", circ, "-w", wit, "-p", str(tmp_path / "proof.bin"), "-j", str(tmp_path / "p.json"),
                        "-i", str(tmp_path / "i.json")], capture_output=True, text=True, timeout=300)
    print(r.stderr)
    assert r.returncode == 101
    lines = [ln for ln in r.stderr.splitlines() if not ln.startswith("Loading circuit from ")]
    assert lines and lines[0] == "read key_monomial_form err: read key err: point not on curve (status 6)"
    assert not (tmp_path / "proof.bin").exists()
    for cmd in (["export-verification-key", "-m", str(key), "-c", circ, "-v", str(tmp_path / "vk.bin")],
                ["dump-lagrange", "-m", str(key), "-c", circ, "-l", str(tmp_path / "lag.key")]):
        r = subprocess.run([cli] + cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 101 and "read key_monomial_form err: read key err: point not on curve (status 6)" in r.stderr
