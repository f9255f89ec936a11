"""commitments against caller-supplied bases (plk_msm_g1_bases_dev) beside the resident-key path, one process, one GPU: the numbers of
DESIGN.md section 4.2c and profiles/msm_bases_path.txt.  Every call timed here is synchronous (it ends in a stream synchronise), so the host
clock around it is the call's time; medians of REPS calls after WARM warm-up calls.
  python tools/msm_bases_probe.py [log_n ...]        the table (default 12 16 20 24) and the two key checks at 2^20 points
  python tools/msm_bases_probe.py front [log_n]      only bases-path calls, unchecked then checked: run it under a kernel trace
                                                     (rocprofv3 --kernel-trace --stats -- python ...) to read bases_to_w_kernel's own time"""
import os, statistics, sys, time
sys.path.insert(0, os.path.abspath(os.environ.get("PLK_AB_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import plonkit_amd as pa

WARM, REPS = 3, 20
dev = torch.device("cuda:0")


def timed(fn, warm=WARM, reps=REPS):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def scalars(n, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    s = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device=dev, generator=g); s[:, 3] &= (1 << 60) - 1
    torch.cuda.synchronize()
    return s


def points(n):
    """42^j G, j < n, in a buffer of the caller's (generated as a key on a context that is closed again)"""
    c = pa.Context(0)
    c.srs_generate(n, 0, 42)
    p = torch.from_numpy(c.srs_download(0, n).view(np.int64)).to(dev)
    torch.cuda.synchronize()
    c.close()
    return p


def front_only(log_n):
    n = 1 << log_n
    p, s = points(n), scalars(n, log_n)
    c = pa.Context(0)
    for check in (False, True):
        med, lo, hi = timed(lambda: c.msm_bases_dev(p, s, n, check=check))
        print("2^%d terms, bases path, check=%s: %.3f ms (min %.3f max %.3f); front kernel traffic 128 B/point = %.1f MiB per call"
              % (log_n, check, med, lo, hi, 128.0 * n / 2 ** 20), flush=True)
    c.close()


def table(logs):
    nmax = 1 << max(logs + [20])
    p = points(nmax)
    print("terms | bases path | bases path, checked | resident key, table built | first commitment on a fresh key (once) | shape of the bases pass")
    for log_n in logs:
        n = 1 << log_n
        s = scalars(n, log_n)
        c = pa.Context(0)                                          # no key
        plain = timed(lambda: c.msm_bases_dev(p, s, n))
        shape = c.msm_last_shape()
        checked = timed(lambda: c.msm_bases_dev(p, s, n, check=True))
        c.close()
        k = pa.Context(0)
        k.srs_generate(n, 0, 42)
        k.synchronize()
        t0 = time.perf_counter()
        first_point = k.msm_dev(s, n)
        first = (time.perf_counter() - t0) * 1e3
        resident = timed(lambda: k.msm_dev(s, n))
        kshape = k.msm_last_shape()
        k.close()
        c = pa.Context(0)
        assert np.array_equal(c.msm_bases_dev(p, s, n), first_point), "the two paths disagree"
        c.close()
        print("2^%-2d | %8.3f ms (%.3f-%.3f) | %8.3f ms | %8.3f ms (%.3f-%.3f; %s, %d copies) | %9.3f ms | c=%d, %d sets, variant %d, %d lanes, %s"
              % (log_n, plain[0], plain[1], plain[2], checked[0], resident[0], resident[1], resident[2], kshape["path"], kshape["table_copies"], first,
                 shape["window_bits"], shape["bucket_sets"], shape["accumulate_variant"], shape["reduce_lanes"], shape["path"]), flush=True)
    # the two key checks at 2^20 points: a fresh context each time for plk_srs_check (its first commitment builds the table), then repeated
    n = 1 << 20
    g2, seed = pa.crs42_g2_bytes(), bytes(range(32))
    cand = p[:n]
    fresh = []
    for _ in range(3):
        k = pa.Context(0)
        k.srs_generate(n, 0, 42)
        k.synchronize()
        t0 = time.perf_counter()
        assert k.srs_check(g2, seed=seed) == (True, None)
        fresh.append((time.perf_counter() - t0) * 1e3)
        again = timed(lambda: k.srs_check(g2, seed=seed), warm=1, reps=5)
        k.close()
    c = pa.Context(0)
    t0 = time.perf_counter()
    assert c.srs_check_points_dev(cand, n, g2, seed=seed) == (True, None)
    first_points = (time.perf_counter() - t0) * 1e3
    pts = timed(lambda: c.srs_check_points_dev(cand, n, g2, seed=seed), warm=1, reps=REPS)
    c.close()
    print("key check at 2^20 points: srs_check on a fresh context %.1f ms (median of 3; table build included), repeated %.2f ms; "
          "srs_check_points_dev first call %.1f ms, repeated %.2f ms (%.2f-%.2f)" % (statistics.median(fresh), again[0], first_points, pts[0], pts[1], pts[2]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "front":
        front_only(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    else:
        table([int(a) for a in sys.argv[1:]] or [12, 16, 20, 24])
