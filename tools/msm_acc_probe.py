"""one 2^20-term commitment at a time, 40 times: wall ms and the accumulate bracket (plk_msm_last_kernel_ms), median and min: python tools/msm_acc_probe.py"""
import os, sys, time
sys.path.insert(0, os.path.abspath(os.environ.get("PLK_AB_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # PLK_AB_ROOT=ab_old: tools/ab_build.sh
import numpy as np, torch
import plonkit_amd as pa
log_n, reps = 20, 40
ctx = pa.Context(0)
ctx.srs_generate(1 << log_n, 0, 42)
rng = np.random.default_rng(11)
a = rng.integers(0, 1 << 62, size=(1 << log_n, 4), dtype=np.uint64); a[:, 3] &= np.uint64((1 << 60) - 1)
t = torch.from_numpy(a.view(np.int64)).to("cuda:0")
torch.cuda.synchronize()
ctx.set_kernel_timing(True)
for _ in range(8): first = ctx.msm_dev(t, 1 << log_n)
wall, acc = [], []
for _ in range(reps):
    t0 = time.perf_counter(); ctx.msm_dev(t, 1 << log_n); wall.append((time.perf_counter() - t0) * 1e3); acc.append(ctx.msm_last_kernel_ms())
wall.sort(); acc.sort()
print("msm 2^20 over %d: wall median %.4f ms min %.4f | accumulate median %.4f ms min %.4f | fp %s" % (reps, wall[reps // 2], wall[0], acc[reps // 2], acc[0], hex(int(np.asarray(first).ravel()[0]))), flush=True)
