"""bench.py as the driver runs it.  A plain run (`--gpus 1 --steps K --warmup W`) times the headline region and prints the headline
fields only; `--dump-outputs DIR` writes the commitment of the last timed step, which must be the commitment of the seeded
scalars against the tau = 42 SRS (checked against the CPU oracle).  The secondary legs run with --full (tests/test_gpu_sharded_prove.py)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = {"roofline", "sustained", "value_sustained", "cpu_baseline", "prove", "cli", "cli_ci_shape", "kernels_ms", "strong", "notes"}


def _bench_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_compact_line_of_a_plain_run_has_no_secondary_fields():
    """-m "not gpu": the printed line of a plain run is the headline and `config`, nothing that a --full run measures"""
    bench = _bench_module()
    line = {"metric": "m", "value": 1.0, "unit": "u", "n_gpus": 1, "steps": 3, "warmup": 1, "ms_per_step": 2.0, "higher_is_better": True,
            "dtype": "d", "config": {"terms_per_gpu": 1 << 14, "pipeline_depth": 3, "settle_steps": 0}, "failed_legs": []}
    c = bench.compact_line(line)
    assert {k: c[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype")} == \
        {k: line[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype")}
    assert not SECONDARY & set(c), sorted(SECONDARY & set(c))


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_commitment(tmp_path):
    import torch
    import plonkit_amd as pa
    from oracle import oracle_lib as ol
    log_n, n = 14, 1 << 14
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--log-n", str(log_n),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["steps"] == 5 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "Mscalar·mul/s" and line["dtype"].startswith("u256") and line["config"]["terms_per_gpu"] == n
    assert line["value"] * line["ms_per_step"] == pytest.approx(n / 1e3, rel=1e-2)     # both describe the same K timed steps
    assert not SECONDARY & set(line), sorted(SECONDARY & set(line))
    assert line["failed_legs"] == []
    got = np.load(out / "commitment.npy")
    assert got.dtype == np.float32 and got.shape == (2, 32)
    # the same inputs rebuilt here: bench.py's seeded scalars of rank 0 and the first 2^14 points of the tau = 42 SRS, through the CPU oracle
    bench = _bench_module()
    scalars = bench.rand_scalars(n, bench.SCALAR_SEED, torch.device("cuda", 0)).cpu().numpy().view(np.uint64)
    ctx = pa.Context(0)
    try:
        ctx.srs_generate(n, 0, 42)
        bases = ctx.srs_download(0, n)
    finally:
        ctx.close()
    want = np.frombuffer(pa.g1_to_bytes(ol.msm(bases, scalars)), dtype=np.uint8).reshape(2, 32)
    assert np.array_equal(got.astype(np.uint8), want)
