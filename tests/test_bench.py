"""bench.py: the plain headline line, --full, and --dump-outputs (what the last timed step returned, written as .npy)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from custom_op_benchmark_amd import graphs
from util import oracle_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_stays_in_budget_and_samples_the_same_rows_every_time(tmp_path):
    """Arrays within their share of the budget are written whole; a larger one as a sorted, seeded sample of its rows
    (the same rows in every run), every file float32 or float64, all files together within the budget."""
    import bench
    n = 50_000
    ids = torch.arange(n, dtype=torch.float64)
    outs = {"rows": ids[:, None].repeat(1, 8).float(),          # 1.6 MB: sampled under a 1 MB budget
            "edges": ids.clone(),                              # 0.4 MB of fp64: sampled
            "small": torch.full((10, 3), 0.25, dtype=torch.float16)}
    budget = 1 << 20
    written = [bench.dump_outputs(outs, str(tmp_path / r), budget=budget) for r in ("a", "b")]
    assert written[0] == written[1]
    total = 0
    for name, t in outs.items():
        a, b = (np.load(str(tmp_path / r / (name + ".npy"))) for r in ("a", "b"))
        assert np.array_equal(a, b)
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32)
        assert a.shape[1:] == tuple(t.shape[1:]) and a.shape[0] == written[0][name]
        total += os.path.getsize(str(tmp_path / "a" / (name + ".npy")))
        if name == "small":
            assert np.array_equal(a, t.float().numpy())
            continue
        rows = a[:, 0] if a.ndim == 2 else a
        assert 0 < a.shape[0] < n and np.all(np.diff(rows) > 0)           # sorted, distinct rows
        assert np.array_equal(a, t.numpy()[rows.astype(np.int64)])         # each one the source's row
    assert total <= budget


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_bench_line_and_dumped_outputs_match_the_oracle(dev, tmp_path, full):
    """A plain run prints the headline line only; --full adds the secondary figures.  Either way --dump-outputs holds what
    the last timed step returned (o, dQ, dK, dV, s, a), equal to the oracle on the same seeded graph and inputs."""
    N, E, d = 3000, 60000, 64
    out_dir = str(tmp_path / "outputs")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--graph", "custom", "--nodes", str(N),
           "--edges", str(E), "--d", str(d), "--steps", "3", "--warmup", "1", "--dump-outputs", out_dir]
    r = subprocess.run(cmd + (["--full", "--profile-steps", "1"] if full else []), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    for key in ("roofline", "fused", "cpu_baseline"):
        assert (key in line) == full, key

    # bench.py's inputs: Chung-Lu(alpha 0.5, seed 0) on the device, then Q, K, V, dO ~ U[0,1) from one generator
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=0, chunk_size=32, device=dev).to("cpu")
    gen = torch.Generator(device=dev).manual_seed(1)
    Q, K, V, dO = (torch.rand((N, d), device=dev, generator=gen).cpu() for _ in range(4))
    want = oracle_step(oracle, g, Q, K, V, dO)
    for name in ("o", "dQ", "dK", "dV", "s", "a"):
        got = np.load(os.path.join(out_dir, name + ".npy"))
        assert got.dtype == np.float32
        torch.testing.assert_close(torch.from_numpy(got), want[name], rtol=1e-4, atol=1e-5, msg=lambda m: name + ": " + m)
