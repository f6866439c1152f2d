"""bench.py's driver contract (one JSON line on rank 0 with the required keys), at a tiny shape:
1 rank with the virtual-worker Krum block (--full), a plain 1-rank run with --dump-outputs, and
2 ranks sharing cuda:0 over gloo (the N > 1 fields: dist_backend, world_size_seen,
replicas_identical, engine_step_ms)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int, "warmup": int,
        "ms_per_step": float, "higher_is_better": bool, "scaling": str, "dtype": str,
        "data": str, "config": dict}
PLAIN = ["--batch", "16", "--image-size", "64", "--steps", "2", "--warmup", "1",
         "--no-miopen-find"]
SMALL = [*PLAIN, "--full", "--b256-batch", "8", "--b256-steps", "2"]


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _json_line(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def _check_headline(r: dict, n: int):
    for k, t in KEYS.items():
        assert k in r and isinstance(r[k], t), (k, r.get(k))
    assert "vs_baseline" in r
    assert r["n_gpus"] == n and r["steps"] == 2 and r["warmup"] == 1
    assert r["value"] > 0 and r["ms_per_step"] > 0 and r["higher_is_better"] is True
    for k in ("model", "global_batch", "seq_len", "parallelism"):
        assert k in r["config"]
    assert r["config"]["global_batch"] == 16 * n


def _check(r: dict, n: int):
    _check_headline(r, n)
    assert r["full"] is True
    # the communication-visible small-batch block (here batch 8 per rank)
    for k in ("b256_samples_per_s", "b256_ms_per_step", "b256_allreduce_ms_per_step",
              "b256_agg_overhead_vs_allreduce", "b256_engine_step_ms"):
        assert isinstance(r[k], float), (k, r.get(k))
    assert r["b256_config"]["global_batch"] == 8 * n and r["b256_loss_finite"] is True


def test_bench_single_rank_contract(cuda):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "bench.py", *SMALL, "--virtual-batch", "8",
                          "--virtual-steps", "2"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = _json_line(out.stdout)
    _check(r, 1)
    assert r["krum_n8_virtual_config"]["workers"] == 8 and r["krum_n8_virtual_config"]["f"] == 2
    assert r["krum_n8_virtual_loss_finite"] is True


def test_bench_plain_run_and_dump(cuda, tmp_path):
    """Without --full only the headline run is timed (no baseline, virtual-worker or batch-256
    keys), and --dump-outputs writes the last timed step's outputs as float .npy files."""
    import numpy as np
    env = dict(os.environ, PYTHONPATH=ROOT)
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *PLAIN, "--dump-outputs",
                          str(d)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = _json_line(out.stdout)
    _check_headline(r, 1)
    assert r["full"] is False and r["allreduce_ms_per_step"] is None
    assert not [k for k in r if k.startswith(("b256_", "krum_n8_virtual"))]
    assert "mean/allreduce" not in out.stderr and "V=8" not in out.stderr
    assert sorted(p.name for p in d.iterdir()) == ["agg_weights.npy", "buffers.npy", "loss.npy",
                                                   "params.npy"]
    arrs = {p.stem: np.load(p) for p in d.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 10**6
    assert arrs["loss"].shape == (1,) and np.isfinite(arrs["loss"]).all()
    assert arrs["params"].size == min(r["config"]["params"], 4 * 2**20)
    assert np.isfinite(arrs["params"]).all() and np.abs(arrs["params"]).max() > 0
    assert arrs["agg_weights"].shape == (1,) and arrs["agg_weights"][0] > 0
    assert arrs["buffers"].size > 0 and np.isfinite(arrs["buffers"]).all()


def test_bench_two_ranks_gloo_contract(cuda):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2",
           "--dist-backend", "gloo", *SMALL]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    r = _json_line(out.stdout)
    _check(r, 2)
    assert r["dist_backend"] == "gloo" and r["world_size_seen"] == 2
    assert r["replicas_identical"] is True and r["engine_step_ms"] >= 0
    assert r["b256_replicas_identical"] is True
