"""Robustness outcomes with worker-side momentum (``optim.worker_momentum``) in the setting of
``test_robustness.py`` / ``test_nnm_robustness.py``: mlp, n = 8 virtual workers, 2 Byzantine
from step 0, 150 steps, seed 2019. The rule sees momenta, whose variance is reduced over the
momentum window, instead of raw mini-batch gradients. Thresholds sit between the server-momentum
and the worker-momentum outcome of each cell (CPU, fp32: accuracy server -> worker)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "bench"))
from robustness import run_one  # noqa: E402

STEPS = 150
CPU = torch.device("cpu")


def _run(rule, attack, wm=True, pre="none", device=CPU):
    return run_one("mlp", rule, attack, n=8, f=2, steps=STEPS, device=device, pre=pre,
                   worker_momentum=wm)


def test_krum_ipm_survives_with_worker_momentum():
    """0.038 -> 0.741 (other seeds 0.757 / 0.763)."""
    r = _run("krum", "ipm")
    assert r["worker_momentum"] is True
    assert not r["diverged"]
    assert r["eval_accuracy"] > 0.5, r
    plain = _run("krum", "ipm", wm=False)
    assert "worker_momentum" not in plain
    assert plain["eval_accuracy"] < 0.5, plain


def test_krum_clean_gains_from_worker_momentum():
    """0.830 -> 0.897: clean Krum keeps one row, and that row is now a momentum."""
    r = _run("krum", "none")
    plain = _run("krum", "none", wm=False)
    assert r["eval_accuracy"] >= plain["eval_accuracy"] + 0.03, (r, plain)


@pytest.mark.parametrize("rule", ["median", "geomed"])
def test_alie_loses_its_cover(rule):
    """median 0.885 -> 0.931, geomed 0.872 -> 0.930."""
    r = _run(rule, "alie")
    assert not r["diverged"]
    assert r["eval_accuracy"] > 0.9, r


def test_krum_nnm_ipm_with_worker_momentum():
    """krum + nnm / ipm: 0.899 -> 0.928."""
    r = _run("krum", "ipm", pre="nnm")
    assert r["pre"] == "nnm" and r["worker_momentum"] is True
    assert not r["diverged"]
    assert r["eval_accuracy"] > 0.85, r


@pytest.mark.gpu
def test_gpu_krum_ipm_survives_with_worker_momentum(cuda):
    """The krum / ipm cell on the HIP kernels (bf16 rows, fp32 worker state): measured 0.750
    (server momentum 0.056), profiles/worker_momentum/README.md."""
    r = _run("krum", "ipm", device=cuda)
    print(r)
    assert r["dtype"] == "bf16" and r["worker_momentum"] is True and not r["diverged"]
    assert r["eval_accuracy"] > 0.5, r
