"""Robustness outcomes with nearest-neighbour mixing (``agg.pre=nnm``) in the setting of
``test_robustness.py``: mlp, n = 8 virtual workers, 2 Byzantine from step 0, 150 steps. Plain
Krum is broken by IPM (``test_robustness.py::test_krum_ipm_known_failure``); on the mixed rows
the two colluders are no longer each other's whole neighbourhood."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "bench"))
from robustness import run_one  # noqa: E402

STEPS = 150
CPU = torch.device("cpu")


def _run(rule, attack, pre="nnm", device=CPU):
    return run_one("mlp", rule, attack, n=8, f=2, steps=STEPS, device=device, pre=pre)


def test_nnm_krum_survives_ipm():
    r = _run("krum", "ipm")
    assert r["pre"] == "nnm" and "byzantine_selected_frac" not in r
    assert not r["diverged"]
    assert r["eval_accuracy"] > 0.8, r
    assert r["final_train_loss"] < 0.5 * r["initial_loss"], r


def test_nnm_krum_clean_no_worse_than_plain_krum():
    mixed = _run("krum", "none")
    plain = _run("krum", "none", pre="none")
    assert "pre" not in plain and "byzantine_selected_frac" in plain
    assert mixed["eval_accuracy"] >= plain["eval_accuracy"], (mixed, plain)


@pytest.mark.parametrize("attack", ["sign_flip", "alie"])
def test_nnm_trimmed_mean_bounded(attack):
    r = _run("trimmed_mean", attack)
    assert not r["diverged"]
    assert r["eval_accuracy"] > 0.8, r


@pytest.mark.gpu
def test_gpu_nnm_krum_survives_ipm(cuda):
    """The krum / ipm cell on the HIP kernels (bf16 rows)."""
    r = _run("krum", "ipm", device=cuda)
    print(r)
    assert r["dtype"] == "bf16" and not r["diverged"]
    assert r["eval_accuracy"] > 0.8, r
