"""MeaMed and Phocas in the robustness benchmark (bench/robustness.py), as test_robustness.py does
for the other coordinate rules: n = 8 virtual workers, 2 Byzantine from step 0, 150 steps, MLP
on a learnable teacher task. The clean / ALIE / IPM cells and the resnet_tiny tables are recorded
in profiles/meamed/README.md, not asserted."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "bench"))
from robustness import ALL_RULES, NEAR_RULES, RULES, markdown, run_one  # noqa: E402

STEPS = 150
CPU = torch.device("cpu")


def test_rule_tuples():
    assert NEAR_RULES == ("meamed", "phocas")
    assert set(ALL_RULES) == set(RULES) | set(NEAR_RULES) and len(ALL_RULES) == len(RULES) + 2
    assert not set(RULES) & set(NEAR_RULES)          # the first tuple keeps its length


@pytest.mark.parametrize("rule", NEAR_RULES)
@pytest.mark.parametrize("attack", ["sign_flip", "scaled"])
def test_near_rules_bounded(rule, attack):
    """The bar test_robustness.py::test_robust_rules_bounded sets for the coordinate rules."""
    r = run_one("mlp", rule, attack, n=8, f=2, steps=STEPS, device=CPU)
    print(rule, attack, r["eval_accuracy"], r["final_train_loss"], r["initial_loss"])
    assert not r["diverged"]
    assert r["eval_accuracy"] > 0.8, r
    assert r["final_train_loss"] < 0.5 * r["initial_loss"], r
    md = markdown([r])
    assert f"| {rule} |" in md


@pytest.mark.gpu
def test_gpu_near_rules_cells(cuda):
    """The same outcomes on the HIP kernels (bf16 rows: the fp32 network of the nearest-to-centre
    combine, multi-segment launches of the sharded engine)."""
    for rule in NEAR_RULES:
        r = run_one("mlp", rule, "sign_flip", n=8, f=2, steps=STEPS, device=cuda)
        assert not r["diverged"] and r["eval_accuracy"] > 0.8, r
        assert r["final_train_loss"] < 0.5 * r["initial_loss"], r
