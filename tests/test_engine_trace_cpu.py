"""The engine's launches, their arguments and the collectives between them on CPU equal, record
for record, what the commit before ``ops.kernels.rule_combine`` issued (``engine_trace.py`` lists
the cases and says how ``golden/engine_trace_cpu.json`` was recorded)."""
import os

import pytest
import torch

import engine_trace as ET

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "engine_trace_cpu.json")


@pytest.fixture(scope="module")
def want():
    return ET.load_traces(GOLDEN)


def _compare(got, want, ids):
    assert sorted(got) == sorted(ids)
    for cid in ids:
        assert got[cid], cid
        diff = ET.first_difference(got[cid], want[cid])
        assert diff is None, f"{cid} {diff}"


def test_world1_traces_equal_parent(want):
    got, _ = ET.run_world1(torch.device("cpu"))
    ids = [c for c in want if not c.startswith("w2-")]
    assert len(ids) == 40
    _compare(got, want, ids)


def test_world2_traces_equal_parent(want, tmp_path):
    got = ET.run_world2(tmp_path)
    ids = [c for c in want if c.startswith("w2-")]
    assert len(ids) == 2 * len(ET.WORLD2_CASES) == 8
    _compare(got, want, ids)
    for cid in ids:     # both ranks issued collectives
        assert any(r["fn"].startswith("dist.") for r in got[cid]), cid
