"""The engine's launches and their arguments on the GPU equal, record for record, what the commit
before ``ops.kernels.rule_combine`` issued, and three steps of every case end in the same bits
(``engine_trace.py`` lists the cases and says how the ``golden/engine_trace_gpu.*`` files were
recorded on an MI355X). Same hardware, kernels, arguments and order: no tolerance."""
import os

import pytest
import torch

import engine_trace as ET

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_trace_gpu")


def test_traces_and_final_state_bit_identical_to_parent(cuda):
    want = ET.load_traces(GOLDEN + ".json")
    tensors = torch.load(GOLDEN + ".pt", weights_only=True)
    got, got_tensors = ET.run_world1(cuda)
    assert sorted(got) == sorted(want) and len(want) == 40
    assert sorted(got_tensors) == sorted(tensors) and len(tensors) == 2 * len(want)
    for cid in want:
        assert got[cid], cid
        diff = ET.first_difference(got[cid], want[cid])
        assert diff is None, f"{cid} {diff}"
    for key in sorted(tensors):
        t = got_tensors[key]
        assert t.dtype == tensors[key].dtype and torch.equal(t.flatten(), tensors[key]), key
