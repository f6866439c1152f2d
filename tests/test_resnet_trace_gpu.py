"""The bottleneck's native launches, library convs / GEMMs and the tensors wired between them
equal, record for record, what the commit before the 3x3 Functions and
``Bottleneck._forward_fused`` were folded issued (``resnet_trace.py`` lists the cases and says how
``golden/resnet_trace_gpu.json`` was recorded on an MI355X). No tensor values: no tolerance."""
import os

import pytest
import torch

import resnet_trace as RT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "resnet_trace_gpu.json")


def test_traces_identical_to_parent(cuda):
    want = RT.load_traces(GOLDEN)
    assert sorted(want) == sorted(c[0] for c in RT.case_list()) and len(want) == RT.N_CASES == 69
    assert all(want.values())
    bad = RT.compare_cases(cuda, want)
    assert not bad, f"{len(bad)} cases differ:\n" + "\n".join(bad)


@pytest.mark.parametrize("stride", [1, 2])
def test_fp32_bn1_takes_the_unfused_bn1_rung(cuda, stride):
    """A block whose bn1 has fp32 parameters: ``bn_fwd`` does not take them, so the prologue rung
    (bn1 + ReLU inside the 3x3 Function) is guarded by ``fused_ok`` at both strides and bn1 runs
    as the module; the 3x3 conv stays on the own kernels with the plain data gradient."""
    from consensusml_amd.models.resnet import Bottleneck
    torch.manual_seed(0)
    m = RT.init_bn(Bottleneck(64, 64, stride, True))
    m = m.to(device=cuda, dtype=torch.bfloat16, memory_format=torch.channels_last)
    m.bn1.float()
    gen = torch.Generator(device=cuda).manual_seed(1)
    x = torch.randn(2, 64, 16, 16, device=cuda, generator=gen).relu().bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    recs = RT.run_model(m, x)
    for p in m.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all())
    fns = [r["fn"] for r in recs]
    assert fns.count("lib.conv_gemm_bn") == 1 and "lib.conv_gemm_bnsums" not in fns
    dgrad = [r for r in recs if r["fn"] == ("lib.conv_gemm" if stride == 1
                                            else "lib.conv_gemm_s2dgrad")]
    # the data gradient without bn1's sums: (dy, wr, taps, zero row) / (dy, wr, zero row)
    assert len(dgrad) == 1 and len(dgrad[0]) == 1 + (4 if stride == 1 else 3), dgrad
    # no native call sees bn1's parameters, and the 3x3 conv reads the module BN's output
    used = [v[0] for r in recs for v in r.values() if isinstance(v, list) and v]
    assert "bn1.weight" not in used and "bn1.bias" not in used
    conv2 = recs[fns.index("lib.conv_gemm_bn")]
    assert conv2["a0"][0] == "other", conv2
