"""``fused_qkv_attention(..., lens=...)`` on CPU fp32 (qkv_split + SDPA under a key-padding mask)
against plain softmax(Q K^T) V on each sequence's unpadded slice."""
import math

import pytest
import torch

from consensusml_amd.ops.transformer import fused_qkv_attention

H, S, LENS = 2, 37, (37, 1, 20)


def _plain(x, causal):
    """x [n, 3 H 64] fp32 -> [n, H 64]."""
    n = x.shape[0]
    q, k, v = x.view(n, 3, H, 64).permute(1, 2, 0, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(64)
    if causal:
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), float("-inf"))
    return torch.matmul(torch.softmax(s, -1), v).transpose(0, 1).reshape(n, H * 64)


@pytest.mark.parametrize("causal", [False, True])
def test_lens_cpu_vs_per_sequence(causal):
    torch.manual_seed(0)
    qkv = torch.randn(len(LENS), S, 3 * H * 64)
    do, x = torch.randn(len(LENS), S, H * 64), qkv.clone().requires_grad_()
    o = fused_qkv_attention(x, H, 64, causal, lens=torch.tensor(LENS, dtype=torch.int32))
    o.backward(do)
    for b, n in enumerate(LENS):
        xr = qkv[b, :n].clone().requires_grad_()
        ref = _plain(xr, causal)
        ref.backward(do[b, :n])
        torch.testing.assert_close(o[b, :n], ref, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(x.grad[b, :n], xr.grad, rtol=1e-4, atol=1e-5)
        assert (o[b, n:] == 0).all() and (x.grad[b, n:] == 0).all()
