"""``fused_qkv_attention(..., causal=True)`` off the GPU: the fp32 CPU composition against a plain
masked softmax(Q K^T) V."""
import math

import pytest
import torch

from consensusml_amd.ops.transformer import fused_qkv_attention


@pytest.mark.parametrize("causal", [False, True])
def test_fused_qkv_attention_causal_cpu(causal):
    torch.manual_seed(0)
    B, S, H, hd = 2, 37, 3, 64
    qkv = torch.randn(B, S, 3 * H * hd)
    q, k, v = qkv.view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    want = torch.matmul(torch.softmax(s, -1), v).transpose(1, 2).reshape(B, S, H * hd)
    torch.testing.assert_close(fused_qkv_attention(qkv, H, hd, causal=causal), want,
                               rtol=1e-4, atol=1e-5)
