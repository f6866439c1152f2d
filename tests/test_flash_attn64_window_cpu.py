"""The sliding-window keyword of flash_attention on the SDPA fallback (CPU tensors): the mask
max(lo[b, i], i - W + 1) <= j <= i against an explicit fp64 softmax, and the argument errors."""
import math

import pytest
import torch

from consensusml_amd.ops.transformer import flash_attention

B, H, KV, S, HD = 2, 4, 2, 12, 16


def _qkv():
    g = torch.Generator().manual_seed(0)
    return (torch.randn(B, H, S, HD, generator=g), torch.randn(B, KV, S, HD, generator=g),
            torch.randn(B, KV, S, HD, generator=g))


def _ref(q, k, v, W, lo=None):
    pos = torch.arange(S)
    first = (pos - W + 1).clamp_min(0).expand(B, S)
    if lo is not None:
        first = torch.maximum(first, lo.long())
    seen = (first[:, :, None] <= pos) & (pos <= pos[:, None])            # [B, S, S]
    s = q.double() @ k.double().repeat_interleave(H // KV, 1).transpose(-1, -2) / math.sqrt(HD)
    p = torch.softmax(s.masked_fill(~seen[:, None], float("-inf")), -1)
    return (p @ v.double().repeat_interleave(H // KV, 1)).transpose(1, 2).reshape(B, S, H * HD)


@pytest.mark.parametrize("W,docs", [(1, False), (5, False), (S, False), (5, True)])
def test_window_fallback_mask(W, docs):
    q, k, v = _qkv()
    lo = hi = None
    if docs:   # documents [0, 7) and [7, 12): the window and the document start combine
        lo = torch.tensor([0] * 7 + [7] * 5, dtype=torch.int32).expand(B, S)
        hi = torch.tensor([7] * 7 + [12] * 5, dtype=torch.int32).expand(B, S)
    o = flash_attention(q, k, v, window=W, bounds=(lo, hi) if docs else None)
    assert (o.double() - _ref(q, k, v, W, lo)).abs().max().item() < 1e-5


def test_window_errors():
    q, k, v = _qkv()
    with pytest.raises(ValueError):
        flash_attention(q, k, v, window=0)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, causal=False, window=4)
