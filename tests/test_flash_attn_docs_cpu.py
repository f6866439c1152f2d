"""Document bounds and the document-masked attention fallback on CPU tensors."""
import pytest
import torch
import torch.nn.functional as F

from consensusml_amd.ops.transformer import doc_bounds, flash_attention


@pytest.mark.parametrize("rows", [
    [[5, 5, 2, 2, 2, 5, 9, 9, 0], [3, 3, 3, 3, 3, 3, 3, 3, 3]],   # unsorted, repeated; one run
    [[7]],                                                         # S = 1
    [[0, 1, 2, 3], [4, 4, 4, 1]],
])
def test_doc_bounds_cpu_vs_loop(rows):
    lo, hi = doc_bounds(torch.tensor(rows))
    assert lo.dtype == hi.dtype == torch.int32
    for b, r in enumerate(rows):
        s = 0
        while s < len(r):
            e = s
            while e < len(r) and r[e] == r[s]:
                e += 1
            assert lo[b, s:e].tolist() == [s] * (e - s) and hi[b, s:e].tolist() == [e] * (e - s)
            s = e


def test_fallback_vs_per_document_sdpa():
    torch.manual_seed(0)
    lens, H, KV = (1, 30, 39), 4, 2
    q, k, v = (torch.randn(2, h, 70, 128) for h in (H, KV, KV))
    ids = torch.repeat_interleave(torch.arange(3), torch.tensor(lens)).expand(2, 70)
    o = flash_attention(q, k, v, bounds=doc_bounds(ids))
    s0 = 0
    for n in lens:
        sl = slice(s0, s0 + n)
        ref = F.scaled_dot_product_attention(q[:, :, sl], k[:, :, sl], v[:, :, sl], is_causal=True,
                                             enable_gqa=True)
        torch.testing.assert_close(o[:, sl], ref.transpose(1, 2).reshape(2, n, H * 128),
                                   rtol=1e-5, atol=1e-5)
        s0 += n


def test_bounds_are_causal_only():
    q = torch.randn(1, 2, 8, 128)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal=False, bounds=doc_bounds(torch.zeros(1, 8).long()))
