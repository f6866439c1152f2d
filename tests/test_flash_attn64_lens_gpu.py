"""Per-sequence lengths in the head-dim-64 flash kernels (csrc/kernels/flash_attn64.hip, the VL
instantiations) against the fp32 softmax(Q K^T) V oracle of test_flash_attn64_gpu.py applied to
each sequence's unpadded slice, errors taken per sequence; padded rows of qkv and dO hold NaN."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from consensusml_amd.ops.native import lib  # noqa: E402
from consensusml_amd.ops.transformer import fused_qkv_attention  # noqa: E402

SCALE = 1.0 / math.sqrt(64)


def _ref(x, H, causal):
    """fp32 attention on one sequence x [n, 3 H 64]: (o [n, H 64], log2 lse [H, n])."""
    n = x.shape[0]
    q, k, v = x.view(n, 3, H, 64).permute(1, 2, 0, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if causal:
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool, device=x.device).triu(1), float("-inf"))
    o = torch.matmul(torch.softmax(s, -1), v).transpose(0, 1).reshape(n, H * 64)
    return o, torch.logsumexp(s, -1) / math.log(2.0)


def _inputs(H, S, lens, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn(len(lens), S, 3 * H * 64, device="cuda", generator=g).bfloat16()
    do = torch.randn(len(lens), S, H * 64, device="cuda", generator=g).bfloat16()
    return qkv, do, torch.tensor(lens, dtype=torch.int32, device="cuda")


CASES = [  # H, S, lens, nq (2: the 256-query forward, forced, forward only), causal
    # on / next to every 64 / 128 boundary, three tiles, BH % 8 != 0
    *[(3, 384, (1, 64, 129, 192, 257, 384), 0, c) for c in (False, True)],
    *[(4, 256, (130, 256), 0, c) for c in (False, True)],   # BH = 8: the XCD remap picks the batch
    (4, 128, (128, 37), 0, False),                          # lens=None would go to attention.hip
    # a length inside the first half of a 256-query block and one a row past a block
    *[(3, 600, (600, 100, 257), 2, c) for c in (False, True)],
]


@pytest.mark.parametrize("H,S,lens,nq,causal", CASES)
def test_lens_vs_fp32_per_sequence(H, S, lens, nq, causal):
    """A gradient section whose reference is exactly zero (dq, dk of a one-token sequence) has no
    relative error: every section's error is taken against max(its reference norm, 1e-3 of the
    sequence's whole reference gradient), which is the plain relative error everywhere else."""
    qkv, do, lt = _inputs(H, S, lens)
    for b, n in enumerate(lens):
        qkv[b, n:] = do[b, n:] = float("nan")
    o, lse = lib().flash64_fwd(qkv, H, causal, SCALE, 8.0, nq, lens=lt)
    outs = [o, lse]
    if nq == 0:
        x = qkv.clone().requires_grad_()
        fused_qkv_attention(x, H, 64, causal, lens=lt).backward(do)
        outs.append(x.grad)
    assert all(torch.isfinite(t.float()).all() for t in outs)
    for b, n in enumerate(lens):
        assert all((t[b, n:] == 0).all() for t in outs[::2]) and (lse[b, :, n:] == 0).all()
        xr = qkv[b, :n].float().requires_grad_()
        ro, rl = _ref(xr, H, causal)
        errs = {"o": ((o[b, :n].float() - ro).norm() / ro.norm()).item()}
        lerr = (lse[b, :, :n] - rl).abs().max().item()
        if nq == 0:
            ro.backward(do[b, :n].float())
            floor = 1e-3 * xr.grad.norm()
            for j, name in enumerate(("dq", "dk", "dv")):
                sl = slice(j * H * 64, (j + 1) * H * 64)
                errs[name] = ((x.grad[b, :n, sl].float() - xr.grad[:, sl]).norm()
                              / torch.maximum(xr.grad[:, sl].norm(), floor)).item()
        print(f"len {n}: lse {lerr:.2e}", {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) < 1e-2 and lerr < 1e-3, (n, errs, lerr)


@pytest.mark.parametrize("H,S,causal", [(4, 1000, True), (3, 384, False)])
def test_full_lengths_bit_identical(H, S, causal):
    """lens all equal to S: the variant keeps the summation order of the kernels without it."""
    qkv, do, lt = _inputs(H, S, (S, S), seed=1)
    o, lse = lib().flash64_fwd(qkv, H, causal, SCALE)
    ol, lsel = lib().flash64_fwd(qkv, H, causal, SCALE, lens=lt)
    assert torch.equal(o, ol) and torch.equal(lse, lsel)
    assert torch.equal(lib().flash64_bwd(qkv, o, do, lse, H, causal, SCALE),
                       lib().flash64_bwd(qkv, o, do, lse, H, causal, SCALE, lens=lt))


def test_bert_layer_lens(monkeypatch):
    """A padded batch through a BertLayer equals each sequence run alone, without SDPA."""
    from consensusml_amd.models.transformer import BertConfig, BertLayer
    calls = []
    orig = torch.nn.functional.scaled_dot_product_attention
    monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention",
                        lambda *a, **k: calls.append(1) or orig(*a, **k))
    torch.manual_seed(0)
    layer = BertLayer(BertConfig(d=256, heads=4, ffn=512)).cuda().bfloat16()
    x = torch.randn(2, 256, 256, device="cuda").bfloat16()
    with torch.no_grad():
        y = layer(x, torch.tensor((256, 131), dtype=torch.int32, device="cuda"))
        for b, n in enumerate((256, 131)):
            ref = layer(x[b:b + 1, :n])[0].float()
            assert ((y[b, :n].float() - ref).norm() / ref.norm()).item() < 1e-2, n
    assert not calls
