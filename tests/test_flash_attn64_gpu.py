"""Flash attention for head dim 64 from the fused QKV layout (csrc/kernels/flash_attn64.hip)
against an fp32 softmax(Q K^T) V oracle on the split views of qkv: lengths around every tile and
buffer boundary, both head-count branches of the work remap, causal and full, lse, the deferred
rescale, run-to-run determinism and the dispatch of ``fused_qkv_attention``."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from consensusml_amd import perf  # noqa: E402
from consensusml_amd.ops.native import lib  # noqa: E402
from consensusml_amd.ops.transformer import fused_qkv_attention  # noqa: E402

SCALE = 1.0 / math.sqrt(64)


def _ref(qkv, H, causal, lse=False):
    """fp32 attention on the split views of qkv [B, S, 3 H 64]: [B, S, H * 64] (or log2 lse)."""
    B, S, _ = qkv.shape
    q, k, v = qkv.float().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=qkv.device).triu(1), float("-inf"))
    if lse:
        return torch.logsumexp(s, -1) / math.log(2.0)
    return torch.matmul(torch.softmax(s, -1), v).transpose(1, 2).reshape(B, S, H * 64)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()


def _qkv(B, H, S, mag=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, S, 3 * H * 64, device="cuda", generator=g) * mag).bfloat16()


def _check_fwd_bwd(qkv, H, causal, fwd, gtol):
    x = qkv.clone().requires_grad_()
    o = fwd(x)
    xr = qkv.float().requires_grad_()
    ref = _ref(xr, H, causal)
    assert o.shape == ref.shape and o.dtype == torch.bfloat16
    assert _rel(o, ref) < 1e-2, _rel(o, ref)
    do = torch.randn_like(ref).bfloat16()
    o.backward(do)
    ref.backward(do.float())
    assert torch.isfinite(x.grad.float()).all()
    for j, name in enumerate(("dq", "dk", "dv")):
        lo, hi = j * H * 64, (j + 1) * H * 64
        err = _rel(x.grad[..., lo:hi], xr.grad[..., lo:hi])
        assert err < gtol, (name, err)
    return o


CASES = [  # B, H, S, causal
    (2, 3, 129, False), (2, 3, 129, True),     # one full tile + 1 row; BH % 8 != 0
    (2, 4, 192, False),                        # partial second tile at a 64 boundary; XCD remap
    (2, 4, 256, False), (2, 4, 256, True),     # two full tiles: both buffers
    (2, 3, 384, False),                        # third tile reuses buffer 0
    (2, 3, 1000, False), (2, 4, 1000, True),   # ragged, many tiles
    (2, 4, 64, True),                          # single partial tile
]


@pytest.mark.parametrize("B,H,S,causal", CASES)
def test_flash64_fwd_bwd_vs_fp32(B, H, S, causal):
    _check_fwd_bwd(_qkv(B, H, S), H, causal, lambda x: fused_qkv_attention(x, H, 64, causal), 1e-2)


@pytest.mark.parametrize("S,causal", [(129, False), (256, True), (1000, False), (1000, True)])
def test_flash64_fwd_64_queries_per_wave(S, causal):
    """The forward's 64-queries-per-wave form (chosen on its own only for grids that fill the
    chip several times over) at the same boundaries, forced through ``nq``."""
    qkv = _qkv(2, 3, S, seed=2)
    o, lse = lib().flash64_fwd(qkv, 3, causal, SCALE, 8.0, 2)
    assert _rel(o, _ref(qkv, 3, causal)) < 1e-2
    assert (lse - _ref(qkv, 3, causal, lse=True)).abs().max().item() < 1e-3


def test_flash64_lse():
    qkv = _qkv(1, 4, 200, seed=5)
    _, lse = lib().flash64_fwd(qkv, 4, True, SCALE)
    assert (lse - _ref(qkv, 4, True, lse=True)).abs().max().item() < 1e-3


def test_flash64_large_scores():
    """Scores of magnitude ~100 and one spiked key mid-sequence: the deferred rescale (threshold
    8) and the textbook one (0) both match the oracle and give the same lse."""
    H, S = 4, 777
    qkv = _qkv(1, H, S, mag=4.0, seed=3)
    qkv[0, 300, (H + 1) * 64:(H + 2) * 64] *= 8      # key 300 of head 1
    _check_fwd_bwd(qkv, H, True, lambda x: fused_qkv_attention(x, H, 64, True), 2e-2)
    (o8, l8), (o0, l0) = (lib().flash64_fwd(qkv, H, True, SCALE, t) for t in (8.0, 0.0))
    ref = _ref(qkv, H, True)
    assert _rel(o8, ref) < 1e-2 and _rel(o0, ref) < 1e-2
    assert (l8 - l0).abs().max().item() < 1e-3


def test_flash64_deterministic():
    qkv = _qkv(2, 4, 1000, seed=7)
    do = torch.randn(2, 1000, 4 * 64, device="cuda").bfloat16()
    outs = []
    for _ in range(2):
        x = qkv.clone().requires_grad_()
        o = fused_qkv_attention(x, 4, 64, True)
        o.backward(do)
        outs.append((o, x.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("flag", [True, False])
def test_flash64_dispatch(flag, monkeypatch):
    """A BertLayer at S = 256 never reaches SDPA (it does with the policy flag off); S = 128 stays
    on the short kernel."""
    from consensusml_amd.models.transformer import BertConfig, BertLayer
    calls = []
    orig = torch.nn.functional.scaled_dot_product_attention
    monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention",
                        lambda *a, **k: calls.append(1) or orig(*a, **k))
    prev = perf.set_policy(perf.policy().replace(flash_attn64=flag))
    try:
        torch.manual_seed(0)
        layer = BertLayer(BertConfig(d=256, heads=4, ffn=512)).cuda().bfloat16()
        x = torch.randn(2, 256, 256, device="cuda").bfloat16().requires_grad_()
        layer(x).float().square().mean().backward()
        assert torch.isfinite(x.grad.float()).all()
        assert bool(calls) == (not flag)
        qkv = _qkv(2, 4, 128, seed=9)
        assert torch.equal(fused_qkv_attention(qkv, 4, 64), lib().attn_fwd(qkv, 4, SCALE)[0])
    finally:
        perf.set_policy(prev)
