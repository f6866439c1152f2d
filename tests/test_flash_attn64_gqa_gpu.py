"""Head-dim-64 grouped-query flash attention (csrc/kernels/flash_attn64_gqa.hip) against an fp32
softmax(q k^T scale [+ causal]) v oracle with the kv heads expanded: forward, dQ and the dK / dV
kernel that sums each kv head's query heads inside its flat (head, query tile) loop."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from consensusml_amd.ops.native import lib  # noqa: E402
from consensusml_amd.ops.transformer import (flash_attention, qkv_attention,  # noqa: E402
                                             rope_tables)

HD = 64
SCALE = 1.0 / math.sqrt(HD)


def _ref(q, k, v, causal):
    """fp32 attention with GQA expansion: [B, S, H * hd]."""
    B, H, S, D = q.shape
    grp = H // k.shape[1]
    s = torch.matmul(q.float(), k.float().repeat_interleave(grp, 1).transpose(-1, -2)) * SCALE
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    o = torch.matmul(torch.softmax(s, -1), v.float().repeat_interleave(grp, 1))
    return o.transpose(1, 2).reshape(B, S, H * D)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()


def _inputs(B, H, KV, S, mag=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda h: (torch.randn(B, h, S, HD, device="cuda", generator=g) * mag).bfloat16()  # noqa
    return mk(H), mk(KV), mk(KV)


@pytest.mark.parametrize("B,H,KV,S,causal,mag,tol", [
    (1, 4, 1, 129, True, 1.0, 1e-2),      # one key past a tile
    (2, 6, 2, 300, True, 1.0, 1e-2),      # grp 3: 9 items, buffer parity flips at each head change
    (1, 8, 1, 257, True, 1.0, 1e-2),      # grp 8
    (2, 4, 4, 320, True, 1.0, 1e-2),      # grp 1
    (1, 8, 2, 1000, False, 1.0, 1e-2),    # full attention, ragged
    (1, 4, 2, 40, True, 1.0, 1e-2),       # S below one wave's tile
    (1, 4, 2, 40, False, 1.0, 1e-2),
    (1, 32, 8, 2048, True, 1.0, 1e-2),    # the Llama-3.2-1B layer
    (1, 4, 2, 777, True, 4.0, 2e-2),      # large scores: magnitude 4 and a spiked key (below)
])
def test_gqa64_fwd_bwd_vs_fp32(B, H, KV, S, causal, mag, tol):
    """Forward + backward through flash_attention: o at 1e-2, gradients at tol (2e-2 for the
    large-score case, as the head-dim-128 test has it)."""
    q, k, v = _inputs(B, H, KV, S, mag, seed=3 if mag > 1 else 0)
    if mag > 1:
        k[0, 1, 300] *= 8      # its row max appears mid-sequence: the running max jumps
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    o = flash_attention(qa, ka, va, causal=causal)
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    ref = _ref(qr, kr, vr, causal)
    assert o.shape == ref.shape and o.dtype == torch.bfloat16
    assert torch.isfinite(o.float()).all() and _rel(o, ref) < 1e-2
    do = torch.randn_like(ref).bfloat16()
    o.backward(do)
    ref.backward(do.float())
    for got, want, name in ((qa.grad, qr.grad, "dq"), (ka.grad, kr.grad, "dk"),
                            (va.grad, vr.grad, "dv")):
        assert got.shape == want.shape, name
        assert torch.isfinite(got.float()).all(), name
        assert _rel(got, want) < tol, (name, _rel(got, want))


@pytest.mark.parametrize("S,rot", [(129, True), (300, True), (256, False)])
def test_gqa64_qkv_rope_vs_fp32(S, rot):
    """Fused path: qkv -> RoPE split -> flash; backward flash (group sum inside) -> RoPE bwd."""
    B, H, KV = 2, 8, 2
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.randn(B, S, (H + 2 * KV) * HD, device="cuda", generator=g).bfloat16()
    cos, sin = rope_tables(S, HD, 500000.0, "cuda") if rot else (None, None)
    x = qkv.clone().requires_grad_()
    o = qkv_attention(x, H, KV, HD, cos, sin)
    xr = qkv.float().requires_grad_()
    t = xr.view(B, S, H + 2 * KV, HD).transpose(1, 2)
    q, k, v = t[:, :H], t[:, H:H + KV], t[:, H + KV:]
    if rot:
        def rope(z):
            z1, z2 = z[..., 0::2], z[..., 1::2]
            c, s_ = cos[None, None], sin[None, None]
            return torch.stack((z1 * c - z2 * s_, z1 * s_ + z2 * c), -1).flatten(-2)
        q, k = rope(q), rope(k)
    ref = _ref(q, k, v, True)
    assert _rel(o, ref) < 1e-2
    do = torch.randn_like(ref).bfloat16()
    o.backward(do)
    ref.backward(do.float())
    assert torch.isfinite(x.grad.float()).all()
    assert _rel(x.grad, xr.grad) < 1e-2
    for lo, hi in ((0, H * HD), (H * HD, (H + KV) * HD), ((H + KV) * HD, (H + 2 * KV) * HD)):
        assert _rel(x.grad[..., lo:hi], xr.grad[..., lo:hi]) < 1e-2


def test_gqa64_lse():
    q, k, v = _inputs(1, 4, 2, 200, seed=5)
    _, lse = lib().flash_fwd(q, k, v, True, SCALE)
    s = torch.matmul(q.float(), k.float().repeat_interleave(2, 1).transpose(-1, -2)) * SCALE
    s = s.masked_fill(torch.ones(200, 200, dtype=torch.bool, device="cuda").triu(1), float("-inf"))
    assert (lse - torch.logsumexp(s, -1) / math.log(2.0)).abs().max().item() < 1e-3


def test_gqa64_deterministic():
    q, k, v = _inputs(2, 8, 2, 1000, seed=7)
    do = torch.randn(2, 1000, 8 * HD, device="cuda").bfloat16()
    outs = []
    for _ in range(2):
        qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
        o = flash_attention(qa, ka, va, causal=True)
        o.backward(do)
        outs.append([o, qa.grad, ka.grad, va.grad])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("docs", [False, True])
def test_gqa64_llama_block_routing(docs):
    """A head-dim-64 Llama layer trains a step on the kernels (no SDPA call); with document bounds
    it takes the documented SDPA fallback."""
    from consensusml_amd.models.transformer import Llama, LlamaConfig
    m = Llama(LlamaConfig(vocab=256, d=256, layers=1, heads=4, kv_heads=2, ffn=256,
                          max_seq=256)).cuda().bfloat16()
    ids = torch.randint(0, 256, (2, 256), device="cuda")
    doc_ids = (torch.arange(256, device="cuda") // 100).expand(2, 256) if docs else None
    calls = []
    orig = torch.nn.functional.scaled_dot_product_attention
    torch.nn.functional.scaled_dot_product_attention = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        m(ids, doc_ids).float().logsumexp(-1).mean().backward()
    finally:
        torch.nn.functional.scaled_dot_product_attention = orig
    assert bool(calls) == docs
    assert all(torch.isfinite(p.grad.float()).all() for p in m.parameters() if p.grad is not None)
