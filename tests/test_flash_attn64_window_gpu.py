"""Sliding-window causal flash attention (csrc/kernels/flash_attn64_gqa_win.hip; head dim 128:
flash_attn.hip's document kernels under window bounds) against an fp32 masked softmax with the kv
heads expanded: query i sees keys i - W < j <= i."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from consensusml_amd.ops.native import lib  # noqa: E402
from consensusml_amd.ops.transformer import (flash_attention, qkv_attention,  # noqa: E402
                                             rope_tables)


def _scores(q, k, W):
    """fp32 masked scores [B, H, S, S] (-inf where j > i or j <= i - W)."""
    S, grp = q.shape[2], q.shape[1] // k.shape[1]
    s = torch.matmul(q.float(), k.float().repeat_interleave(grp, 1).transpose(-1, -2))
    pos = torch.arange(S, device=q.device)
    hidden = (pos > pos[:, None]) | (pos <= pos[:, None] - W)
    return (s / math.sqrt(q.shape[3])).masked_fill(hidden, float("-inf"))


def _ref(q, k, v, W):
    B, H, S, D = q.shape
    o = torch.matmul(torch.softmax(_scores(q, k, W), -1),
                     v.float().repeat_interleave(H // k.shape[1], 1))
    return o.transpose(1, 2).reshape(B, S, H * D)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()


def _inputs(B, H, KV, S, mag=1.0, seed=0, hd=64):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda h: (torch.randn(B, h, S, hd, device="cuda", generator=g) * mag).bfloat16()  # noqa
    return mk(H), mk(KV), mk(KV)


def _run(q, k, v, W, do):
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    o = flash_attention(qa, ka, va, window=W)
    o.backward(do)
    return o, qa.grad, ka.grad, va.grad


@pytest.mark.parametrize("B,H,KV,S,W,hd,mag,tol", [
    (1, 4, 1, 129, 1, 64, 1.0, 1e-2),     # self only: o = v's rows; first tile masked for late rows
    (1, 4, 2, 40, 7, 64, 1.0, 1e-2),      # S below one tile
    (1, 4, 1, 300, 64, 64, 1.0, 1e-2),    # window shorter than a tile
    (2, 6, 2, 300, 128, 64, 1.0, 1e-2),   # W = tile; grp 3: dK / dV ranges restart at head changes
    (1, 8, 1, 385, 129, 64, 1.0, 1e-2),   # lower edge crosses two tiles; grp 8
    (2, 4, 4, 520, 200, 64, 1.0, 1e-2),   # grp 1; key blocks whose query range ends before S
    (1, 4, 2, 777, 256, 64, 4.0, 2e-2),   # large scores: magnitude 4 and a spiked key (below)
    (1, 4, 2, 300, 100, 128, 1.0, 1e-2),  # head dim 128: document kernels under window bounds
])
def test_window_fwd_bwd_vs_fp32(B, H, KV, S, W, hd, mag, tol):
    """o at 1e-2, gradients at tol (2e-2 for the large-score case), relative Frobenius error."""
    q, k, v = _inputs(B, H, KV, S, mag, seed=3 if mag > 1 else 0, hd=hd)
    if mag > 1:
        k[0, 1, 300] *= 8      # its row max appears mid-sequence: the running max jumps
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    ref = _ref(qr, kr, vr, W)
    do = torch.randn_like(ref).bfloat16()
    ref.backward(do.float())
    o, dq, dk, dv = _run(q, k, v, W, do)
    assert o.shape == ref.shape and o.dtype == torch.bfloat16
    assert torch.isfinite(o.float()).all() and _rel(o, ref) < 1e-2, _rel(o, ref)
    for got, want, name in ((dq, qr.grad, "dq"), (dk, kr.grad, "dk"), (dv, vr.grad, "dv")):
        assert got.shape == want.shape, name
        assert torch.isfinite(got.float()).all(), name
        if W == 1 and name != "dv":
            # softmax over one key is constant: dq = dk = 0 exactly and a relative error has no
            # denominator. The kernels form dS = P (dP - D) from two fp32 dot products dO . v that
            # cancel, so the error is held to tol of the terms that cancel: scale |dO_i| |v_i|
            # times |k_i| (dq) or |q_i| (dk, summed over the group), per head and row
            g = H // KV
            rows = lambda t: t.float().norm(dim=-1)  # noqa: E731
            term = (rows(do.view(B, S, H, hd).transpose(1, 2)) * rows(v).repeat_interleave(g, 1)
                    * (rows(k).repeat_interleave(g, 1) if name == "dq" else rows(q)) / math.sqrt(hd))
            bound = term if name == "dq" else term.view(B, KV, g, S).sum(2)
            assert (got.float() - want).norm().item() < tol * bound.norm().item(), name
            continue
        assert _rel(got, want) < tol, (name, _rel(got, want))


def test_window_bit_identity_and_determinism():
    """window >= S is the plain causal path bit for bit; a window below S repeats bit for bit."""
    q, k, v = _inputs(1, 4, 2, 300, seed=7)
    do = torch.randn(1, 300, 4 * 64, device="cuda").bfloat16()
    plain = _run(q, k, v, None, do)
    for W in (300, 305):
        assert all(torch.equal(a, b) for a, b in zip(_run(q, k, v, W, do), plain))
    assert all(torch.equal(a, b) for a, b in zip(_run(q, k, v, 77, do), _run(q, k, v, 77, do)))
    assert not torch.equal(_run(q, k, v, 77, do)[0], plain[0])


def test_window_lse():
    q, k, v = _inputs(1, 4, 2, 200, seed=5)
    _, lse = lib().flash_fwd(q, k, v, True, 0.125, window=70)
    ref = torch.logsumexp(_scores(q, k, 70), -1) / math.log(2.0)
    assert (lse - ref).abs().max().item() < 1e-3


def test_window_qkv_rope_vs_fp32():
    """Fused path: qkv -> RoPE split -> window flash; backward -> RoPE bwd into the fused layout."""
    B, H, KV, S, W, HD = 2, 8, 2, 300, 100, 64
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.randn(B, S, (H + 2 * KV) * HD, device="cuda", generator=g).bfloat16()
    cos, sin = rope_tables(S, HD, 500000.0, "cuda")
    x = qkv.clone().requires_grad_()
    o = qkv_attention(x, H, KV, HD, cos, sin, window=W)
    xr = qkv.float().requires_grad_()
    t = xr.view(B, S, H + 2 * KV, HD).transpose(1, 2)

    def rope(z):
        z1, z2 = z[..., 0::2], z[..., 1::2]
        return torch.stack((z1 * cos - z2 * sin, z1 * sin + z2 * cos), -1).flatten(-2)
    ref = _ref(rope(t[:, :H]), rope(t[:, H:H + KV]), t[:, H + KV:], W)
    assert _rel(o, ref) < 1e-2
    do = torch.randn_like(ref).bfloat16()
    o.backward(do)
    ref.backward(do.float())
    assert torch.isfinite(x.grad.float()).all()
    for lo, hi in ((0, H * HD), (H * HD, (H + KV) * HD), ((H + KV) * HD, (H + 2 * KV) * HD)):
        assert _rel(x.grad[..., lo:hi], xr.grad[..., lo:hi]) < 1e-2


@pytest.mark.parametrize("docs", [False, True])
def test_window_llama_block_routing(docs):
    """A head-dim-64 Llama layer with a window trains a step on the kernels (no SDPA call); with
    document bounds as well it takes the SDPA fallback."""
    from consensusml_amd.models.transformer import Llama, LlamaConfig
    m = Llama(LlamaConfig(vocab=256, d=256, layers=1, heads=4, kv_heads=2, ffn=256, max_seq=256,
                          window=100)).cuda().bfloat16()
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
