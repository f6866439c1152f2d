"""Fused dropout (csrc/kernels/dropout.h inside transformer.hip's add+norm passes and attention.hip)
vs fp64 references built from ``dropout_mask`` for the same (seed, offset), plus the statistics of
the counter-based mask itself."""
import math

import pytest
import torch
import torch.nn.functional as F

from consensusml_amd.ops import transformer as T
from consensusml_amd.ops import worker_grads as WG

pytestmark = pytest.mark.gpu
RNG = (0x1234_5678_9ABC, 7)


def _inv_keep(p):
    return 65536.0 / (65536 - round(p * 65536))   # 1 / (1 - p_eff)


def _close(a, b, rtol, atol, p):
    # the dropout-free op's tolerance, its absolute term times 1 / (1 - p_eff): kept values are
    # scaled by that factor
    torch.testing.assert_close(a.double(), b, rtol=rtol, atol=atol * _inv_keep(p))


def _norm64(s, w, b, eps):
    if b is not None:
        return F.layer_norm(s, s.shape[-1:], w, b, eps)
    return s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + eps) * w


def _norm_inputs(M, D, kind, cuda):
    torch.manual_seed(D + M)
    x = (torch.randn(M, D, device=cuda) * 2 + 0.5).bfloat16().requires_grad_(True)
    r = torch.randn(M, D, device=cuda).bfloat16().requires_grad_(True)
    w = (torch.rand(D, device=cuda) + 0.5).bfloat16().requires_grad_(True)
    b = torch.randn(D, device=cuda).bfloat16().requires_grad_(True) if kind == "ln" else None
    return x, r, w, b, torch.randn_like(x), torch.randn_like(x)


# D 64: a partly filled wave, 768: NV = 2, 2048: four waves per row; V = 2: the segmented backward
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D,V", [(64, 1), (768, 1), (2048, 1), (768, 2)])
@pytest.mark.parametrize("kind", ["ln", "rms"])
def test_add_norm_dropout(cuda, kind, D, V, p):
    M, eps = 37 + (V - 1), 1e-5
    x, r, w, b, dy, ds = _norm_inputs(M, D, kind, cuda)
    views = {id(t): torch.zeros(V, D, device=cuda, dtype=torch.bfloat16) for t in (w, b) if t is not None}
    prev = WG.activate(WG.WorkerGrads(V, views)) if V > 1 else None
    try:
        s, y = T.add_norm(x, r, w, b, eps, dropout=p, rng=RNG)
        torch.autograd.backward([y, s], [dy, ds])
    finally:
        if V > 1:
            WG.activate(prev)
    keep = T.dropout_mask(*RNG, r.shape, p, cuda)
    xr, rr, wr = (t.detach().double().requires_grad_(True) for t in (x, r, w))
    br = b.detach().double().requires_grad_(True) if b is not None else None
    sr = xr + keep.double() * rr * _inv_keep(p)
    yr = _norm64(sr, wr, br, eps)
    if V > 1:   # worker 1's own dgamma: the loss over its rows only
        rows = torch.arange(M, device=cuda)[:, None] >= M // 2
        (g1,) = torch.autograd.grad(yr, wr, dy.double() * rows, retain_graph=True)
        _close(views[id(w)][1], g1, 2e-2, 0.3, p)
    torch.autograd.backward([yr, sr], [dy.double(), ds.double()])
    _close(s, sr.detach(), 2e-2, 2e-2, p)
    _close(y, yr.detach(), 2e-2, 2e-2, p)
    _close(x.grad, xr.grad, 3e-2, 3e-2, p)
    _close(r.grad, rr.grad, 3e-2, 3e-2, p)
    assert (r.grad[keep == 0] == 0).all() and (keep == 0).any()
    if V == 1:
        dw, db = w.grad, b.grad if b is not None else None
    else:   # the V segments' partial sums add up to the whole batch's gradient
        dw, db = views[id(w)].float().sum(0), views[id(b)].float().sum(0) if b is not None else None
    _close(dw, wr.grad, 2e-2, 0.3, p)
    if b is not None:
        _close(db, br.grad, 2e-2, 0.3, p)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D", [64, 2048])
def test_norm_output_dropout(cuda, D, p):
    """The embedding site: y = keep * LN(x) / (1 - p), the backward masks dy on load."""
    x, _, w, b, dy, _ = _norm_inputs(37, D, "ln", cuda)
    y = T.norm(x, w, b, 1e-5, dropout=p, rng=RNG)
    y.backward(dy)
    m = T.dropout_mask(*RNG, x.shape, p, cuda).double() * _inv_keep(p)
    xr, wr, br = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    yr = _norm64(xr, wr, br, 1e-5) * m
    yr.backward(dy.double())
    assert (y[m == 0] == 0).all()
    _close(y, yr.detach(), 2e-2, 2e-2, p)
    _close(x.grad, xr.grad, 3e-2, 3e-2, p)
    _close(w.grad, wr.grad, 2e-2, 0.3, p)
    _close(b.grad, br.grad, 2e-2, 0.3, p)


def _attn64(qkv, H, keep_scaled):
    B, S, _ = qkv.shape
    x = qkv.view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    pr = torch.softmax(x[0] @ x[1].transpose(-1, -2) / 8.0, -1) * keep_scaled
    return (pr @ x[2]).transpose(1, 2).reshape(B, S, H * 64)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("S", [32, 96, 128])
def test_attention_dropout(cuda, S, p):
    torch.manual_seed(S)
    B, H = 2, 3
    qkv = (torch.randn(B, S, 3 * H * 64, device=cuda) * 1.5).bfloat16().requires_grad_(True)
    out = T.fused_qkv_attention(qkv, H, 64, dropout=p, rng=RNG)
    dout = torch.randn_like(out)
    out.backward(dout)
    keep = T.dropout_mask(*RNG, (B, H, S, S), p, cuda)
    xr = qkv.detach().double().requires_grad_(True)
    ref = _attn64(xr, H, keep.double() * _inv_keep(p))
    ref.backward(dout.double())
    _close(out, ref.detach(), 2e-2, 2e-2, p)
    _close(qkv.grad, xr.grad, 5e-2, 5e-2, p)
    # same (seed, offset): bit-identical output and gradient
    q2 = qkv.detach().clone().requires_grad_(True)
    o2 = T.fused_qkv_attention(q2, H, 64, dropout=p, rng=RNG)
    o2.backward(dout)
    assert torch.equal(o2, out) and torch.equal(q2.grad, qkv.grad)


@pytest.mark.parametrize("kw", [dict(dropout=0.0), dict(dropout=0.3, training=False)])
def test_no_dropout_is_bit_identical(cuda, kw):
    x, r, w, b, dy, _ = _norm_inputs(37, 768, "ln", cuda)
    qkv = torch.randn(2, 96, 3 * 3 * 64, device=cuda).bfloat16()

    def run(**k):
        xs, rs, qs = (t.detach().clone().requires_grad_(True) for t in (x, r, qkv))
        _, y = T.add_norm(xs, rs, w, b, 1e-5, **k)
        z = T.norm(xs, w, b, 1e-5, **k)
        o = T.fused_qkv_attention(qs, 3, 64, **k)
        torch.autograd.backward([y, z, o], [dy, dy, torch.ones_like(o)])
        return y, z, o, xs.grad, rs.grad, qs.grad
    before = T.dropout_stream.counter
    for a, c in zip(run(), run(**kw)):
        assert torch.equal(a, c)
    assert T.dropout_stream.counter == before   # inactive sites take no draw


def test_same_rng_is_deterministic_and_stream_advances(cuda):
    x, r, w, b, dy, _ = _norm_inputs(37, 2048, "rms", cuda)

    def run(rng):
        xs, rs = (t.detach().clone().requires_grad_(True) for t in (x, r))
        s, y = T.add_norm(xs, rs, w, None, 1e-5, dropout=0.5, rng=rng)
        y.backward(dy)
        return s, y, xs.grad, rs.grad
    for a, c in zip(run(RNG), run(RNG)):
        assert torch.equal(a, c)
    assert not torch.equal(run(None)[0], run(None)[0])   # the stream: a new offset per call


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics(cuda, p):
    """2^20-element masks: keep rate within 5 sigma of 1 - p_eff; masks of neighbouring offsets,
    batch entries and heads agree at the rate of independent ones, (1 - p)^2 + p^2."""
    N, pe = 1 << 20, round(p * 65536) / 65536
    m0 = T.dropout_mask(*RNG, (N,), p, cuda)
    assert set(m0.unique().tolist()) == {0, 1}
    assert abs(m0.float().mean().item() - (1 - pe)) < 5 * math.sqrt(pe * (1 - pe) / N)
    m1 = T.dropout_mask(RNG[0], RNG[1] + 1, (N,), p, cuda)
    a = T.dropout_mask(*RNG, (2, 2, 512, 512), p, cuda)            # [B, H, S, S], 2^18 per (b, h)
    ind = (1 - pe) ** 2 + pe ** 2
    for u, v in ((m0, m1), (a[0], a[1]), (a[:, 0], a[:, 1])):
        sig = math.sqrt(ind * (1 - ind) / u.numel())
        assert abs((u == v).float().mean().item() - ind) < 5 * sig
