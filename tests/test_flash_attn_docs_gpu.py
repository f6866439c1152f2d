"""Document-masked causal attention (the DOC kernels of csrc/kernels/flash_attn.hip and the bounds
kernel of flash_attn_doc.hip) against the fp32 softmax(Q K^T) V oracle of test_flash_attn_gpu.py
applied to each document's slice alone, errors taken per document."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from consensusml_amd.ops.native import lib  # noqa: E402
from consensusml_amd.ops.transformer import (doc_bounds, flash_attention,  # noqa: E402
                                             qkv_attention, rope_tables)

SCALE = 1.0 / math.sqrt(128)
LENS = (1, 63, 64, 129, 255, 88)   # starts at 1, 64, 128, 257, 512 of S = 600
CASES = {600: [LENS], 1000: [(300, 700), (1000,)], 130: [(1,) * 130]}   # S: lengths per row


def _ref(q, k, v):
    """fp32 causal attention with GQA expansion: (o [B, S, H * hd], log2 lse [B, H, S])."""
    B, H, S, D = q.shape
    kf, vf = (t.float().repeat_interleave(H // k.shape[1], 1) for t in (k, v))
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * SCALE
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    o = torch.matmul(torch.softmax(s, -1), vf).transpose(1, 2).reshape(B, S, H * D)
    return o, torch.logsumexp(s, -1) / math.log(2.0)


def _ids(rows):
    """doc ids [B, S] of rows: one tuple of document lengths per batch row."""
    return torch.stack([torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r))
                        for r in rows])


def _inputs(rows, S, H, KV, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda *sh: torch.randn(*sh, device="cuda", generator=g).bfloat16()  # noqa: E731
    B = len(rows)
    return (mk(B, H, S, 128), mk(B, KV, S, 128), mk(B, KV, S, 128), mk(B, S, H * 128),
            _ids(rows).cuda())


def _per_doc(rows, o, grads, ref_of, do):
    """Per document: max over o and the gradient sections of |got - ref| / max(|ref|, 1e-3 of the
    document's whole reference gradient) (a one-token document's dq and dk are exactly zero).
    ref_of(b, sl) -> (leaf tensors, o reference); grads: tensors sliced like the leaves."""
    for b, lens in enumerate(rows):
        for s0, n in zip(torch.tensor((0,) + lens).cumsum(0).tolist(), lens):
            sl = slice(s0, s0 + n)
            leaves, ro = ref_of(b, sl)
            ro.backward(do[b:b + 1, sl].float())
            floor = 1e-3 * torch.cat([t.grad.flatten() for t in leaves]).norm()
            errs = [((o[b:b + 1, sl].float() - ro).norm() / ro.norm()).item()]
            for got, t in zip(grads(b, sl), leaves):
                errs.append(((got.float() - t.grad).norm()
                             / torch.maximum(t.grad.norm(), floor)).item())
            print(f"row {b} doc [{s0}, {s0 + n}):", [f"{e:.2e}" for e in errs])
            assert max(errs) < 1e-2, (b, s0, n, errs)


@pytest.mark.parametrize("S", list(CASES))
def test_docs_vs_fp32_per_document(S):
    rows, H, KV = CASES[S], 4, 2
    q, k, v, do, ids = _inputs(rows, S, H, KV)
    bounds = doc_bounds(ids)
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    o = flash_attention(qa, ka, va, bounds=bounds)
    o.backward(do)
    lse = lib().flash_fwd(q, k, v, True, SCALE, lo=bounds[0])[1]
    assert all(torch.isfinite(t.float()).all() for t in (o, lse, qa.grad, ka.grad, va.grad))
    if S == 130:   # every document is one token: P = 1 on the diagonal alone
        assert torch.equal(o.view(1, S, H, 128), v.repeat_interleave(H // KV, 1).transpose(1, 2))

    def ref_of(b, sl):
        leaves = [t[b:b + 1, :, sl].float().requires_grad_() for t in (q, k, v)]
        ro, rl = _ref(*leaves)
        assert (lse[b:b + 1, :, sl] - rl).abs().max().item() < 1e-3
        return leaves, ro
    _per_doc(rows, o, lambda b, sl: [t.grad[b:b + 1, :, sl] for t in (qa, ka, va)], ref_of, do)


def test_single_document_bit_identical():
    q, k, v, do, ids = _inputs([(1000,), (1000,)], 1000, 8, 2, seed=1)
    lo, hi = doc_bounds(ids)
    o, lse = lib().flash_fwd(q, k, v, True, SCALE)
    od, lsed = lib().flash_fwd(q, k, v, True, SCALE, lo=lo)
    assert torch.equal(o, od) and torch.equal(lse, lsed)
    for a, b in zip(lib().flash_bwd(q, k, v, o, do, lse, True, SCALE),
                    lib().flash_bwd(q, k, v, o, do, lse, True, SCALE, lo=lo, hi=hi)):
        assert torch.equal(a, b)


def test_documents_are_isolated():
    """Other finite values in the first document leave the second document's outputs bit for bit:
    masked elements contribute exact zeros."""
    q, k, v, do, ids = _inputs([(257, 343)], 600, 4, 2, seed=2)
    lo, hi = doc_bounds(ids)

    def run():
        o, lse = lib().flash_fwd(q, k, v, True, SCALE, lo=lo)
        outs = lib().flash_bwd(q, k, v, o, do, lse, True, SCALE, lo=lo, hi=hi)
        return [o[:, 257:], lse[..., 257:]] + [t[:, :, 257:] for t in outs]
    before = [t.clone() for t in run()]
    for t in (q, k, v):
        t[:, :, :257] = torch.randn_like(t[:, :, :257]) * 3
    do[:, :257] = torch.randn_like(do[:, :257])
    assert all(torch.equal(a, b) for a, b in zip(before, run()))


def test_qkv_rope_flash_docs_vs_fp32():
    B, S, H, KV, hd = 1, 600, 8, 2, 128
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.randn(B, S, (H + 2 * KV) * hd, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, S, H * hd, device="cuda", generator=g).bfloat16()
    cols = (0, H * hd, (H + KV) * hd, (H + 2 * KV) * hd)   # q / k / v column sections
    cos, sin = rope_tables(S, hd, 500000.0, "cuda")
    x = qkv.clone().requires_grad_()
    o = qkv_attention(x, H, KV, hd, cos, sin, bounds=doc_bounds(_ids([LENS]).cuda()))
    o.backward(do)

    def rope(z, sl):
        z1, z2, c, s_ = z[..., 0::2], z[..., 1::2], cos[None, None, sl], sin[None, None, sl]
        return torch.stack((z1 * c - z2 * s_, z1 * s_ + z2 * c), -1).flatten(-2)

    def ref_of(b, sl):   # one leaf per column section of the document's rows
        leaves = [qkv[b:b + 1, sl, c0:c1].float().requires_grad_() for c0, c1 in zip(cols, cols[1:])]
        qh, kh, vh = (t.view(1, t.shape[1], -1, hd).transpose(1, 2) for t in leaves)
        return leaves, _ref(rope(qh, sl), rope(kh, sl), vh)[0]
    _per_doc([LENS], o,
             lambda b, sl: [x.grad[b:b + 1, sl, c0:c1] for c0, c1 in zip(cols, cols[1:])], ref_of, do)


def test_llama_doc_ids_uses_flash(monkeypatch):
    from consensusml_amd.models.transformer import Llama, LlamaConfig
    m = Llama(LlamaConfig(vocab=256, d=512, layers=1, heads=4, kv_heads=2, ffn=512,
                          max_seq=256)).cuda().bfloat16()
    ids = torch.randint(0, 256, (2, 256), device="cuda")
    doc_ids = _ids([(100, 156), (1, 64, 191)]).cuda()
    calls = []
    orig = torch.nn.functional.scaled_dot_product_attention
    monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention",
                        lambda *a, **k: calls.append(1) or orig(*a, **k))
    m(ids, doc_ids).float().logsumexp(-1).mean().backward()
    assert not calls
    assert all(torch.isfinite(p.grad.float()).all() for p in m.parameters() if p.grad is not None)


def test_doc_bounds_device_equals_cpu():
    g = torch.Generator().manual_seed(3)
    long = torch.zeros(1, 8192, dtype=torch.int64)
    long[0, torch.randperm(8191, generator=g)[:50] + 1] = 1
    rows = [_ids(r) for r in CASES.values()]
    rows += [torch.zeros(2, 1000, dtype=torch.int32), _ids([(257, 343)]),
             long.cumsum(1) % 7]   # ids repeat later in the row
    for ids in rows:
        for got, want in zip(doc_bounds(ids.cuda()), doc_bounds(ids)):
            assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
