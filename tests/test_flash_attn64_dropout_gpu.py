"""Attention dropout inside the head-dim-64 flash kernels (csrc/kernels/flash_attn64_drop.hip)
against float64 softmax(q k^T / 8) * dropout_mask / (1 - p_eff) @ v and its autograd gradient;
bound 1e-2 on the relative Frobenius error (per sequence), as in test_flash_attn64_lens_gpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from consensusml_amd.ops import transformer as T  # noqa: E402
from consensusml_amd.ops.native import lib  # noqa: E402

SCALE = 1.0 / math.sqrt(64)
RNG = (1234, 77)


def _ref(x, H, causal, keep):
    """float64 dropped attention on one sequence x [n, 3 H 64], keep [H, n, n] already scaled."""
    n = x.shape[0]
    q, k, v = x.view(n, 3, H, 64).permute(1, 2, 0, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if causal:
        s = s.masked_fill(torch.ones(n, n, device=x.device).triu(1).bool(), float("-inf"))
    return torch.matmul(torch.softmax(s, -1) * keep, v).transpose(0, 1).reshape(n, H * 64)


def _inputs(B, H, S):
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * 64, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, S, H * 64, device="cuda", generator=g).bfloat16()
    return qkv, do


LENS = (1, 64, 129, 192, 257, 384)
CASES = [  # H, S, lens (None: B = 2 full sequences), causal
    *[(3, 320, None, c) for c in (False, True)],   # 3 key tiles, half-filled last, BH % 8 != 0
    (4, 256, None, True),                          # BH = 8: the XCD remap
    *[(3, 384, LENS, c) for c in (False, True)],   # on / next to every 64 / 128 boundary
    (3, 64, None, True),                           # the single-tile flash path
    (3, 100, None, False),                         # S % 8 != 0: the composition
]


@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("H,S,lens,causal", CASES)
def test_dropout_vs_fp64(H, S, lens, causal, p):
    """Sections whose reference is zero (dq, dk of a one-token sequence) take the floor of the
    lengths test, 1e-3 of the sequence's whole gradient (the 1e-30 only keeps 0 / 0 out).
    There dS = M dP - D must cancel: the kernels take D = rowsum(dO * O) from the forward's fp32
    output row, since bf16(V / (1 - p_eff)) is rounded unless 1 / (1 - p_eff) is a power of two."""
    ns = lens or (S, S)
    qkv, do = _inputs(len(ns), H, S)
    lt = lens and torch.tensor(lens, dtype=torch.int32, device="cuda")
    for b, n in enumerate(lens or ()):
        qkv[b, n:] = do[b, n:] = float("nan")
    x = qkv.clone().requires_grad_()
    o = T.fused_qkv_attention(x, H, 64, causal, lens=lt, dropout=p, rng=RNG)
    o.backward(do)
    assert torch.isfinite(o.float()).all() and torch.isfinite(x.grad.float()).all()
    keep = T.dropout_mask(*RNG, (len(ns), H, S, S), p).double()
    keep *= 65536.0 / (65536 - round(p * 65536))
    for b, n in enumerate(ns):
        assert (o[b, n:] == 0).all() and (x.grad[b, n:] == 0).all()
        xr = qkv[b, :n].double().requires_grad_()
        ro = _ref(xr, H, causal, keep[b, :, :n, :n])
        ro.backward(do[b, :n].double())
        errs = {"o": ((o[b, :n].double() - ro).norm() / ro.norm().clamp_min(1e-30)).item()}
        floor = (1e-3 * xr.grad.norm()).clamp_min(1e-30)
        for j, name in enumerate(("dq", "dk", "dv")):
            sl = slice(j * H * 64, (j + 1) * H * 64)
            errs[name] = ((x.grad[b, :n, sl].double() - xr.grad[:, sl]).norm()
                          / torch.maximum(xr.grad[:, sl].norm(), floor)).item()
        print(f"len {n}:", {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) < 1e-2, (n, errs)


def test_deterministic_and_offset():
    qkv, do = _inputs(2, 3, 320)
    def run(rng):  # noqa: E306
        x = qkv.clone().requires_grad_()
        o = T.fused_qkv_attention(x, 3, 64, True, dropout=0.1, rng=rng)
        o.backward(do)
        return o, x.grad
    (o1, g1), (o2, g2), (o3, _) = run(RNG), run(RNG), run((RNG[0], RNG[1] + 1))
    assert torch.equal(o1, o2) and torch.equal(g1, g2) and not torch.equal(o1, o3)


def test_bert_layer_reaches_the_kernels(monkeypatch):
    from consensusml_amd.models.transformer import BertConfig, BertLayer
    calls = []
    for mod, name in ((T, "_dropout_attention"),
                      (torch.nn.functional, "scaled_dot_product_attention")):
        monkeypatch.setattr(mod, name, lambda *a, _f=getattr(mod, name), **k:
                            calls.append(1) or _f(*a, **k))
    torch.manual_seed(0)
    cfg = BertConfig(d=256, heads=4, ffn=512, dropout=0.1, attn_dropout=0.1)
    layer = BertLayer(cfg).cuda().bfloat16().train()
    x = torch.randn(2, 256, 256, device="cuda").bfloat16().requires_grad_()
    y = layer(x, torch.tensor((256, 131), dtype=torch.int32, device="cuda"))
    y.float().square().mean().backward()
    assert torch.isfinite(y.float()).all() and torch.isfinite(x.grad.float()).all()
    assert not calls
    qkv, _ = _inputs(2, 3, 320)
    a, b = (lib().flash64_fwd(qkv, 3, False, SCALE, **k) for k in ({"thr": 0}, {}))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
