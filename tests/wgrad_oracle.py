"""Exact and fp64 oracles of the weight-gradient kernels (wgrad1x1.hip: register-staged, LDS-DMA,
stride-2 gather, direct write, split-K folds; wgrad3x3.hip) and the case tables of
``test_wgrad3x3_exact_gpu.py``, ``test_wgrad_s2_exact_gpu.py``, ``test_wgrad1x1_exact_gpu.py`` and
``test_wgrad_exact_env_gpu.py`` (not collected: no ``test_`` prefix). Shaped like gemm_exact.py,
whose ``ints``, ``share_small``, ``mismatch_report`` and child-process runner it uses.

The reference is the definition, dW[co, tap, ci] = sum_p dy[p - s(tap), co] x[p, ci]: per tap one
fp64 matmul A_t^T B_t over the kernel's reduction index. At stride 1 that index is the input pixel,
A_t is a shifted slice of the zero-padded dy and B is x; at stride 2 it is the output pixel, A is dy
and B_t a strided slice of the zero-padded x (the single tap is tap 4 without padding). No library
convolution: an algorithm that transforms the operands need not be exact even on integers.

Exact tier. dy is bf16 integers in [-2, 2], x in [-1, 1] (seeded CPU generator): every product and
partial sum is an integer of magnitude <= 2 P < 2^24, so the fp32 accumulators, the per-split
partials and the fold are exact in any order. fp32 dW must EQUAL the fp64 sum, bf16 dW must equal
bf16_rne(sum); ``share_small`` (>= 99 % of |sum| < 256, integers bf16 holds exactly) is asserted
from the reference alone before the kernel's output is looked at, and the bf16 cases keep
P <= 4096 (std of a sum sqrt(4 P / 3)). Prologues stay exact with dyadic parameters: sc / da / db
in {+-0.5, +-1, 2}, bi / dc multiples of 0.5 up to 2, z integers in [-2, 2], random mask bytes; the
staged operands are multiples of 0.5 up to 10 (bf16 holds them, fused or not), the sums multiples
of 0.25 below 2^22, the column sums exact too. z sc + bi == 0 and g da + db == 0 are planted.

fp64 tier. randn bf16 inputs, per element
    |got - ref| <= (P + splits) 2^-24 sum_p |dy x|  (+ 2^-8 |ref| for bf16 output),
the recursive-summation bound over P products and `splits` partials. With a prologue the staged
bf16 operand is formed fused (fp64 multiply-add -> fp32 -> bf16, the reference) and unfused (fp32
multiply, fp32 add -> bf16) and sum_p |other operand| |fused - unfused| is added to the bound: a
1-ulp bf16 tie may go either way and nothing else may. The worst error-to-bound ratio is returned.

Guard tier. The exact inputs as 16-byte-aligned views inside NaN-filled bf16 buffers, the zero row
passed explicitly (inside a NaN buffer as well), wgrad1x1's ``out=`` a view inside a NaN row: dW
must equal the exact oracle and every guard element must still be NaN. A halo, clamped tail load
or padded slot fetched from outside the tensor and multiplied in turns dW NaN.

On a mismatch ``assert_dw`` raises with the count, the first few (co, tap, ci, got, want),
histograms by tap, TM x TN tile, 32-row co block and 64-column ci block, and whether got - want is
the contribution of one chunk or one pixel (dropped or counted twice).

Child mode: ``python wgrad_oracle.py '{"expect": {...}, "cases": [...]}'`` runs the named cases in
the environment it was started in and prints one JSON line per case with what wgrad_settings()
read; ``run_child`` is gemm_exact.run_child on this script and these settings.
"""
import functools
import json
import sys
import time

import torch

import gemm_exact as gx
from gemm_exact import _seed, ints, share_small

ENV_OF = {"wgrad_dma": "CML_WGRAD_DMA", "wgrad_dma_xf": "CML_WGRAD_DMA_XF",
          "wgrad_dma_ns128": "CML_WGRAD_DMA_NS128", "fold_wide_min": "CML_FOLD_WIDE_MIN",
          "wgrad3x3_direct": "CML_WGRAD3X3_DIRECT"}
DEFAULTS = {"wgrad_dma": 1, "wgrad_dma_xf": 1, "wgrad_dma_ns128": 4, "fold_wide_min": 32,
            "wgrad3x3_direct": 1}
DP_NONE, DP_FULL, DP_MASK, DP_BNRELU = 0, 1, 2, 3
BF16_MAX_P = 4096
U32 = 2.0 ** -24


def _lib():
    from consensusml_amd.ops.native import lib
    return lib()


# ------------------------------------------------------------------------------------ the oracle
class Taps:
    """The operand pairs of a weight gradient: dW[:, t, :] = A_t^T B_t, rows = the kernel's
    reduction index. dy [N, Ho, Wo, Co], x [N, H, W, Ci] (NHWC, any float type); taps 9 (3x3,
    padding 1) or 1 (tap (1, 1) alone, no padding), stride 1 or 2."""

    def __init__(self, dy, x, taps=9, stride=1):
        assert taps in (1, 9) and stride in (1, 2) and dy.dim() == 4 and x.dim() == 4
        N, H, W, Ci = x.shape
        assert dy.shape[:3] == (N, H // stride, W // stride) and H % stride == 0 and W % stride == 0
        self.taps, self.stride, self.shape = taps, stride, (N, H, W)
        self.Co, self.Ci = dy.shape[3], Ci
        self.tap0 = 4 if taps == 1 else 0
        self.dy, self.x = dy.double(), x.double()
        self.K = N * H * W // stride ** 2
        self._pad = None

    def _padded(self, t):
        if self._pad is None:
            n, h, w, c = t.shape
            self._pad = torch.zeros(n, h + 2, w + 2, c, dtype=torch.float64)
            self._pad[:, 1:h + 1, 1:w + 1, :] = t
        return self._pad

    def pair(self, t):
        N, H, W = self.shape
        kh, kw = divmod(self.tap0 + t, 3)
        if self.stride == 1:
            B = self.x.reshape(-1, self.Ci)
            if self.taps == 1:
                return self.dy.reshape(-1, self.Co), B
            dyp = self._padded(self.dy)     # dy[p - s]: row h - (kh - 1) of the image = 2 - kh + h
            return dyp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W, :].reshape(-1, self.Co), B
        Ho, Wo = H // 2, W // 2
        xp = self._padded(self.x)           # x[2 o + k - 1]: index 2 o + k of the padded image
        return (self.dy.reshape(-1, self.Co),
                xp[:, kh:kh + 2 * (Ho - 1) + 1:2, kw:kw + 2 * (Wo - 1) + 1:2, :].reshape(-1, self.Ci))

    def sums(self, absolute=False):
        """fp64 [Co, taps, Ci]; absolute: sum_p |dy x| (the fp64 tier's bound)."""
        out = torch.empty(self.Co, self.taps, self.Ci, dtype=torch.float64)
        for t in range(self.taps):
            A, B = self.pair(t)
            out[:, t, :] = (A.abs().t() @ B.abs()) if absolute else (A.t() @ B)
        return out

    def contributions(self, idx):
        """[K, n]: what reduction index k adds to each of the n elements idx = (co, tap, ci)."""
        out = torch.empty(self.K, idx.shape[0], dtype=torch.float64)
        for t in idx[:, 1].unique().tolist():
            sel = (idx[:, 1] == t).nonzero().flatten()
            A, B = self.pair(t)
            out[:, sel] = A[:, idx[sel, 0]] * B[:, idx[sel, 2]]
        return out


def bits_of(mask, C):
    """mask bytes [P, C / 8] -> 0 / 1 [P, C] (bit i of byte j: channel 8 j + i)."""
    sh = torch.arange(8, dtype=torch.uint8)
    return ((mask.unsqueeze(-1) >> sh) & 1).reshape(mask.shape[0], C).double()


def _fma(a, b, c, fused):
    """a b + c -> fp32: one rounding of the fp64 value, or an fp32 product and an fp32 sum."""
    if fused:
        return (a.double() * b.double() + c.double()).float()
    return a.float() * b.float() + c.float()


def stage_x(x, sc, bi, fused=True):
    """The x prologue: bf16(max(x sc + bi, 0)); x [P, Ci] bf16."""
    return _fma(x, sc, bi, fused).clamp_min(0).bfloat16()


def stage_dy(g, dmode, da=None, db=None, dc=None, mask=None, z=None, fused=True):
    """The dy prologues on g [P, Co] bf16: DP_FULL da (m ? g : 0) + (db z + dc), DP_MASK
    da (m ? g : 0) + dc, DP_BNRELU max(g da + db, 0); bf16-rounded once."""
    if dmode == DP_NONE:
        return g
    if dmode == DP_BNRELU:
        return _fma(g, da, db, fused).clamp_min(0).bfloat16()
    gm = g.double() * bits_of(mask, g.shape[1])
    if dmode == DP_MASK:
        return _fma(gm, da, dc, fused).bfloat16()
    return _fma(gm, da, _fma(z, db, dc, fused), fused).bfloat16()


# ------------------------------------------------------------------------------------ the report
def _hist(keys):
    u, n = torch.unique(keys, return_counts=True, dim=0)
    return {tuple(k) if isinstance(k, list) else k: c for k, c in zip(u.tolist(), n.tolist())}


def _in_order(counts):
    return ", ".join(f"{k}: {v}" for k, v in sorted(counts.items()))


def explain(tp, got, want, chunk, sample=48):
    """Whether got - want is +- the contribution of one reduction index (pixel) or of one chunk of
    `chunk` consecutive indices, on (a sample of) the differing elements."""
    d = got.double() - want.double()
    idx = (d != 0).nonzero()
    if idx.shape[0] == 0 or not bool(torch.isfinite(d).all()):
        return "  got - want is not finite" if idx.shape[0] else None
    idx = idx[torch.linspace(0, idx.shape[0] - 1, min(sample, idx.shape[0])).long()]
    dv = d[idx[:, 0], idx[:, 1], idx[:, 2]]
    c = tp.contributions(idx)
    lines = []

    def hits(table, what, unit):
        for sign, verb in ((-1.0, "dropped"), (1.0, "counted twice")):
            h = (table == sign * dv).all(1).nonzero().flatten().tolist()
            if h:
                lines.append(f"  got - want == {verb} {what} {h[:4]}{unit} on {idx.shape[0]} sampled "
                             "differing elements")

    N, H, W = tp.shape
    hits(c, "pixel", f" (reduction index; images of {H // tp.stride} x {W // tp.stride})")
    nch = (tp.K + chunk - 1) // chunk
    cp = torch.zeros(nch * chunk, c.shape[1], dtype=torch.float64)
    cp[:tp.K] = c
    hits(cp.view(nch, chunk, -1).sum(1), "chunk", f" of {chunk} pixels")
    return "\n".join(lines) if lines else "  got - want is no single pixel's or chunk's contribution"


def dw_report(got, want, TM, TN, tp=None, chunk=None, first=8):
    """None when got == want ([Co, taps, Ci]), else the count, the first mismatches, where they
    cluster and (tp given) which pixel or chunk explains them."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    Co, T, Ci = want.shape
    base = gx.mismatch_report(got.reshape(Co, T * Ci), want.reshape(Co, T * Ci), first=0)
    if base is None:
        return None
    idx = (~(got == want)).nonzero()
    lines = [base.splitlines()[0]]
    for co, t, ci in idx[:first].tolist():
        lines.append(f"  (co {co}, tap {t}, ci {ci}) got {float(got[co, t, ci])} want "
                     f"{float(want[co, t, ci])}")
    co, t, ci = idx[:, 0], idx[:, 1], idx[:, 2]
    lines.append("  by tap: " + _in_order(_hist(t)))
    lines.append(f"  by {TM} x {TN} tile (co, ci): " +
                 _in_order(_hist(torch.stack([co // TM, ci // TN], 1))))
    lines.append(f"  by 32-row co block of the tile (co % {TM} // 32): " + _in_order(_hist(co % TM // 32)))
    lines.append(f"  by 64-column ci block of the tile (ci % {TN} // 64): " +
                 _in_order(_hist(ci % TN // 64)))
    if tp is not None:
        lines.append(explain(tp, got, want, chunk))
    return "\n".join(lines)


def assert_dw(got, want, what, TM, TN, tp=None, chunk=None):
    rep = dw_report(got, want, TM, TN, tp, chunk)
    if rep is not None:
        raise AssertionError(f"{what}: {rep}")


def bound_ratio(got, ref, absum, P, splits, bf16, extra=None):
    """max |got - ref| / bound of the fp64 tier (bound 0 and error 0 count as ratio 0)."""
    bound = (P + splits) * U32 * absum + (2.0 ** -8 * ref.abs() if bf16 else 0.0)
    if extra is not None:
        bound = bound + extra
    err = (got.double().cpu() - ref).abs()
    assert bool(torch.isfinite(err).all()), "non-finite output"
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max())


# ------------------------------------------------------------------------------------ operands
def _nhwc(t, dev):
    """[N, H, W, C] CPU tensor -> [N, C, H, W] channels-last view on dev."""
    return t.to(dev).permute(0, 3, 1, 2)


class Guarded:
    """t as a 16-byte-aligned view inside a NaN-filled buffer of its type on dev."""

    def __init__(self, t, dev, pad):
        pad = (pad + 63) // 64 * 64
        self.buf = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device=dev)
        self.view = self.buf[pad:pad + t.numel()].view(t.shape)
        self.view.copy_(t)
        self.pad = pad
        assert self.view.data_ptr() % 16 == 0

    def overwritten(self):
        """guard elements that are no longer NaN"""
        p = self.pad
        return int((~torch.isnan(self.buf[:p])).sum()) + int((~torch.isnan(self.buf[-p:])).sum())


@functools.lru_cache(maxsize=None)
def conv_ref(N, H, W, Co, Ci, taps, stride):
    """(dy, x, Taps, sums) of integers on the CPU; shared, read only."""
    key = (N, H, W, Co, Ci, taps, stride)
    dy = ints((N, H // stride, W // stride, Co), 2, _seed(21, *key))
    x = ints((N, H, W, Ci), 1, _seed(22, *key))
    tp = Taps(dy, x, taps, stride)
    assert 2 * tp.K < 2 ** 24
    return dy, x, tp, tp.sums()


@functools.lru_cache(maxsize=None)
def conv_ref_randn(N, H, W, Co, Ci, taps, stride):
    g = torch.Generator().manual_seed(_seed(23, N, H, W, Co, Ci, taps, stride))
    dy = torch.randn(N, H // stride, W // stride, Co, generator=g).bfloat16()
    x = torch.randn(N, H, W, Ci, generator=g).bfloat16()
    tp = Taps(dy, x, taps, stride)
    return dy, x, tp, tp.sums(), tp.sums(absolute=True)


def _dw(t, Co, taps, Ci):
    """a kernel's dW ([Co, Ci, k, k] channels-last, or flat) as [Co, taps, Ci]"""
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1)
    return t.reshape(Co, taps, Ci)


def _subset(route, want):
    got = {k: route.get(k) for k in want}
    assert got == want, f"route {dict(route)}, expected {want}"


# ------------------------------------------------------------------------------------ 3x3 and s2
def case_conv(dev, kind, N, H, W, Co, Ci, taps, route, bf16=True):
    """wgrad3x3 (kind '3x3') or wgrad3x3s2 (kind 's2'): route, exact fp32 / bf16, guard, fp64."""
    L = _lib()
    stride = 1 if kind == "3x3" else 2
    r = dict(L.wgrad_route(kind, N, H, W, Co, Ci) if kind == "3x3" else
             L.wgrad_route(kind, N, H, W, Co, Ci, taps))
    _subset(r, dict(route, ok=True))
    if kind == "3x3":
        TM, TN, chunk, zn = 64, r["tci"], r["npx"], 8
        run = lambda dy, x, dt, zero: L.wgrad3x3(dy, x, dt, zero)
    else:
        TM, TN, chunk, zn = r["TM"], r["TN"], 32, 256
        run = lambda dy, x, dt, zero: L.wgrad3x3s2(dy, x, dt, zero, taps)
    dy, x, tp, s = conv_ref(N, H, W, Co, Ci, taps, stride)
    P = tp.K
    stats = {"cases": 0, "guard": 0, "share": 1.0, "ratio": 0.0, "ratio32": 0.0}
    if bf16:
        assert P <= BF16_MAX_P
        stats["share"] = share_small(s)
    zero = torch.zeros(zn, dtype=torch.bfloat16, device=dev)
    dyd, xd = _nhwc(dy, dev), _nhwc(x, dev)
    for dt in (torch.float32, torch.bfloat16)[:2 if bf16 else 1]:
        assert_dw(_dw(run(dyd, xd, dt, zero), Co, taps, Ci), s.to(dt), f"exact {dt}", TM, TN, tp, chunk)
        stats["cases"] += 1
    # guard: a row of pixels and one more on either side of each tensor is NaN
    gd = Guarded(dy, dev, 2 * (W + 2) * Co)
    gx_ = Guarded(x, dev, 2 * (W + 2) * Ci)
    gz = Guarded(torch.zeros(zn, dtype=torch.bfloat16), dev, 64)
    got = run(gd.view.permute(0, 3, 1, 2), gx_.view.permute(0, 3, 1, 2), torch.float32, gz.view)
    assert_dw(_dw(got, Co, taps, Ci), s.float(), "guard", TM, TN, tp, chunk)
    stats["guard"] = gd.overwritten() + gx_.overwritten() + gz.overwritten()
    assert stats["guard"] == 0, "a guard element was overwritten"
    stats["cases"] += 1
    # fp64 tier
    dyr, xr, _, ref, absum = conv_ref_randn(N, H, W, Co, Ci, taps, stride)
    dyd, xd = _nhwc(dyr, dev), _nhwc(xr, dev)
    for dt in (torch.float32, torch.bfloat16):
        got = _dw(run(dyd, xd, dt, zero), Co, taps, Ci)
        q = bound_ratio(got, ref, absum, P, r["splits"], dt == torch.bfloat16)
        stats["ratio"] = max(stats["ratio"], q)
        if dt == torch.float32:
            stats["ratio32"] = q
        stats["cases"] += 1
    print(f"  worst error / bound {stats['ratio']:.3e} (fp32 output {stats['ratio32']:.3e})")
    assert stats["ratio"] <= 1.0, f"fp64 tier: error / bound {stats['ratio']:.3f}"
    return stats


# ------------------------------------------------------------------------------------ 1x1
def dyadic(n, seed, scale):
    """scale: values in {+-0.5, +-1, 2}; else multiples of 0.5 with |v| <= 2 (fp32 [n])."""
    g = torch.Generator().manual_seed(seed)
    if scale:
        return torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0])[torch.randint(0, 5, (n,), generator=g)]
    return torch.randint(-4, 5, (n,), generator=g).float() * 0.5


@functools.lru_cache(maxsize=None)
def ref_1x1(P, Co, Ci, pro, dmode, exact):
    """Operands, staged operands, sums, column sums and (fp64 tier) the bound's terms of one
    wgrad1x1 problem on the CPU; shared, read only."""
    key = (P, Co, Ci, int(pro), dmode)
    o = {}
    if exact:
        assert 40 * P < 2 ** 22
        o["dy"], o["x"] = ints((P, Co), 2, _seed(31, *key)), ints((P, Ci), 1, _seed(32, *key))
        o["z"] = ints((P, Co), 2, _seed(33, *key))
        for i, (name, n) in enumerate((("sc", Ci), ("da", Co), ("db", Co))):
            o[name] = dyadic(n, _seed(34 + i, *key), True)
        o["bi"], o["dc"] = dyadic(Ci, _seed(37, *key), False), dyadic(Co, _seed(38, *key), False)
        # the ReLU boundaries: x sc + bi == 0 and g da + db == 0 at (pixel 0, channel 0)
        o["sc"][0], o["bi"][0], o["da"][0], o["dc"][0] = 1.0, -1.0, 1.0, 0.5
        o["x"][0, 0] = 1.0
        if dmode == DP_BNRELU:
            o["db"][0] = -2.0
            o["dy"][0, 0] = 2.0
    else:
        g = torch.Generator().manual_seed(_seed(39, *key))
        o["dy"], o["x"] = torch.randn(P, Co, generator=g).bfloat16(), torch.randn(P, Ci, generator=g).bfloat16()
        o["z"] = torch.randn(P, Co, generator=g).bfloat16()
        o["sc"], o["bi"] = torch.rand(Ci, generator=g) + 0.5, torch.randn(Ci, generator=g) * 0.1
        o["da"], o["db"] = torch.randn(Co, generator=g), torch.randn(Co, generator=g) * 0.5
        o["dc"] = torch.randn(Co, generator=g) * 0.1
    gm = torch.Generator().manual_seed(_seed(40, *key))
    o["mask"] = torch.randint(0, 256, (P, Co // 8), generator=gm, dtype=torch.uint8)

    def staged(fused):
        xs = stage_x(o["x"], o["sc"], o["bi"], fused) if pro else o["x"]
        ds = stage_dy(o["dy"], dmode, o["da"], o["db"], o["dc"], o["mask"], o["z"], fused)
        return ds.double(), xs.double()

    D, X = staged(True)
    o["sums"] = (D.t() @ X).view(Co, 1, Ci)
    o["colsum"] = D.sum(0)
    o["tp"] = Taps(D.view(P, 1, 1, Co), X.view(P, 1, 1, Ci), 1, 1)
    if exact:
        Du, Xu = staged(False)
        assert torch.equal(D, Du) and torch.equal(X, Xu), "dyadic operands: fused == unfused"
        if pro:
            assert float(X[0, 0]) == 0.0
        if dmode == DP_BNRELU:
            assert float(D[0, 0]) == 0.0
    else:
        Du, Xu = staged(False)
        eD, eX = (D - Du).abs(), (X - Xu).abs()
        o["absum"] = (D.abs().t() @ X.abs()).view(Co, 1, Ci)
        o["extra"] = (eD.t() @ X.abs() + D.abs().t() @ eX + eD.t() @ eX).view(Co, 1, Ci)
        o["cs_abs"], o["cs_extra"] = D.abs().sum(0), eD.sum(0)
    return o


def _rows4(t, dev):
    """[P, C] -> the [P, C, 1, 1] channels-last view the bindings take"""
    return t.to(dev).view(t.shape[0], 1, 1, t.shape[1]).permute(0, 3, 1, 2)


def call_1x1(L, o, dev, pro, dmode, colsum, dtype, t=None, out=None):
    """Run the binding that reaches (pro, dmode, colsum): wgrad1x1 for DP_NONE / DP_FULL without
    column sums, else wgrad1x1_ex (fp32). t: replacement device tensors (guard views)."""
    t = t or {}
    dy = t.get("dy", None)
    dy = _rows4(o["dy"], dev) if dy is None else dy
    x = t["x"] if "x" in t else _rows4(o["x"], dev)
    sc, bi = (o["sc"].to(dev), o["bi"].to(dev)) if pro else (None, None)
    f = lambda k: o[k].to(dev)
    if dmode in (DP_NONE, DP_FULL) and not colsum and not (o["dy"].shape[1] == 64 and o["x"].shape[1] == 64):
        if dmode == DP_FULL:
            z = t["z"] if "z" in t else _rows4(o["z"], dev)
            return L.wgrad1x1(dy, x, dtype, sc, bi, z, f("mask"), f("da"), f("db"), f("dc"), out=out), None
        return L.wgrad1x1(dy, x, dtype, sc, bi, out=out), None
    assert dtype == torch.float32 and out is None and dmode != DP_FULL
    return L.wgrad1x1_ex(dy, x, sc, bi, dmode, f("mask") if dmode == DP_MASK else None,
                         f("da") if dmode else None, f("db") if dmode == DP_BNRELU else None,
                         f("dc") if dmode == DP_MASK else None, colsum)


def plain_1x1(Co, Ci, dmode, colsum):
    """whether the call goes through wgrad1x1 (bf16 output, out=) rather than wgrad1x1_ex"""
    return dmode in (DP_NONE, DP_FULL) and not colsum and not (Co == 64 and Ci == 64)


def bf16_exact_1x1(P, Co, Ci, pro, dmode, colsum):
    """whether the exact tier also runs bf16 output: integer sums (no prologue) within the
    share_small range"""
    return plain_1x1(Co, Ci, dmode, colsum) and not pro and dmode == DP_NONE and P <= BF16_MAX_P


def case_1x1(dev, P, Co, Ci, pro, dmode, colsum, route, bf16=None):
    """One wgrad1x1 problem: route, exact (fp32, and bf16 where the binding and P allow), guard
    (inputs, z and out= inside NaN buffers), fp64 tier."""
    L = _lib()
    r = dict(L.wgrad_route("1x1", P, Co, Ci, pro, dmode, colsum))
    _subset(r, dict(route, ok=True))
    TM, TN, chunk = r["TM"], r["TN"], r["KC"]
    plain_binding = plain_1x1(Co, Ci, dmode, colsum)
    if bf16 is None:
        bf16 = bf16_exact_1x1(P, Co, Ci, pro, dmode, colsum)
    o = ref_1x1(P, Co, Ci, pro, dmode, True)
    s, tp = o["sums"], o["tp"]
    stats = {"cases": 0, "guard": 0, "share": 1.0, "ratio": 0.0, "ratio32": 0.0}
    if bf16:
        stats["share"] = share_small(s)
    for dt in (torch.float32, torch.bfloat16)[:2 if bf16 else 1]:
        dw, cs = call_1x1(L, o, dev, pro, dmode, colsum, dt)
        assert_dw(_dw(dw, Co, 1, Ci), s.to(dt), f"exact {dt}", TM, TN, tp, chunk)
        if colsum:
            assert torch.equal(cs.cpu(), o["colsum"].float()), \
                f"column sums: {int((cs.cpu() != o['colsum'].float()).sum())} of {Co} differ"
        stats["cases"] += 1
    # guard
    g = {k: Guarded(o[k].view(P, 1, 1, -1), dev, 4096) for k in ("dy", "x", "z")}
    views = {k: v.view.permute(0, 3, 1, 2) for k, v in g.items()}
    row = None
    if plain_binding:
        row = Guarded(torch.zeros(Co * Ci), dev, 256)
        row.view.fill_(float("nan"))
    dw, cs = call_1x1(L, o, dev, pro, dmode, colsum, torch.float32, views,
                      out=None if row is None else row.view)
    if row is not None:
        assert dw.data_ptr() == row.view.data_ptr()
    assert_dw(_dw(dw, Co, 1, Ci), s.float(), "guard", TM, TN, tp, chunk)
    if colsum:
        assert torch.equal(cs.cpu(), o["colsum"].float()), "guard: column sums"
    stats["guard"] = sum(v.overwritten() for v in g.values()) + (row.overwritten() if row else 0)
    assert stats["guard"] == 0, "a guard element was overwritten"
    stats["cases"] += 1
    # fp64 tier
    f = ref_1x1(P, Co, Ci, pro, dmode, False)
    for dt in (torch.float32, torch.bfloat16)[:2 if plain_binding else 1]:
        dw, cs = call_1x1(L, f, dev, pro, dmode, colsum, dt)
        q = bound_ratio(_dw(dw, Co, 1, Ci), f["sums"], f["absum"], P, r["splits"],
                        dt == torch.bfloat16, f["extra"])
        if colsum:
            q = max(q, bound_ratio(cs, f["colsum"], f["cs_abs"], P, r["splits"], False, f["cs_extra"]))
        stats["ratio"] = max(stats["ratio"], q)
        if dt == torch.float32:
            stats["ratio32"] = q
        stats["cases"] += 1
    print(f"  worst error / bound {stats['ratio']:.3e} (fp32 output {stats['ratio32']:.3e})")
    assert stats["ratio"] <= 1.0, f"fp64 tier: error / bound {stats['ratio']:.3f}"
    return stats


def case_direct(dev, P, Co, Ci):
    """The one-split direct write: fp32 and bf16, with and without out= (inside a NaN row)."""
    L = _lib()
    r = dict(L.wgrad_route("1x1", P, Co, Ci, False, 0, False))
    _subset(r, {"ok": True, "path": "dma", "splits": 1, "direct": True, "fold": "none"})
    o = ref_1x1(P, Co, Ci, False, DP_NONE, True)
    stats = {"cases": 0, "guard": 0, "share": share_small(o["sums"]), "ratio": 0.0,
             "ratio32": 0.0}
    for dt in (torch.float32, torch.bfloat16):
        for use_out in (False, True):
            row = None
            if use_out:
                row = Guarded(torch.zeros(Co * Ci, dtype=dt), dev, 256)
                row.view.fill_(float("nan"))
            dw, _ = call_1x1(L, o, dev, False, DP_NONE, False, dt, out=row.view if row else None)
            assert_dw(_dw(dw, Co, 1, Ci), o["sums"].to(dt), f"direct {dt} out={use_out}",
                      r["TM"], r["TN"], o["tp"], r["KC"])
            if row:
                assert dw.data_ptr() == row.view.data_ptr()
                stats["guard"] += row.overwritten()
            stats["cases"] += 1
    assert stats["guard"] == 0, "a guard element was overwritten"
    return stats


@functools.lru_cache(maxsize=None)
def fold_ref(S, n, bf16):
    """integer partials [S, n] fp32 (|v| < 2^12; bf16: |v| <= 8 so that |sum| < 256) and their
    fp64 sums"""
    g = torch.Generator().manual_seed(_seed(41, S, n, int(bf16)))
    amax = 8 if bf16 else 4095
    part = torch.randint(-amax, amax + 1, (S, n), generator=g).float()
    return part, part.double().sum(0)


def case_fold(dev, S, n, bf16, kind):
    """split_fold of integer partials (|v| < 2^12; bf16: small enough that |sum| < 256) against the
    fp64 sum, bitwise; `kind`: the fold kernel the settings give S."""
    L = _lib()
    wmin = dict(L.wgrad_settings())["fold_wide_min"]
    got_kind = "wide" if wmin > 0 and S >= wmin else "narrow"
    assert got_kind == kind, f"fold of {S} splits is {got_kind}, expected {kind}"
    part, s = fold_ref(S, n, bf16)
    share = share_small(s) if bf16 else 1.0
    want = s.bfloat16() if bf16 else s.float()
    out = L.split_fold(part.to(dev), bf16)
    rep = gx.mismatch_report(out.view(1, n), want.view(1, n))
    assert rep is None, f"fold S={S} n={n}: {rep}"
    return {"cases": 1, "guard": 0, "share": share, "ratio": 0.0, "ratio32": 0.0}


def case_refused3x3(dev, shapes):
    """CML_WGRAD3X3_DIRECT=0: no shape has a plan (host predicates only)."""
    L = _lib()
    for s in shapes:
        assert dict(L.wgrad_route("3x3", *s)) == {"ok": False}, s
        assert not L.wgrad3x3_direct_ok(*s), s
    return {"cases": len(shapes), "guard": 0, "share": 1.0, "ratio": 0.0, "ratio32": 0.0}


# ------------------------------------------------------------------------------------ case tables
CASES = {}


def _reg(name, fn, **kw):
    assert name not in CASES, name
    CASES[name] = functools.partial(fn, **kw)
    return name


# wgrad3x3: (B, H, W, Co, Ci) -> the route fields each case is there for
W3 = [
    # multi-image chunks (G > 1); one chunk, one split (nch = 1), grids below 8
    ((4, 5, 5, 64, 64), {"G": 4, "R": 5, "nch": 1, "splits": 1, "tci": 64, "grid": 1}),
    ((3, 5, 5, 128, 64), {"G": 3, "R": 5, "nch": 1, "tci": 64, "grid": 2}),
    ((4, 7, 7, 64, 128), {"G": 2, "R": 7, "nch": 2, "cps": 1, "tci": 128, "grid": 2}),
    # whole-image chunks (G = 1, R = H: both halo rows dead); grid 10 and 8
    ((5, 5, 5, 128, 128), {"G": 1, "R": 5, "npx": 25, "tci": 128, "grid": 10}),
    ((2, 10, 10, 256, 64), {"G": 1, "R": 10, "npx": 100, "tci": 64, "grid": 8}),
    # single-row images: both halo rows outside the image
    ((11, 1, 16, 64, 64), {"G": 1, "R": 1, "npx": 16, "grid": 11}),
    ((1, 1, 16, 64, 64), {"G": 1, "R": 1, "nch": 1, "grid": 1}),
    # multi-row chunks
    ((2, 14, 14, 128, 256), {"G": 1, "R": 7, "npx": 98, "tci": 128, "grid": 16}),
    ((1, 28, 28, 256, 128), {"G": 1, "R": 4, "npx": 112, "nch": 7, "grid": 28}),
    ((1, 56, 56, 64, 256), {"G": 1, "R": 2, "npx": 112, "dy_rows": 232, "grid": 56}),
    ((1, 16, 16, 256, 256), {"G": 1, "R": 4, "npx": 64, "grid": 32}),
    ((1, 30, 30, 64, 64), {"G": 1, "R": 3, "npx": 90, "grid": 10}),
    # non-square and prime
    ((2, 6, 37, 64, 128), {"G": 1, "R": 3, "npx": 111, "grid": 4}),
    ((1, 13, 9, 128, 128), {"G": 1, "R": 1, "npx": 9, "nch": 13, "grid": 26}),
    # the LDS row limit
    ((1, 64, 2, 64, 64), {"G": 1, "R": 32, "dy_rows": 232}),
    # ragged last split (nch % cps != 0), two chunks per split, grid 144
    ((5, 28, 28, 256, 256), {"R": 4, "nch": 35, "cps": 2, "splits": 18, "grid": 144}),
]
# ragged, grid 132 (no multiple of 8), wide fold; 6500 pixels: fp32 output only
W3_FP32 = [((65, 10, 10, 128, 256), {"G": 1, "R": 10, "nch": 65, "cps": 2, "splits": 33,
                                     "grid": 132, "fold": "wide"})]
W3_REFUSED = [(1, 120, 1, 64, 64), (1, 2, 113, 64, 64), (28, 2, 2, 64, 64)]
_reg("refused3x3", case_refused3x3, shapes=tuple(c for c, _ in W3 + W3_FP32) + tuple(W3_REFUSED))
W3_NAMES = [_reg("w3-%dx%dx%d-co%d-ci%d" % c, case_conv, kind="3x3", N=c[0], H=c[1], W=c[2],
                 Co=c[3], Ci=c[4], taps=9, route=r) for c, r in W3]
W3_NAMES += [_reg("w3-%dx%dx%d-co%d-ci%d" % c, case_conv, kind="3x3", N=c[0], H=c[1], W=c[2],
                  Co=c[3], Ci=c[4], taps=9, route=r, bf16=False) for c, r in W3_FP32]

# stride-2 gather: (N, H, W) of the input. P = 32 in one chunk; one chunk over eight images; image
# boundaries mid-chunk, non-square; several splits
S2_GEOM = [(2, 8, 8), (8, 4, 4), (4, 8, 12), (2, 4, 16), (8, 16, 16)]
S2_STAGES = {(128, 128): 4, (128, 256): 6, (256, 128): 6, (256, 256): 4}
S2_NAMES = []
for _g in S2_GEOM:
    for _co in (128, 256):
        for _ci in (128, 256):
            for _t in (9, 1):
                S2_NAMES.append(_reg(
                    f"s2-{_g[0]}x{_g[1]}x{_g[2]}-co{_co}-ci{_ci}-t{_t}", case_conv, kind="s2", N=_g[0],
                    H=_g[1], W=_g[2], Co=_co, Ci=_ci, taps=_t,
                    route={"TM": _co, "TN": _ci, "stages": S2_STAGES[(_co, _ci)],
                           "splits": _g[0] * _g[1] * _g[2] // 128}))
# several chunks per split: 3 (below the pipeline depth, ragged last split) and 10 (steady state)
S2_NAMES.append(_reg("s2-8x16x16-co512-ci512-t9", case_conv, kind="s2", N=8, H=16, W=16, Co=512,
                     Ci=512, taps=9, route={"TM": 256, "TN": 256, "cps": 3, "splits": 6}))
S2_NAMES.append(_reg("s2-32x16x16-co512-ci512-t9", case_conv, kind="s2", N=32, H=16, W=16, Co=512,
                     Ci=512, taps=9, route={"TM": 256, "TN": 256, "cps": 10, "splits": 7}))
# the 128 x 128 tile's ring in its steady state: 11 chunks per split over 4 stages
S2_NAMES.append(_reg("s2-32x16x16-co384-ci384-t9", case_conv, kind="s2", N=32, H=16, W=16, Co=384,
                     Ci=384, taps=9, route={"TM": 128, "TN": 128, "stages": 4, "cps": 11, "splits": 6}))
S2_REFUSED = [(3, 7, 7, 128, 128), (1, 10, 10, 128, 128), (8, 16, 16, 64, 128), (8, 16, 16, 128, 64)]


def _st(TM, TN, **kw):
    return dict({"path": "staged", "TM": TM, "TN": TN, "KC": 64}, **kw)


def _dma(TM, TN, **kw):
    return dict({"path": "dma", "TM": TM, "TN": TN, "KC": 32}, **kw)


def _c1(tag, P, Co, Ci, pro, dmode, colsum, route):
    return _reg(f"{tag}-p{P}-co{Co}-ci{Ci}-x{int(pro)}-d{dmode}-cs{int(colsum)}", case_1x1, P=P,
                Co=Co, Ci=Ci, pro=pro, dmode=dmode, colsum=colsum, route=route)


# staged kernel, tail chunk (clamped prefetch): P below, at and past the 64-pixel chunk
C1_TAIL = [_c1("tail", P, 128, 128, False, 0, False, _st(128, 128)) for P in (1, 63, 64, 65, 147, 200)]
# staged kernel, every tile; 2048 x 1024 with 4 chunks per split (the steady-state loop)
C1_TILES = [_c1("tile", 200, 64, 64, False, 0, False, _st(64, 64)),
            _c1("tile", 200, 256, 64, False, 0, False, _st(256, 64)),
            _c1("tile", 200, 512, 512, False, 0, False, _st(128, 128)),
            _c1("tile", 200, 256, 256, False, 0, False, _st(256, 256)),
            _c1("tile", 200, 256, 256, True, 0, False, _st(256, 128)),
            _c1("tile", 1000, 2048, 1024, False, 0, False, _st(128, 128, cps=4, splits=4))]
# staged kernel, dy prologues x the x prologue (x column sums where the binding has them)
C1_DPRO = []
for _pro in (False, True):
    C1_DPRO.append(_c1("dpro", 147, 256, 128, _pro, DP_FULL, False, _st(256, 128)))
    for _cs in (False, True):
        C1_DPRO.append(_c1("dpro", 147, 256, 128, _pro, DP_MASK, _cs, _st(256, 128)))
        C1_DPRO.append(_c1("dpro", 147, 128, 256, _pro, DP_BNRELU, _cs, _st(128, 256)))
        C1_DPRO.append(_c1("dpro", 147, 256, 256, _pro, DP_BNRELU, _cs, _st(256, 128)))
C1_DPRO.append(_c1("dpro", 147, 64, 64, True, DP_BNRELU, True, _st(64, 64)))
C1_DPRO.append(_c1("dpro", 147, 256, 64, False, 0, True, _st(256, 64)))
# LDS-DMA kernel, plain: the three tiles at one, three and 64 chunks (wide fold at 64 splits)
C1_DMA = [_c1("dma", P, Co, Ci, False, 0, False,
              _dma(Co, Ci, splits=P // 32, fold="none" if P == 32 else ("wide" if P == 2048 else "narrow")))
          for P in (32, 96, 2048) for Co, Ci in ((256, 256), (128, 256), (256, 128))]
C1_DMA.append(_c1("dma", 2048, 1024, 1024, False, 0, False, _dma(256, 256, cps=4, splits=16)))
# LDS-DMA kernel, in-LDS prologues
C1_DMA_XF = [_c1("xf", 96, 256, 256, True, 0, False, _dma(256, 256)),
             _c1("xf", 96, 128, 256, True, 0, False, _dma(128, 256)),
             _c1("xf", 2048, 1024, 1024, True, DP_MASK, True, _dma(256, 256, cps=4, splits=16))]
for _cs in (False, True):
    C1_DMA_XF.append(_c1("xf", 96, 256, 256, False, DP_MASK, _cs, _dma(256, 256)))
    C1_DMA_XF.append(_c1("xf", 96, 256, 256, True, DP_MASK, _cs, _dma(256, 256)))
# declined: a prologue on a TN = 128 tile stays on the staged kernel
C1_DECLINED = [_c1("declined", 96, 256, 128, True, 0, False, _st(256, 128)),
               _c1("declined", 96, 256, 128, False, DP_MASK, False, _st(256, 128))]
DIRECT_NAMES = [_reg("direct-p32-co256-ci256", case_direct, P=32, Co=256, Ci=256)]

FOLD_S, FOLD_N = (1, 31, 32, 33, 129), (64, 4100, 65536)


def fold_names(wmin):
    """the fold cases under CML_FOLD_WIDE_MIN = wmin (registered on first use)"""
    names = []
    for S in FOLD_S:
        for n in FOLD_N:
            for bf in (False, True):
                kind = "wide" if wmin > 0 and S >= wmin else "narrow"
                name = f"fold-{kind}-s{S}-n{n}-{'bf16' if bf else 'fp32'}"
                if name not in CASES:
                    _reg(name, case_fold, S=S, n=n, bf16=bf, kind=kind)
                names.append(name)
    return names


FOLD_NAMES = fold_names(32)
FOLD_ALL_WIDE, FOLD_ALL_NARROW = fold_names(1), fold_names(0)

# the environment children's subsets: the cases as they route under each switch
ENV_DMA_OFF = [_c1("env-dma0", 96, 256, 256, False, 0, False, _st(256, 256)),
               _c1("env-dma0", 2048, 128, 256, False, 0, False, _st(128, 256)),
               _c1("env-dma0", 96, 256, 256, True, DP_MASK, True, _st(256, 128))]
ENV_XF_OFF = [_c1("env-xf0", 96, 256, 256, True, 0, False, _st(256, 128)),
              _c1("env-xf0", 96, 256, 256, True, DP_MASK, True, _st(256, 128)),
              _c1("env-xf0", 96, 256, 256, False, DP_MASK, False, _st(256, 128)),
              "dma-p96-co256-ci256-x0-d0-cs0"]
ENV_NS128 = [_reg(f"env-ns8-{n}x{h}x{w}-t{t}", case_conv, kind="s2", N=n, H=h, W=w, Co=128, Ci=128,
                  taps=t, route={"TM": 128, "TN": 128, "stages": 8})
             for (n, h, w) in ((2, 8, 8), (4, 8, 12), (8, 16, 16)) for t in (9, 1)]
# (11 chunks per split: past the 8-stage ring)
ENV_NS128.append(_reg("env-ns8-32x16x16-co384-t9", case_conv, kind="s2", N=32, H=16, W=16, Co=384,
                      Ci=384, taps=9, route={"TM": 128, "TN": 128, "stages": 8, "cps": 11, "splits": 6}))


def bf16_sums(name):
    """The reference sums of a case whose exact tier compares a bf16 output (share_small is
    asserted on them), else None."""
    fn = CASES[name]
    kw = fn.keywords
    if fn.func is case_conv and kw.get("bf16", True):
        return conv_ref(kw["N"], kw["H"], kw["W"], kw["Co"], kw["Ci"], kw["taps"],
                        1 if kw["kind"] == "3x3" else 2)[3]
    if fn.func is case_direct or (fn.func is case_1x1 and (
            bf16_exact_1x1(kw["P"], kw["Co"], kw["Ci"], kw["pro"], kw["dmode"], kw["colsum"])
            if kw.get("bf16") is None else kw["bf16"])):
        return ref_1x1(kw["P"], kw["Co"], kw["Ci"], False, DP_NONE, True)["sums"]
    if fn.func is case_fold and kw["bf16"]:
        return fold_ref(kw["S"], kw["n"], True)[1]
    return None


# ------------------------------------------------------------------------------------ running
def check_settings(expect):
    """wgrad_settings() must be the defaults overridden by `expect` and nothing else."""
    got = dict(_lib().wgrad_settings())
    want = dict(DEFAULTS, **expect)
    assert got == want, f"wgrad_settings() {got}, expected {want}"
    return got


TOTALS = {}


def run_case(name, dev):
    """Run one case; returns its figures. Raises on a mismatch."""
    t0 = time.perf_counter()
    st = CASES[name](dev)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    fam = name.split("-")[0]
    tot = TOTALS.setdefault(fam, {"cases": 0, "guard": 0, "share": 1.0, "ratio": 0.0, "ratio32": 0.0})
    for k in ("cases", "guard"):
        tot[k] += st[k]
    tot["share"] = min(tot["share"], st["share"])
    for k in ("ratio", "ratio32"):
        tot[k] = max(tot[k], st[k])
    print(f"{name}: {dt:.2f} s, {st['cases']} runs, |s| < 256 share {st['share']:.4%}, worst error / "
          f"bound {st['ratio']:.3e} (fp32 output {st['ratio32']:.3e}), guard elements overwritten "
          f"{st['guard']}")
    print("FAMILY " + json.dumps({fam: tot}))
    return st, dt


def check_route(name):
    """The case's route alone (no GPU: wgrad_route only evaluates host predicates)."""
    kw = CASES[name].keywords
    L = _lib()
    if "shapes" in kw:
        CASES[name](None)
    elif "kind" in kw and "N" in kw:
        args = (kw["N"], kw["H"], kw["W"], kw["Co"], kw["Ci"]) + ((kw["taps"],) if kw["kind"] == "s2" else ())
        _subset(dict(L.wgrad_route(kw["kind"], *args)), dict(kw["route"], ok=True))
    elif "route" in kw:
        _subset(dict(L.wgrad_route("1x1", kw["P"], kw["Co"], kw["Ci"], kw["pro"], kw["dmode"],
                                   kw["colsum"])), dict(kw["route"], ok=True))
    elif "S" in kw:
        wmin = dict(L.wgrad_settings())["fold_wide_min"]
        assert ("wide" if wmin > 0 and kw["S"] >= wmin else "narrow") == kw["kind"], name
    else:
        _subset(dict(L.wgrad_route("1x1", kw["P"], kw["Co"], kw["Ci"], False, 0, False)),
                {"ok": True, "path": "dma", "splits": 1, "direct": True})


def run_child(expect, names, routes_only=False):
    return gx.run_child(expect, names, routes_only, script=__file__, env_of=ENV_OF, defaults=DEFAULTS)


def _main():
    job = json.loads(sys.argv[1])
    settings = check_settings(job["expect"])
    for name in job["cases"]:
        out = {"name": name, "ok": True, "report": None, "settings": settings}
        t0 = time.perf_counter()
        try:
            if job.get("routes_only"):
                check_route(name)
            else:
                out["stats"], _ = run_case(name, torch.device("cuda", 0))
        except AssertionError as e:
            out["ok"], out["report"] = False, str(e)[:4000]
        out["seconds"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    _main()
