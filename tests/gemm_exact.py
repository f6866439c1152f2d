"""Bit-exact oracles of the MFMA GEMM pipelines (gemm.hip, gemm128.hip, gemm_w4.hip,
conv_gemm.hip) and the case tables of ``test_gemm_exact_gpu.py``, ``test_gemm_exact_env_gpu.py``
and ``test_conv_gemm_exact_gpu.py`` (not collected: no ``test_`` prefix).

Why the oracle is exact. Operands are bf16 tensors of small integers from a seeded CPU generator:
A side in [-2, 2], B side (weights) in [-1, 1], bias in [-3, 3], cin in [-4, 4]. A product of two
such values is an integer, exact in fp32; for K <= 4608 every partial sum in any order has
|s| <= 2 K < 2^24, so the fp32 accumulator is exact whatever the MFMA shape, the K order or the
number of pipeline stages. The kernel's output must therefore EQUAL bf16_rne(exact) (pk_bf16 /
f2bf are v_cvt_pk_bf16_f32, round to nearest even). ``expected`` forms the sum in fp64, adds the
bias in fp64 and converts once to bf16 (the fp64 -> fp32 step of that conversion is exact: the
values are integers below 2^24); with cin it converts, adds cin in fp64 and converts again -- the
two rounding points gemm.hip documents. The comparison is ``torch.equal``: no tolerance. Random
integers are asymmetric in row, column and K index, so a swapped, shifted, dropped or duplicated
16-byte chunk changes the sums.

Condition on the inputs (``share_small``): at least 99 % of the expected values must have
|s| < 256 -- integers bf16 holds exactly, so an error of one cannot hide in the output rounding.
It is asserted from the reference alone, before the kernel's output is looked at.

Conv reference (``conv_sums``): nine shifted (strided) slices of a zero-padded NHWC tensor, one
fp64 matmul per tap. Not F.conv2d: a library algorithm that transforms the operands need not be
exact even on integers.

On a mismatch ``assert_exact`` raises with the count, the first few (row, col, got, want) and
histograms by 256 x 256 tile, 16-row block and 64-column block, so that the log alone localises a
wave, a fragment or a K-tile.

Child mode: ``python gemm_exact.py '{"expect": {...}, "cases": [...]}'`` runs the named
cases in the environment it was started in and prints one JSON line per case: name, pass / fail,
the mismatch report, the shares, the seconds and the dispatch values the process actually read.
``run_child`` starts it as a fresh process (one at a time) and checks all of that.
"""
import functools
import json
import os
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the read-once dispatch values (``dispatch_settings()``), their variables and defaults
ENV_OF = {"gemm_gm": "CML_GEMM_GM", "w4_sched": "CML_W4_SCHED", "gemm2_tall": "CML_GEMM2_TALL",
          "conv_gemm_variant": "CML_CONV_GEMM_VARIANT", "conv_gemm_narrow": "CML_CONV_GEMM_NARROW",
          "conv_gemm_smallm": "CML_CONV_GEMM_SMALLM", "conv_gemm_smallv": "CML_CONV_GEMM_SMALLV",
          "conv_gemm2": "CML_CONV_GEMM2", "gemm2_s2": "CML_GEMM2_S2"}
DEFAULTS = {"gemm_gm": 4, "w4_sched": 0, "gemm2_tall": 1024, "conv_gemm_variant": 4,
            "conv_gemm_narrow": 0, "conv_gemm_smallm": 512, "conv_gemm_smallv": 0, "conv_gemm2": 1,
            "gemm2_s2": 1}
MIN_SMALL_SHARE = 0.99


def _lib():
    from consensusml_amd.ops.native import lib
    return lib()


# ------------------------------------------------------------------------------------ the oracle
def ints(shape, amax, seed):
    """bf16 integers in [-amax, amax] from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amax, amax + 1, tuple(shape), generator=g).bfloat16()


def expected(s, bias=None, cin=None):
    """bf16_rne(s + bias) [then bf16_rne(. + cin)] of exact fp64 sums s [M, N]."""
    v = s if bias is None else s + bias.double()
    y = v.bfloat16()
    if cin is not None:
        y = (y.double() + cin.double()).bfloat16()
    return y


def share_small(v):
    """The share of |v| < 256 (integers bf16 holds exactly); asserted >= 99 %."""
    share = float((v.abs() < 256).double().mean())
    assert share >= MIN_SMALL_SHARE, f"only {share:.4%} of the expected values have |s| < 256"
    return share


def conv_sums(x, w, taps, stride):
    """Exact fp64 sums [Nimg OH OW, Co] of a 3x3 / padding 1 (taps 9) or 1x1 (taps 1) conv of
    x [Nimg, H, W, C] with w [Co, taps C] (k = tap C + c, tap = 3 ky + kx)."""
    Nimg, H, W, C = x.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    xd, wd = x.double(), w.double()
    if taps == 1:
        return xd[:, ::stride, ::stride, :].reshape(-1, C) @ wd.t()
    xp = torch.zeros(Nimg, H + 2, W + 2, C, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1, :] = xd
    s = torch.zeros(Nimg * OH * OW, w.shape[0], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            tap = 3 * ky + kx
            sl = xp[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride, :]
            s += sl.reshape(-1, C) @ wd[:, tap * C:(tap + 1) * C].t()
    return s


def _top(counts, n=12):
    items = sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))
    return ", ".join(f"{k}: {v}" for k, v in items[:n]) + (" ..." if len(items) > n else "")


def mismatch_report(got, want, first=8):
    """None when got == want, else the count, the first mismatches and where they cluster."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    bad = ~(got == want)
    idx = bad.nonzero()
    lines = [f"{idx.shape[0]} of {bad.numel()} elements differ"]
    for r, c in idx[:first].tolist():
        lines.append(f"  (row {r}, col {c}) got {float(got[r, c])} want {float(want[r, c])}")
    rows, cols = idx[:, 0], idx[:, 1]

    def hist(keys):
        u, n = torch.unique(keys, return_counts=True, dim=0)
        return {tuple(k) if isinstance(k, list) else k: c for k, c in zip(u.tolist(), n.tolist())}

    def in_order(counts):
        return ", ".join(f"{k}: {v}" for k, v in sorted(counts.items()))

    lines.append("  by 256 x 256 tile (m, n), most hit first: " +
                 _top(hist(torch.stack([rows // 256, cols // 256], 1))))
    lines.append("  by 16-row block of the tile (row % 256 // 16): " +
                 in_order(hist(rows % 256 // 16)))
    lines.append("  by 64-column block of the tile (col % 256 // 64): " +
                 in_order(hist(cols % 256 // 64)))
    return "\n".join(lines)


def assert_exact(got, want, what):
    rep = mismatch_report(got, want)
    if rep is not None:
        raise AssertionError(f"{what}: {rep}")


def _seed(*key):
    h = 1469598103
    for k in key:
        h = (h * 1000003 + int(k)) % (2 ** 31 - 1)
    return h


# ------------------------------------------------------------------------------------ GEMM cases
@functools.lru_cache(maxsize=None)
def gemm_ref(M, N, K):
    """(A [M, K], B [N, K], bias [N], cin [M, N], sums fp64 [M, N]) on the CPU; shared, read only."""
    assert K <= 4608
    A, B = ints((M, K), 2, _seed(1, M, N, K)), ints((N, K), 1, _seed(2, M, N, K))
    bias, cin = ints((N,), 3, _seed(3, M, N, K)), ints((M, N), 4, _seed(4, M, N, K))
    return A, B, bias, cin, A.double() @ B.double().t()


def _wide(t, left, right, seed):
    """A buffer of other integers, `left` / `right` columns wider, holding t as a column slice."""
    big = ints((t.shape[0], left + t.shape[1] + right), 2, seed)
    big[:, left:left + t.shape[1]] = t
    return big


def case_nt(dev, M, N, K, tile):
    """gemm_nt EP_STORE on the 256 x 256 (gemm.hip) or 128 x 128 (gemm128.hip) tile: plain, with
    bias, bias + cin aliasing out, and row-strided a / b / out."""
    L = _lib()
    A, B, bias, cin, s = gemm_ref(M, N, K)
    want = {"plain": expected(s), "bias": expected(s, bias), "cin": expected(s, bias, cin)}
    shares = {"plain": share_small(s), "bias": share_small(s + bias.double()),
              "cin": share_small(want["bias"].double() + cin.double())}
    a, b, bd = A.to(dev), B.to(dev), bias.to(dev)
    assert_exact(L.gemm_nt(a, b, 0, tile=tile), want["plain"], "plain")
    assert_exact(L.gemm_nt(a, b, 0, bias=bd, tile=tile), want["bias"], "bias")
    yc = cin.to(dev)
    y = L.gemm_nt(a, b, 0, bias=bd, out=yc, cin=yc, tile=tile)
    assert y.data_ptr() == yc.data_ptr()
    assert_exact(yc, want["cin"], "bias + cin in place")
    Ab = _wide(A, 64, 0, _seed(5, M, N, K)).to(dev)
    Bb = _wide(B, 0, 72, _seed(6, M, N, K)).to(dev)
    Y = torch.zeros(M, 3 * N, dtype=torch.bfloat16, device=dev)
    L.gemm_nt(Ab[:, 64:], Bb[:, :K], 0, out=Y[:, N:2 * N], tile=tile)
    assert_exact(Y[:, N:2 * N], want["plain"], "row-strided a, b, out")
    assert int(torch.count_nonzero(Y[:, :N])) == 0 and int(torch.count_nonzero(Y[:, 2 * N:])) == 0, \
        "row-strided out: a neighbouring column was written"
    return shares


def case_gelu(dev, M, N, K):
    """EP_GELU: aux (h) bitwise, y against gelu of the kernel's own h (test_gemm_bias_gelu's
    tolerance)."""
    L = _lib()
    A, B, bias, _, s = gemm_ref(M, N, K)
    share = share_small(s + bias.double())
    h = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    y = L.gemm_nt(A.to(dev), B.to(dev), 1, bias=bias.to(dev), aux=h)
    assert_exact(h, expected(s, bias), "h = bf16(acc + bias)")
    torch.testing.assert_close(y.float(), F.gelu(h.float()).bfloat16().float(), rtol=8e-3, atol=1e-5)
    return {"h": share}


def case_dgelu(dev, M, N, K, nseg):
    """EP_DGELU: dh against gelu' of the stored h times the exact bf16 g, and the column sums
    against the fp64 sums of the kernel's own dh per segment (test_gemm_dgelu_colsum's
    tolerances)."""
    L = _lib()
    A, B, _, _, s = gemm_ref(M, N, K)
    share = share_small(s)
    g0 = torch.Generator().manual_seed(_seed(7, M, N, K))
    h = ((torch.rand(M, N, generator=g0) * 2 - 1) * 3.0).bfloat16().to(dev)
    a, b = A.to(dev), B.to(dev)
    cs = torch.empty(nseg, N, dtype=torch.float32, device=dev)
    dh = L.gemm_nt(a, b, 2, aux=h, colsum_out=cs)
    gb = expected(s).to(dev)
    hf = h.float().requires_grad_(True)
    F.gelu(hf).backward(gb.float())
    torch.testing.assert_close(dh.float(), hf.grad.bfloat16().float(), rtol=1.6e-2, atol=1e-4)
    seg = dh.double().view(nseg, M // nseg, N).sum(1)
    torch.testing.assert_close(cs.double(), seg, rtol=1e-4, atol=1e-3)
    return {"g": share}


def w4_ops(mode, A, B):
    """A [M, K], B [N, K] -> the stored operands of `mode` (bit 0: a is [K, M]; bit 1: b [K, N])."""
    return (A.t().contiguous() if mode & 1 else A), (B.t().contiguous() if mode & 2 else B)


def case_w4(dev, mode, M, N, K):
    """gemm_w4: plain, bias, bias + cin in place; out is the interior of a larger zero buffer and
    nothing outside [M, N] may be written."""
    L = _lib()
    A, B, bias, cin, s = gemm_ref(M, N, K)
    want = {"plain": expected(s), "bias": expected(s, bias), "cin": expected(s, bias, cin)}
    shares = {"plain": share_small(s), "bias": share_small(s + bias.double()),
              "cin": share_small(want["bias"].double() + cin.double())}
    a, b = (t.to(dev) for t in w4_ops(mode, A, B))
    bd = bias.to(dev)
    for what in ("plain", "bias", "cin"):
        big = torch.zeros(M + 16, N + 16, dtype=torch.bfloat16, device=dev)
        out = big[8:8 + M, 8:8 + N]
        if what == "cin":
            out.copy_(cin)
            y = L.gemm_w4(a, b, mode, out=out, bias=bd, cin=out)
        else:
            y = L.gemm_w4(a, b, mode, out=out, bias=bd if what == "bias" else None)
        assert y.data_ptr() == out.data_ptr()
        assert_exact(out, want[what], f"mode {mode} {what}")
        out.zero_()
        assert int(torch.count_nonzero(big)) == 0, f"mode {mode} {what}: wrote outside [M, N]"
    return shares


# ------------------------------------------------------------------------------------ conv cases
@functools.lru_cache(maxsize=None)
def conv_ref(Nimg, C, Co, H, W, taps, stride):
    """(x [Nimg, H, W, C], w [Co, taps C], sums fp64 [M, Co]) on the CPU; shared, read only."""
    assert taps * C <= 4608
    key = (Nimg, C, Co, H, W, taps, stride)
    x, w = ints((Nimg, H, W, C), 2, _seed(11, *key)), ints((Co, taps * C), 1, _seed(12, *key))
    return x, w, conv_sums(x, w, taps, stride)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def case_conv(dev, Nimg, C, Co, H, W, taps, stride, route):
    """conv_gemm bitwise against conv_sums on the route asserted first; conv_gemm_bn (and at
    stride 1 conv_gemm_bnsums) must store the same y, with statistics / sums within
    test_conv_gemm2_gpu.py's tolerances of the fp64 values of the kernel's own output."""
    L = _lib()
    got_route = tuple(L.conv_gemm_route(Nimg, H, W, C, Co, taps, stride))
    assert got_route == tuple(route), f"route {got_route}, expected {tuple(route)}"
    x, w, s = conv_ref(Nimg, C, Co, H, W, taps, stride)
    share = share_small(s)
    want = expected(s)
    xd = x.to(dev).permute(0, 3, 1, 2)          # [Nimg, C, H, W], channels-last memory
    wd = w.to(dev)
    zero = torch.zeros(256, dtype=torch.bfloat16, device=dev)
    y = L.conv_gemm(xd, wd, taps, zero, stride)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert tuple(y.shape) == (Nimg, Co, OH, OW)
    assert_exact(_rows(y), want, "conv_gemm")
    # BN statistics epilogue
    rm, rv = torch.zeros(Co, device=dev), torch.ones(Co, device=dev)
    y2, mean, invstd = L.conv_gemm_bn(xd, wd, taps, zero, rm, rm, rv, 1e-5, 0.1, stride)
    assert_exact(_rows(y2), want, "conv_gemm_bn y")
    Y = _rows(y).double()
    print(f"  mean err {float((mean.double() - Y.mean(0)).abs().max()):.3e} invstd err "
          f"{float((invstd.double() - (Y.var(0, unbiased=False) + 1e-5).rsqrt()).abs().max()):.3e}")
    torch.testing.assert_close(mean.double(), Y.mean(0), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(invstd.double(), (Y.var(0, unbiased=False) + 1e-5).rsqrt(),
                               rtol=1e-3, atol=1e-3)
    if stride == 1:
        # BN + ReLU backward sums epilogue (z: the forward's conv output, any values)
        g0 = torch.Generator().manual_seed(_seed(13, Nimg, C, Co, H, W, taps))
        z = torch.randn(Nimg, H, W, Co, generator=g0).bfloat16().to(dev).permute(0, 3, 1, 2)
        gam = (torch.rand(Co, generator=g0) + 0.5).bfloat16().to(dev)
        bet = (torch.randn(Co, generator=g0) * 0.1).bfloat16().to(dev)
        Z = _rows(z).double()
        zmean = Z.mean(0).float()
        zinv = (Z.var(0, unbiased=False) + 1e-5).rsqrt().float()
        sc = gam.float() * zinv
        bi = bet.float() - zmean * sc
        y3, sdz, sdzx = L.conv_gemm_bnsums(xd, wd, taps, zero, z, sc, bi, zmean, zinv)
        assert_exact(_rows(y3), want, "conv_gemm_bnsums y")
        m = (torch.addcmul(bi, _rows(z), sc) > 0).double()
        dyv = Y * m
        qref = (dyv * (Z - zmean.double()) * zinv.double()).sum(0)
        print(f"  sdz err {float((sdz.double() - dyv.sum(0)).abs().max()):.3e} sdzx err "
              f"{float((sdzx.double() - qref).abs().max()):.3e}")
        torch.testing.assert_close(sdz.double(), dyv.sum(0), rtol=1e-5, atol=1e-3)
        torch.testing.assert_close(sdzx.double(), qref, rtol=1e-5, atol=1e-3)
    return {"y": share}


# ------------------------------------------------------------------------------------ case tables
# gemm_nt, 256 x 256 tile: one tile at nk = 1, 2, 3, 4, 7 (the prologue's clamp; odd and even
# buffer parity at exit); 5 m-tiles x 3 (a ragged gm group, G = 15: the XCD remap's G % 8 != 0);
# G = 7 < 8 tiles; two full groups + a ragged one
NT256 = [(256, 256, 64), (256, 256, 128), (256, 256, 192), (256, 256, 256), (256, 256, 448),
         (1280, 768, 192), (1792, 256, 128), (2304, 512, 320)]
NT128 = [(128, 128, 64), (128, 128, 128), (128, 128, 192), (128, 128, 448), (384, 640, 192)]
GELU = [(256, 256, 192), (1280, 768, 192)]
DGELU = [(1280, 768, 192, 1), (1280, 768, 192, 5)]
# gemm_w4: 32-deep sub-stages, the 4-deep ring wraps from K = 192; ragged M / N; 6 m-tiles (a
# ragged group of kGM = 4) with ragged rows
W4 = [(256, 256, 64), (256, 256, 128), (256, 256, 192), (256, 256, 256), (256, 256, 320),
      (256, 256, 576), (296, 520, 320), (8, 264, 192), (1288, 264, 192)]

CASES = {}
for _M, _N, _K in NT256:
    CASES[f"nt256-{_M}x{_N}x{_K}"] = functools.partial(case_nt, M=_M, N=_N, K=_K, tile=256)
for _M, _N, _K in NT128:
    CASES[f"nt128-{_M}x{_N}x{_K}"] = functools.partial(case_nt, M=_M, N=_N, K=_K, tile=128)
for _M, _N, _K in GELU:
    CASES[f"gelu-{_M}x{_N}x{_K}"] = functools.partial(case_gelu, M=_M, N=_N, K=_K)
for _M, _N, _K, _S in DGELU:
    CASES[f"dgelu-{_M}x{_N}x{_K}-seg{_S}"] = functools.partial(case_dgelu, M=_M, N=_N, K=_K, nseg=_S)
for _mode in range(4):
    for _M, _N, _K in W4:
        CASES[f"w4-mode{_mode}-{_M}x{_N}x{_K}"] = functools.partial(case_w4, mode=_mode, M=_M,
                                                                     N=_N, K=_K)
NT256_NAMES = [n for n in CASES if n.startswith("nt256-")]
NT128_NAMES = [n for n in CASES if n.startswith("nt128-")]
GELU_NAMES = [n for n in CASES if n.startswith(("gelu-", "dgelu-"))]
W4_NAMES = [n for n in CASES if n.startswith("w4-")]


def conv_name(Nimg, C, Co, H, W, taps, stride, route):
    return f"conv-{Nimg}x{C}x{Co}-{H}x{W}-t{taps}-s{stride}@{route[0]}-{route[1]}x{route[2]}"


def conv_cases(shapes, route, taps=9, stride=1):
    """Register (images, C, Co, H, W) conv cases on `route`; returns their names."""
    names = []
    for Nimg, C, Co, H, W in shapes:
        name = conv_name(Nimg, C, Co, H, W, taps, stride, route)
        CASES[name] = functools.partial(case_conv, Nimg=Nimg, C=C, Co=Co, H=H, W=W, taps=taps,
                                        stride=stride, route=route)
        names.append(name)
    return names


# the square-tile shapes: layer-3 / 4 channel counts, 7 x 7 images (8-row staging groups and
# tiles straddle image boundaries), H != W
SQUARE = [(4, 64, 256, 16, 16), (4, 256, 256, 16, 16), (16, 512, 512, 8, 8), (256, 64, 256, 7, 7),
          (32, 128, 256, 4, 8)]
RAGGED = (3, 64, 256, 9, 7)       # 189 pixels
# default environment: what small shapes really take. 4 tiles of 256 x 256 < CML_CONV_GEMM_SMALLM
# -> variant CML_CONV_GEMM_SMALLV = 0 (128 x 128); Co = 128 cannot take 256 x 256 tiles and gets
# variant 2 (256 x 128) before the small-M rule is looked at; ragged M
CONV_DEFAULT = (conv_cases([(4, 256, 256, 16, 16)], ("conv_gemm", 128, 128)) +
                conv_cases([(3, 64, 128, 9, 7)], ("conv_gemm", 256, 128)))
# CML_CONV_GEMM_SMALLM=0: gemm.hip's square conv mode (TM = 256)
CONV_GEMM2_SQUARE = conv_cases(SQUARE, ("gemm2", 256, 256))
# CML_CONV_GEMM_SMALLM=0 CML_CONV_GEMM2=0: conv_gemm.hip's own variant 4
CONV_VARIANT4 = conv_cases(SQUARE + [RAGGED], ("conv_gemm", 256, 256))
# CML_GEMM2_TALL=1: gemm.hip's tall tile (TM = 512), stride 1 and the stride-2 gather from even
# and odd inputs (same 16 x 16 output)
CONV_TALL = (conv_cases([(4, 64, 128, 16, 16), (4, 128, 128, 16, 16)], ("gemm2", 512, 128)) +
             conv_cases([(4, 128, 128, 32, 32), (4, 64, 128, 31, 31)], ("gemm2", 512, 128), stride=2))


def conv_ab_cases(k):
    """CML_CONV_GEMM2=0 CML_CONV_GEMM_VARIANT=k CML_CONV_GEMM_NARROW=k: wide (Co = 128) and
    narrow (Co = 192: no multiple of 128, not conv3x3p's) tiles, taps 9 and 1, whole-tile and
    ragged M."""
    wide = ("conv_gemm", 256 if k >= 2 else 128, 128)
    narrow = ("conv_gemm", 128 if k >= 2 else 256, 64)
    names = []
    for Co, route in ((128, wide), (192, narrow)):
        names += conv_cases([(4, 64, Co, 16, 16), (3, 64, Co, 9, 7)], route)
        names += conv_cases([(4, 128, Co, 16, 16), (3, 128, Co, 9, 7)], route, taps=1)
    return names


CONV_AB = {k: conv_ab_cases(k) for k in (1, 2, 3)}


# ------------------------------------------------------------------------------------ running
def check_settings(expect):
    """dispatch_settings() must be the defaults overridden by `expect` and nothing else."""
    got = dict(_lib().dispatch_settings())
    want = dict(DEFAULTS, **expect)
    assert got == want, f"dispatch_settings() {got}, expected {want}"
    return got


def run_case(name, dev):
    """Run one case; returns (shares, seconds). Raises on a mismatch."""
    t0 = time.perf_counter()
    shares = CASES[name](dev)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    print(f"{name}: {dt:.2f} s, |s| < 256 share " +
          ", ".join(f"{k} {v:.4%}" for k, v in shares.items()))
    return shares, dt


def check_route(name):
    """The conv case's route alone (needs no GPU: conv_gemm_route only evaluates predicates)."""
    kw = CASES[name].keywords
    got = tuple(_lib().conv_gemm_route(kw["Nimg"], kw["H"], kw["W"], kw["C"], kw["Co"], kw["taps"],
                                       kw["stride"]))
    assert got == tuple(kw["route"]), f"route {got}, expected {tuple(kw['route'])}"


def run_child(expect, names, routes_only=False, script=None, env_of=None, defaults=None):
    """Run `names` in a fresh process whose environment sets exactly `expect`'s variables, one
    JSON line per case; assert the settings it read and that every case passed. routes_only: the
    child checks the settings and the conv cases' routes and touches no GPU. script / env_of /
    defaults: another oracle's child mode with its own read-once settings (wgrad_oracle.py)."""
    env_of = ENV_OF if env_of is None else env_of
    env = {k: v for k, v in os.environ.items() if k not in env_of.values()}
    env["PYTHONPATH"] = ROOT
    for k, v in expect.items():
        env[env_of[k]] = str(v)
    r = subprocess.run([sys.executable, os.path.abspath(script or __file__),
                        json.dumps({"expect": expect, "cases": list(names),
                                    "routes_only": routes_only})],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"child exit {r.returncode}: {r.stderr[-3000:]}"
    res = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    want = dict(DEFAULTS if defaults is None else defaults, **expect)
    assert [x["name"] for x in res] == list(names), "the child did not run every case"
    for x in res:
        assert x["settings"] == want, (x["name"], x["settings"], want)
    failed = [f"{x['name']}: {x['report']}" for x in res if not x["ok"]]
    assert not failed, "\n".join(failed)
    return res


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
                out["shares"], _ = run_case(name, torch.device("cuda", 0))
        except AssertionError as e:
            out["ok"], out["report"] = False, str(e)[:4000]
        out["seconds"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    _main()
