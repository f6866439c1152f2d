"""conv1's backward with bn1's apply pass inside (``csrc/kernels/conv1_bwd.hip``,
``lib().conv1_bn_bwd``) against the three launches it replaces and an fp64 oracle.

dz1 must equal ``bn_bwd_apply`` bit for bit. dx and dW1 round the same exact quantities as the
parent path (``bn_bwd_apply`` + ``conv1x1_link`` / ``conv1x1_link_s2`` / a plain GEMM +
``wgrad1x1`` / the library weight gradient) and differ from it only in fp32 summation order, which
moves an individual error by about its own size: the new path's error against the fp64 oracle
(built from the bf16 dz1) may be at most 2x the parent's, as a maximum and as a root mean square.
Both errors are printed."""
import pytest
import torch

from consensusml_amd import perf
from consensusml_amd.ops import bn as fbn
from consensusml_amd.ops import native

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (3, 9), (2, 28)]          # (N, H = W): 9 / 243 / 1568 pixels
PC = [(64, 256), (128, 512)]                # (p, Cin): one and two channel slices
S2_SHAPES = [(2, 6), (3, 10)]               # compact stride-2 link, (p, Cin) = (128, 256)


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _inputs(dev, N, H, p, Cin, kind, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed + 1000 * N + 10 * H + p)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    M = N * H * H
    d = {"N": N, "H": H, "p": p, "Cin": Cin, "M": M, "kind": kind}
    d["dy"] = _nhwc(rn(N, p, H, H).bfloat16())
    d["z"] = _nhwc((rn(N, p, H, H) * 1.5 + 0.3).bfloat16())
    d["x"] = _nhwc(rn(N, Cin, H, H).relu().bfloat16())
    d["w"] = (rn(p, Cin) * Cin ** -0.5).bfloat16()
    gamma = torch.empty(p, device=dev).uniform_(0.5, 1.5, generator=gen)
    gamma[1::7] *= -1.0                      # negative and exactly zero entries: the mask is
    gamma[3::11] = 0.0                       # recomputed from fmaf(z, sc, bi) > 0
    d["gamma"] = gamma.bfloat16()
    d["beta"] = torch.empty(p, device=dev).uniform_(-0.3, 0.3, generator=gen).bfloat16()
    zf = d["z"].float().permute(0, 2, 3, 1).reshape(M, p)
    d["mean"] = zf.mean(0).contiguous()
    d["invstd"] = (zf.var(0, unbiased=False) + 1e-5).rsqrt().contiguous()
    # bn1's backward sums by a real reduction of the same dy1 / z1
    sc = d["invstd"] * d["gamma"].float()
    bi = d["beta"].float() - d["mean"] * sc
    dyf = d["dy"].float().permute(0, 2, 3, 1).reshape(M, p)
    dm = torch.where(zf * sc + bi > 0, dyf, torch.zeros_like(dyf))
    d["s1"] = dm.sum(0).contiguous()
    d["q1"] = (dm * ((zf - d["mean"]) * d["invstd"])).sum(0).contiguous()
    if kind == "mask":
        d["g"] = _nhwc(rn(N, Cin, H, H).bfloat16())
        mask = torch.randint(0, 256, (M, Cin // 8), device=dev, generator=gen, dtype=torch.uint8)
        mask[:, 0] = 0                       # all-zero and all-one bytes
        mask[:, 1] = 255
        mask[0] = 0
        mask[-1] = 255
        d["mask"] = mask.contiguous()
    elif kind == "s2":
        d["g"] = _nhwc(rn(N, Cin, (H + 1) // 2, (H + 1) // 2).bfloat16())
    return d


def _new(L, d, dtype=torch.bfloat16, **kw):
    if d["kind"] == "mask":
        kw.update(link=d["g"], lmask=d["mask"])
    elif d["kind"] == "s2":
        kw.update(link=d["g"], link_s2=True)
    return L.conv1_bn_bwd(d["dy"], d["z"], d["gamma"], d["beta"], d["mean"], d["invstd"], d["s1"],
                          d["q1"], d["x"], d["w"], dtype, **kw)


def _parent(L, d):
    """The three launches: (dz1, dx, dW1)."""
    N, H, p, Cin, M = d["N"], d["H"], d["p"], d["Cin"], d["M"]
    dz = L.bn_bwd_apply(d["dy"], d["z"], d["gamma"], d["beta"], d["mean"], d["invstd"], d["s1"],
                        d["q1"])
    wt = d["w"].t().contiguous()
    if d["kind"] == "mask":
        dx = L.conv1x1_link(dz, wt, d["g"], d["mask"])[0]
    elif d["kind"] == "s2":
        dx = L.conv1x1_link_s2(dz, wt, d["g"])
    else:
        rows = dz.permute(0, 2, 3, 1).reshape(M, p)
        dx = torch.mm(rows, d["w"]).view(N, H, H, Cin).permute(0, 3, 1, 2)
    w4 = d["w"].view(p, Cin, 1, 1)
    if p % 128 == 0:
        dw = L.wgrad1x1(dz, d["x"], torch.bfloat16)
    else:                                    # 256 -> 64: the library's weight gradient
        dw = torch.ops.aten.convolution_backward(dz, d["x"], w4, None, [1, 1], [0, 0], [1, 1],
                                                 False, [0, 0], 1, [False, True, False])[1]
    return dz, dx, dw.reshape(p, Cin)


def _oracle(d, dz):
    """fp64 (dx [M, Cin], dW1 [p, Cin]) from the bf16 dz1."""
    N, H, p, Cin, M = d["N"], d["H"], d["p"], d["Cin"], d["M"]
    z64 = dz.double().permute(0, 2, 3, 1).reshape(M, p)
    dx = z64 @ d["w"].double()
    if d["kind"] == "mask":
        sh = torch.arange(8, device=dz.device, dtype=torch.uint8)
        bits = ((d["mask"].view(M, Cin // 8, 1) >> sh) & 1).view(M, Cin).double()
        dx = dx + bits * d["g"].double().permute(0, 2, 3, 1).reshape(M, Cin)
    elif d["kind"] == "s2":
        full = torch.zeros(N, H, H, Cin, device=dz.device, dtype=torch.float64)
        full[:, ::2, ::2] = d["g"].double().permute(0, 2, 3, 1)
        dx = dx + full.view(M, Cin)
    dw = z64.t() @ d["x"].double().permute(0, 2, 3, 1).reshape(M, Cin)
    return dx, dw


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t


def _errs(got, ref):
    e = (_rows(got).double() - ref).abs()
    return float(e.max()), float(e.pow(2).mean().sqrt())


def _check_vs_parent(tag, new, par, ref):
    (nm, nr), (pm, pr) = _errs(new, ref), _errs(par, ref)
    print(f"{tag}: max |err| new {nm:.4e} parent {pm:.4e}; rms new {nr:.4e} parent {pr:.4e}")
    assert nm <= 2.0 * pm and nr <= 2.0 * pr, (tag, nm, pm, nr, pr)


def _run_case(cuda, N, H, p, Cin, kind):
    L = native.lib()
    d = _inputs(cuda, N, H, p, Cin, kind)
    dx, dw, dz = _new(L, d, want_dz=True)
    pdz, pdx, pdw = _parent(L, d)
    # 1. dz1 is bn_bwd_apply's, bit for bit
    assert torch.equal(dz.view(torch.int16), pdz.view(torch.int16))
    # 2. dx, dW1 against fp64, relative to the parent's error
    rdx, rdw = _oracle(d, pdz)
    tag = f"N{N} H{H} p{p} Cin{Cin} {kind}"
    _check_vs_parent(tag + " dx", dx, pdx, rdx)
    _check_vs_parent(tag + " dW", dw.reshape(p, Cin), pdw, rdw)
    if p % 128 == 0:   # fp32 dW1 of both paths: no bf16 rounding hides the summation
        dwf = _new(L, dict(d), dtype=torch.float32)[1]
        pdwf = L.wgrad1x1(pdz, d["x"], torch.float32)
        _check_vs_parent(tag + " dW fp32", dwf.reshape(p, Cin), pdwf.reshape(p, Cin), rdw)
    # 3. two launches are bit-identical
    dx2, dw2 = _new(L, d)
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16))
    assert torch.equal(dw.view(torch.int16), dw2.view(torch.int16))
    return d, dw, rdw


@pytest.mark.parametrize("kind", ["mask", "none"])
@pytest.mark.parametrize("p,Cin", PC)
@pytest.mark.parametrize("N,H", SHAPES)
def test_conv1_bn_bwd(cuda, N, H, p, Cin, kind):
    _run_case(cuda, N, H, p, Cin, kind)


@pytest.mark.parametrize("N,H", S2_SHAPES)
def test_conv1_bn_bwd_s2_link(cuda, N, H):
    _run_case(cuda, N, H, 128, 256, "s2")


@pytest.mark.parametrize("p,Cin", PC)
def test_more_workgroups_than_tiles(cuda, p, Cin):
    """9 pixels are one tile: of 16 pixel ranges 15 are empty and still fold as zero slabs."""
    L = native.lib()
    d = _inputs(cuda, 1, 3, p, Cin, "mask")
    dx, dw = _new(L, d)
    dx16, dw16 = _new(L, d, splits=16)
    pdz, pdx, pdw = _parent(L, d)
    rdx, rdw = _oracle(d, pdz)
    _check_vs_parent(f"p{p} Cin{Cin} 16 ranges dW", dw16.reshape(p, Cin), pdw, rdw)
    assert torch.equal(dw16.view(torch.int16), dw.view(torch.int16))
    assert torch.equal(dx16.view(torch.int16), dx.view(torch.int16))


def test_unsupported_shapes_have_no_plan(cuda):
    L = native.lib()
    assert L.conv1_bn_bwd_ok(1568, 64, 256) and L.conv1_bn_bwd_ok(9, 128, 512)
    assert not L.conv1_bn_bwd_ok(1568, 64, 64) and not L.conv1_bn_bwd_ok(1568, 256, 1024)


# --------------------------------------------------------------------------- the blocks
class _Spy:
    """The native module with the calls of a few functions kept: (args, kwargs, result)."""

    def __init__(self, real, names):
        self._real, self._names, self.calls = real, names, []

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if name not in self._names:
            return v

        def f(*a, **k):
            out = v(*a, **k)
            self.calls.append((name, a, k, out))
            return out
        return f


def _block_run(cuda, make, on):
    from resnet_trace import init_bn
    torch.manual_seed(0)
    m = init_bn(make()).to(device=cuda, dtype=torch.bfloat16, memory_format=torch.channels_last)
    m.train()
    gen = torch.Generator(device=cuda).manual_seed(1)
    x = _nhwc(torch.randn(2, 256, 28, 28, device=cuda, generator=gen).relu().bfloat16())
    x.requires_grad_(True)
    if m.down_conv is None:
        x._cml_link = fbn.ResidualLink()     # as a producing block would: the masked link
    real = native.lib()
    spy = _Spy(real, ("conv1_bn_bwd", "bn_bwd_apply"))
    pol = perf.policy().replace(fused_conv1_bwd=on, fused_conv1_bwd_min_pixels=0)
    native._C = spy
    try:
        with perf.use_policy(pol):
            y = m(x)
            gy = _nhwc(torch.randn(y.shape, device=cuda, generator=gen).to(y.dtype))
            y.backward(gy)
        torch.cuda.synchronize()
    finally:
        native._C = real
    return m, x, spy.calls


@pytest.mark.parametrize("block", ["identity", "down_s2"])
def test_bottleneck_policy_on_vs_off(cuda, block):
    from consensusml_amd.models.resnet import Bottleneck
    make = (lambda: Bottleneck(256, 64)) if block == "identity" \
        else (lambda: Bottleneck(256, 128, 2, True))
    m1, x1, c1 = _block_run(cuda, make, True)
    m0, x0, c0 = _block_run(cuda, make, False)
    fused = [c for c in c1 if c[0] == "conv1_bn_bwd"]
    assert len(fused) == 1 and not [c for c in c0 if c[0] == "conv1_bn_bwd"]
    assert len([c for c in c0 if c[0] == "bn_bwd_apply"]) == \
        len([c for c in c1 if c[0] == "bn_bwd_apply"]) + 1
    # bn1's parameter gradients do not pass through the new kernel
    for a, b in ((m1.bn1.weight, m0.bn1.weight), (m1.bn1.bias, m0.bn1.bias)):
        assert torch.equal(a.grad.view(torch.int16), b.grad.view(torch.int16))
    # the parent path and the oracle on the very operands the fused call received
    _, a, k, (dx, dw) = fused[0]
    L = native.lib()
    d = {"N": 2, "H": 28, "p": a[1].shape[1], "Cin": 256, "M": 2 * 28 * 28,
         "dy": a[0], "z": a[1], "gamma": a[2], "beta": a[3], "mean": a[4], "invstd": a[5],
         "s1": a[6], "q1": a[7], "x": a[8].detach(), "w": a[9].detach(),
         "kind": "s2" if k.get("link_s2") else "mask" if "lmask" in k else "none"}
    assert d["kind"] == ("mask" if block == "identity" else "s2")
    d["g"], d["mask"] = k.get("link"), k.get("lmask")
    pdz, pdx, pdw = _parent(L, d)
    rdx, rdw = _oracle(d, pdz)
    assert torch.equal(x1.grad.view(torch.int16), dx.view(torch.int16))   # nothing added after
    _check_vs_parent(block + " x.grad", x1.grad, pdx, rdx)
    _check_vs_parent(block + " conv1.weight.grad", m1.conv1.weight.grad.reshape(-1, 256), pdw, rdw)
    _check_vs_parent(block + " x.grad (policy off run)", x1.grad, x0.grad, rdx)
    _check_vs_parent(block + " conv1.weight.grad (policy off run)",
                     m1.conv1.weight.grad.reshape(-1, 256),
                     m0.conv1.weight.grad.reshape(-1, 256), rdw)
