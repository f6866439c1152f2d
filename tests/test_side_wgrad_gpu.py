"""PerfPolicy.side_wgrad: the 3x3 weight gradients of the BN-fused 3x3 convs run on a second HIP
stream, concurrent with the same conv's data-gradient and BN-backward kernels. The kernels are the
same (all deterministic, fixed-order folds), so the backward must be bit-identical to the
single-stream one, also when the side stream's blocks are reused by the allocator on the next
call; the current stream waits for the side stream before the backward returns."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


# (the 128-channel stride-2 weight gradient runs on MIOpen, whose weight-gradient kernels are not
# bitwise reproducible run to run: not a case here)
@pytest.mark.parametrize("N,C,H,stride", [(16, 64, 56, 1), (16, 128, 28, 1), (8, 256, 14, 1),
                                          (8, 256, 28, 2), (8, 512, 14, 2)])
def test_side_wgrad_bit_identical(cuda, N, C, H, stride):
    from consensusml_amd import perf
    from consensusml_amd.ops import conv as fconv
    fn = fconv._BNReLUConv3x3BNStatsFn
    g0 = torch.Generator(device=cuda).manual_seed(C + H)
    z1 = _nhwc(torch.randn(N, C, H, H, device=cuda, generator=g0).bfloat16())
    g1 = (torch.rand(C, device=cuda, generator=g0) + 0.5).bfloat16()
    b1 = (torch.randn(C, device=cuda, generator=g0) * 0.1).bfloat16()
    zf = z1.float()
    mean1 = zf.mean((0, 2, 3))
    invstd1 = (zf.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()
    w = (torch.randn(C, C, 3, 3, device=cuda, generator=g0) * (9 * C) ** -0.5).bfloat16()
    Ho = H // stride
    gz = _nhwc(torch.randn(N, C, Ho, Ho, device=cuda, generator=g0).bfloat16())
    out = {}
    for side in (False, True, False):
        with perf.use_policy(perf.policy().replace(side_wgrad=side, side_wgrad_min_batch=0)):
            res = []
            for _ in range(2):   # the second call reuses the side stream's freed blocks
                zi, gi, bi, wi = (t.clone().requires_grad_(True) for t in (z1, g1, b1, w))
                rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
                z2, _, _ = fn.apply(zi, gi, bi, mean1, invstd1, 1e-5, wi, rm, rv, 1e-5, 0.1,
                                    stride)
                z2.backward(gz)
                res.append([t.grad.clone() for t in (zi, gi, bi, wi)] + [z2.detach().clone()])
        torch.cuda.synchronize()
        out.setdefault(side, []).append(res)
    ref = out[False][0][0]
    for runs in (out[False], out[True]):
        for res in runs:
            for call in res:
                for a, b in zip(call, ref):
                    assert torch.equal(a, b)



def test_side_wgrad_1x1_model_bit_identical(cuda):
    """The 1x1 convs' weight gradients on the side stream too (side_wgrad_1x1): a ResNet-50
    training backward at 64 x 64 gives the same 1x1 weight gradients with the side stream on and
    off (loosely: MIOpen may pick another algorithm between runs, tools/diag/det_diag.py, so the
    check is for ordering errors -- a missing join reads a half-written gradient)."""
    import copy

    import consensusml_amd.models.resnet as R
    from consensusml_amd import perf
    torch.manual_seed(2)
    base = R.resnet50(num_classes=10).to(cuda).to(memory_format=torch.channels_last).bfloat16()
    x = _nhwc(torch.randn(8, 3, 64, 64, device=cuda).bfloat16())
    out = {}
    for side in (False, True):
        m = copy.deepcopy(base)
        with perf.use_policy(perf.policy().replace(side_wgrad=side, side_wgrad_min_batch=0,
                                                   side_wgrad_1x1=True)):
            m(x).float().square().mean().backward()
        torch.cuda.synchronize()
        out[side] = {n: p.grad.clone() for n, p in m.named_parameters()
                     if p.dim() == 4 and p.shape[2] == 1}
    for n, g in out[False].items():
        rel = ((out[True][n].float() - g.float()).norm() / g.float().norm().clamp_min(1e-12)).item()
        assert rel < 2e-2, (n, rel)
