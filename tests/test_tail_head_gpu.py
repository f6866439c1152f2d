"""A layer-1 recompute tail with the next block's conv1 inside (``csrc/kernels/tail_head.hip``,
``lib().conv1x1_bnres_head`` / ``conv1x1_cat_bnres_head``) against the two launches it replaces
(``conv1x1_bnres`` / ``conv1x1_cat_bnres``, then ``conv1x1_bn_fwd`` on y) and fp64 oracles.

y and its mask use the parent kernels' operand roles, k order and rounding points; whether they
come out bit for bit is printed, and required is the rule of ``test_conv1_bwd_gpu.py``: against an
fp64 oracle the new path's maximum and rms error may be at most 2x the parent's (summation order
moves an error by about its own size), and the mask is (y > 0) of the stored y exactly. z1n is
judged the same way against an fp64 product of the stored bf16 y. The statistics are those of the
stored bf16 z1n, to the tolerances of ``test_conv1x1_bn_gpu.py``."""
import copy

import pytest
import torch

from consensusml_amd import perf
from consensusml_amd.ops import conv as fconv
from consensusml_amd.ops import native

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (3, 9), (2, 28)]          # (N, H = W): 9 / 243 / 1568 pixels
P, CO = 64, 256
EPS, MOM = 1e-5, 0.1


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t


def _inputs(dev, N, H, kind, p2, zero3, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed + 1000 * N + 10 * H + p2)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    M = N * H * H
    d = {"N": N, "H": H, "M": M, "kind": kind, "p2": p2}
    d["z"] = _nhwc((rn(N, P, H, H) * 1.5 + 0.3).bfloat16())
    gamma = torch.empty(P, device=dev).uniform_(0.5, 1.5, generator=gen)
    gamma[1::7] *= -1.0                      # bn2's scale negative and exactly zero in places
    gamma[3::11] = 0.0
    beta = torch.empty(P, device=dev).uniform_(-0.3, 0.3, generator=gen)
    zf = _rows(d["z"]).float()
    mean, invstd = zf.mean(0), (zf.var(0, unbiased=False) + EPS).rsqrt()
    d["sc"] = (gamma.bfloat16().float() * invstd).contiguous()
    d["bi"] = (beta.bfloat16().float() - mean * d["sc"]).contiguous()
    # bn3: scale all zero (the initial state, nn.init.zeros_(bn3.weight)) or a real one
    sc3 = torch.zeros(CO, device=dev) if zero3 else \
        torch.empty(CO, device=dev).uniform_(0.5, 1.5, generator=gen)
    bi3 = torch.empty(CO, device=dev).uniform_(-0.3, 0.3, generator=gen)
    w3 = (rn(CO, P) * P ** -0.5).bfloat16()
    if kind == "identity":
        d["w"], d["sc3"], d["bi3"] = w3.view(CO, P, 1, 1), sc3, bi3
        d["res"] = _nhwc(rn(N, CO, H, H).relu().bfloat16())
    else:   # the scales are folded into w_cat's halves; x is a ReLU output, staged as is
        scd = torch.empty(CO, device=dev).uniform_(0.5, 1.5, generator=gen)
        wd = (rn(CO, P) * P ** -0.5).bfloat16()
        d["w"] = fconv.scaled_cat(w3, sc3, wd, scd).contiguous()
        d["sc3"], d["bi3"] = torch.ones(CO, device=dev), bi3
        d["x"] = _nhwc(rn(N, P, H, H).relu().bfloat16())
    d["w1n"] = (rn(p2, CO) * CO ** -0.5).bfloat16().view(p2, CO, 1, 1)
    d["rm0"] = (rn(p2) * 0.1).contiguous()
    return d


def _new(L, d, **kw):
    rm, rv = d["rm0"].clone(), torch.ones(d["p2"], device=d["z"].device)
    if d["kind"] == "identity":
        out = L.conv1x1_bnres_head(d["z"], d["w"], d["sc"], d["bi"], d["sc3"], d["bi3"], d["res"],
                                   d["w1n"], rm, rv, EPS, MOM, **kw)
    else:
        out = L.conv1x1_cat_bnres_head(d["z"], d["x"], d["sc"], d["bi"], d["w"], d["sc3"],
                                       d["bi3"], d["w1n"], rm, rv, EPS, MOM, **kw)
    return tuple(out[:5]) + (rm, rv)


def _parent(L, d):
    """The two launches: (y, mask, z1n, mean, invstd, rmean, rvar)."""
    if d["kind"] == "identity":
        y, mask = L.conv1x1_bnres(d["z"], d["w"], d["sc"], d["bi"], d["sc3"], d["bi3"], d["res"])
    else:
        y, mask = L.conv1x1_cat_bnres(d["z"], d["x"], d["sc"], d["bi"], None, None, d["w"],
                                      d["sc3"], d["bi3"])
    rm, rv = d["rm0"].clone(), torch.ones(d["p2"], device=y.device)
    z1n, mean, invstd = L.conv1x1_bn_fwd(y, d["w1n"], None, None, rm, rm, rv, 1, True, EPS, MOM)
    return y, mask, z1n, mean, invstd, rm, rv


def _oracle_y(d):
    """fp64 y [M, 256] from the bf16 staged operand."""
    a = torch.relu(_rows(d["z"]).float() * d["sc"] + d["bi"]).bfloat16().double()
    if d["kind"] == "identity":
        acc = a @ d["w"].view(CO, P).double().t()
        v = acc * d["sc3"].double() + d["bi3"].double() + _rows(d["res"]).double()
    else:
        acc = torch.cat([a, _rows(d["x"]).double()], 1) @ d["w"].double().t()
        v = acc + d["bi3"].double()
    return torch.relu(v)


def _errs(got, ref):
    e = (_rows(got).double() - ref).abs()
    return float(e.max()), float(e.pow(2).mean().sqrt())


def _check_vs_parent(tag, new, par, ref):
    (nm, nr), (pm, pr) = _errs(new, ref), _errs(par, ref)
    print(f"{tag}: max |err| new {nm:.4e} parent {pm:.4e}; rms new {nr:.4e} parent {pr:.4e}")
    assert nm <= 2.0 * pm and nr <= 2.0 * pr, (tag, nm, pm, nr, pr)


def _bits(mask, C):
    sh = torch.arange(8, device=mask.device, dtype=torch.uint8)
    return ((mask.view(mask.shape[0], C // 8, 1) >> sh) & 1).view(mask.shape[0], C).bool()


def _check_stats(tag, d, z1n, mean, invstd, rm, rv):
    """Against fp64 statistics of the stored bf16 z1n (tolerances of test_conv1x1_bn_gpu.py)."""
    M = d["M"]
    z64 = _rows(z1n).double()
    m, v = z64.mean(0), z64.var(0, unbiased=False)
    print(f"{tag}: max |mean err| {float((mean.double() - m).abs().max()):.3e}, max rel invstd err "
          f"{float((invstd.double() * (v + EPS).sqrt() - 1).abs().max()):.3e}")
    torch.testing.assert_close(mean.double(), m, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(invstd.double(), (v + EPS).rsqrt(), rtol=2e-3, atol=1e-4)
    torch.testing.assert_close(rm.double(), (1 - MOM) * d["rm0"].double() + MOM * m, rtol=1e-4,
                               atol=1e-5)
    unb = v * M / (M - 1) if M > 1 else v
    torch.testing.assert_close(rv.double(), (1 - MOM) * 1.0 + MOM * unb, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("zero3", [True, False])
@pytest.mark.parametrize("p2", [64, 128])
@pytest.mark.parametrize("kind", ["identity", "down"])
@pytest.mark.parametrize("N,H", SHAPES)
def test_tail_head(cuda, N, H, kind, p2, zero3):
    L = native.lib()
    d = _inputs(cuda, N, H, kind, p2, zero3)
    y, mask, z1n, mean, invstd, rm, rv = _new(L, d)
    py, pmask, pz1n, pmean, pinvstd, prm, prv = _parent(L, d)
    tag = f"N{N} H{H} {kind} p'{p2} zero3={zero3}"
    # 1. y and its mask
    same = torch.equal(y.view(torch.int16), py.view(torch.int16)) and torch.equal(mask, pmask)
    print(f"{tag}: y and mask bit-identical to the parent kernel: {same}")
    _check_vs_parent(tag + " y", y, py, _oracle_y(d))
    assert torch.equal(_bits(mask, CO), _rows(y) > 0)
    # 2. z1n against an fp64 product of each path's own stored y
    w1 = d["w1n"].view(p2, CO).double()
    (nm, nr), (pm, pr) = _errs(z1n, _rows(y).double() @ w1.t()), \
        _errs(pz1n, _rows(py).double() @ w1.t())
    print(f"{tag} z1n: max |err| new {nm:.4e} parent {pm:.4e}; rms new {nr:.4e} parent {pr:.4e}")
    assert nm <= 2.0 * pm and nr <= 2.0 * pr, (tag, nm, pm, nr, pr)
    # 3. statistics of the stored z1n, parent and new against the same oracle
    _check_stats(tag + " new", d, z1n, mean, invstd, rm, rv)
    _check_stats(tag + " parent", d, pz1n, pmean, pinvstd, prm, prv)
    # 4. two launches are bit-identical
    again = _new(L, d)
    for a, b in zip((y, mask, z1n, mean, invstd, rm, rv), again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind,p2", [("identity", 64), ("identity", 128), ("down", 64)])
@pytest.mark.parametrize("N,H,wgs", [(1, 3, 16), (3, 9, 7)])
def test_more_workgroups_than_tiles(cuda, kind, p2, N, H, wgs):
    """Pixel ranges without tiles write zero partial rows: the results do not change (9 pixels
    are one tile of 16 ranges; 243 are four tiles of 7 ranges, one tile each)."""
    L = native.lib()
    d = _inputs(cuda, N, H, kind, p2, False)
    ref, out = _new(L, d), _new(L, d, wgs=wgs)
    for k, (a, b) in enumerate(zip(ref[:3], out[:3])):
        assert torch.equal(a, b), k
    _check_stats(f"{kind} p'{p2} {wgs} ranges", d, *out[2:])
    if N == 1:   # one tile either way: the same sums in the same order
        for a, b in zip(ref[3:], out[3:]):
            assert torch.equal(a, b)


def test_unsupported_shapes_have_no_plan(cuda):
    L = native.lib()
    assert L.tail_head_ok(1568, 64, 256, 64) and L.tail_head_ok(9, 64, 256, 128)
    assert not L.tail_head_ok(1568, 128, 512, 128) and not L.tail_head_ok(1568, 64, 256, 256)
    assert not L.tail_head_ok(0, 64, 256, 64)


# --------------------------------------------------------------------------- the blocks
HEAD_FNS = ("conv1x1_bnres_head", "conv1x1_cat_bnres_head")
SPIED = HEAD_FNS + ("conv1x1_bn_fwd", "conv1x1_bnres", "conv1x1_cat_bnres")


class _Spy:
    """The native module with the calls of a few functions kept: (name, args, kwargs, result)."""

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


def _make(pair):
    from resnet_trace import init_bn
    from consensusml_amd.models.resnet import Bottleneck
    torch.manual_seed(0)
    first = Bottleneck(64, 64, 1, True) if pair == "down" else Bottleneck(256, 64)
    nxt = Bottleneck(256, 64) if pair != "to_layer2" else Bottleneck(256, 128, 2, True)
    m = init_bn(torch.nn.Sequential(first, nxt))
    with torch.no_grad():   # running means off zero, so that a second update would show
        for b in m:
            b.bn1.running_mean.uniform_(-0.2, 0.2)
    return m


def _run(cuda, m, on, dt=torch.bfloat16, pre=None):
    """One forward + backward of the two blocks under ``tail_heads`` -> (y, x.grad, calls)."""
    from consensusml_amd.models.resnet import tail_heads
    m = m.to(device=cuda, dtype=dt, memory_format=torch.channels_last).train()
    gen = torch.Generator(device=cuda).manual_seed(1)
    cin = m[0].conv1.in_channels
    x = _nhwc(torch.randn(2, cin, 28, 28, device=cuda, generator=gen).relu().to(dt))
    x.requires_grad_(True)
    real = native.lib()
    spy = _Spy(real, SPIED)
    pol = perf.policy().replace(fused_tail_head=on, fused_tail_head_min_pixels=0)
    native._C = spy
    try:
        with perf.use_policy(pol), tail_heads(m, list(m)):
            keys = (list(m.state_dict().keys()), [id(p) for p in m.parameters()])
            y = m[0](x)
            if pre is not None:
                pre(y)
            y = m[1](y)
            gy = _nhwc(torch.randn(y.shape, device=cuda, generator=gen).to(dt))
            y.backward(gy)
        torch.cuda.synchronize()
    finally:
        native._C = real
    return y.detach(), x.grad, spy.calls, keys


def _err(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12))


@pytest.mark.parametrize("pair", ["identity", "down", "to_layer2"])
def test_blocks_policy_on_vs_off(cuda, pair):
    """Two consecutive blocks (identity -> identity, down -> identity, identity -> the next
    stage's first block): policy on and off against an fp32 copy, to the tolerances
    ``test_bwd_fusion_gpu.py`` uses for such pairs."""
    m_on = _make(pair)
    m_off, m32 = copy.deepcopy(m_on), copy.deepcopy(m_on)
    keys0 = (list(m_on.state_dict().keys()), None)
    m_on = m_on.to(device=cuda, dtype=torch.bfloat16, memory_format=torch.channels_last)
    rm0 = m_on[1].bn1.running_mean.clone()   # as the forward will find it
    y1, g1, c1, k1 = _run(cuda, m_on, True)
    y0, g0, c0, k0 = _run(cuda, m_off, False)
    yr, gr, _, _ = _run(cuda, m32, False, torch.float32)
    # the kernels by name and count
    heads = [c for c in c1 if c[0] in HEAD_FNS]
    assert len(heads) == 1 and not [c for c in c0 if c[0] in HEAD_FNS]
    assert heads[0][0] == ("conv1x1_cat_bnres_head" if pair == "down" else "conv1x1_bnres_head")
    n = lambda cs, name: len([c for c in cs if c[0] == name])
    assert n(c0, "conv1x1_bn_fwd") == n(c1, "conv1x1_bn_fwd") + 1
    assert n(c0, "conv1x1_bnres") + n(c0, "conv1x1_cat_bnres") == \
        n(c1, "conv1x1_bnres") + n(c1, "conv1x1_cat_bnres") + 1
    # the successor is no submodule: the same keys and parameter order, set or not
    assert k1[0] == k0[0] == keys0[0] == list(m_on.state_dict().keys())
    assert k1[1] == [id(p) for p in m_on.parameters()]
    assert "_cml_next" not in m_on[0].__dict__
    # outputs and gradients
    for tag, a, b, r in (("y", y1, y0, yr), ("x.grad", g1, g0, gr)):
        e_on, e_off = _err(a, r), _err(b, r)
        print(f"{pair} {tag}: rel err on {e_on:.3e} off {e_off:.3e}")
        assert e_on <= 1.5 * e_off + 1e-2, (tag, e_on, e_off)
    for (name, a), b, r in zip(m_on.named_parameters(), m_off.parameters(), m32.parameters()):
        e_on, e_off = _err(a.grad, r.grad), _err(b.grad, r.grad)
        assert e_on <= 1.5 * e_off + 2e-2, (name, e_on, e_off)
    for a, b in zip(m_on.buffers(), m_off.buffers()):   # running statistics
        torch.testing.assert_close(a.float(), b.float(), rtol=1e-3, atol=1e-3)
    # bn1's running statistics advanced once, by the head's own mean
    mean = heads[0][3][3]
    torch.testing.assert_close(m_on[1].bn1.running_mean.float(),
                               (1 - MOM) * rm0.float() + MOM * mean, rtol=1e-4, atol=1e-5)


class _Pending:
    def query(self, params):
        return True


def test_pending_parameters_take_the_parent_path(cuda):
    m = _make("identity")
    stub = _Pending()
    fconv.set_pending_query(m, stub.query)
    try:
        _, _, calls, _ = _run(cuda, m, True)
    finally:
        fconv.set_pending_query(m, None)
    _, _, c_off, _ = _run(cuda, _make("identity"), False)
    assert not [c for c in calls if c[0] in HEAD_FNS]
    assert [c[0] for c in calls] == [c[0] for c in c_off]


@pytest.mark.parametrize("how", ["foreign", "stale"])
def test_stale_or_foreign_head_is_ignored(cuda, how):
    """A block input that carries a conv1 result made for another tensor, or for a weight that
    has changed since, runs its own conv1."""
    m_ref, m = _make("identity"), _make("identity")
    y0, g0, c0, _ = _run(cuda, m_ref, False)

    def plant(y):
        w = m[1].conv1.weight
        junk = torch.zeros(2, 64, 28, 28, device=cuda, dtype=torch.bfloat16)
        st = torch.zeros(64, device=cuda)
        other = y if how == "stale" else torch.empty_like(y)
        y._cml_head = fconv.HeadResult(other, w, w._version - (1 if how == "stale" else 0),
                                       _nhwc(junk), st, st + 1)

    y1, g1, c1, _ = _run(cuda, m, False, pre=plant)
    assert len([c for c in c1 if c[0] == "conv1x1_bn_fwd"]) == \
        len([c for c in c0 if c[0] == "conv1x1_bn_fwd"])
    assert torch.equal(y1, y0) and torch.equal(g1, g0)
