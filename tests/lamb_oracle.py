"""An independent LAMB oracle for the LAMB tests (one parameter tensor at a time, plain fp64 torch
ops from the fp32 inputs, nothing of ``ops.reference``; the definition is ``OptimConfig``'s), the
one layout the kernel tests use, and the loop that drives ``ops.kernels``' three stages over it on
a device (the HIP kernels) or on the CPU (the torch reference path)."""
import math

import pytest
import torch

SIZES = [1, 7, 8, 9, 0, 2055, 4099]     # with chunk 1024: 1, 3 and 5 items, ragged tails, one empty
STARTS = [0, 8, 16, 24, 40, 40, 2096]   # padded to multiples of 8
RANGES = list(zip(STARTS, SIZES))
END, TOTAL = 6195, 6200                 # END is no multiple of 8: the segment's ragged tail
CUT = STARTS[5] + 1024                  # a multiple of 8 inside the 2055 tensor
ADAPT = [0, 1, 1, 1, 1, 1, 1]
HYPER = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-6)
RTOL_NORM = 1e-9             # tests/test_lars_gpu.py: fp64 sums of exact squares
RTOL, ATOL = 2e-5, 2e-6      # ... and its pair for a fused fp32 update against a reference
RTOL_U = 1e-5                # sum u^2 and q: <= six fp32 roundings per u (< 4e-7) and no
                             # cancellation, which check_step asserts of the oracle's own un
# output segments (state offset, length), parameter dtype, grid_cap
VARIANTS = {"one-bf16": ([(0, END)], torch.bfloat16, 0),
            "two-fp32": ([(0, CUT), (CUT, END - CUT)], torch.float32, 0),
            "cap1-bf16": ([(0, CUT), (CUT, END - CUT)], torch.bfloat16, 1)}


def inputs(gdtype, steps=3):
    """p ~ N(0, 1) and ``steps`` gradient rows ~ N(0, 1) over the layout; the alignment padding
    holds NaN (master) and inf (gradient): it must never reach a norm."""
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(TOTAL, generator=gen)
    gs = [torch.randn(TOTAL, generator=gen).to(gdtype) for _ in range(steps)]
    for (s, n), e in zip(RANGES, STARTS[1:] + [TOTAL]):
        for t, pad in [(p, float("nan"))] + [(g, float("inf")) for g in gs]:
            t[s + n:e] = pad
    return p, gs


def tensor_step(p, g, m, v, *, k, scale, wd, adapted, lr, b1, b2, eps):
    """One LAMB step of one tensor in fp64 from the fp32 inputs of the kernels: the fp32 / bf16
    rows, x the fp32-rounded product, and the scalars as the kernels receive them (fp32; the bias
    corrections formed in double from the given betas, then rounded: 1 - fp32(0.999) is 1.3e-5
    from 1 - 0.999, a property of the inputs, not an error of the arithmetic under test).
    Returns (p', m', v', q, wn, un); a non-finite norm returns the state unchanged and q = 0."""
    f32 = lambda c: float(torch.tensor(c, dtype=torch.float32))
    x = (g.float() * torch.tensor(scale, dtype=torch.float32)).double()
    p, m, v = p.double(), m.double(), v.double()
    inv_bc1, inv_sqrt_bc2 = f32(1 / (1 - b1 ** k)), f32(1 / math.sqrt(1 - b2 ** k))
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    m1 = b1 * m + (1 - b1) * x
    v1 = b2 * v + (1 - b2) * x * x
    u = wd * p + (m1 / (v1.sqrt() * inv_sqrt_bc2 + eps)) * inv_bc1
    sw, su = float((p * p).sum()), float((u * u).sum())
    if not (math.isfinite(sw) and math.isfinite(su)):
        return p, m, v, 0.0, sw, su
    wn, un = math.sqrt(sw), math.sqrt(su)
    q = float(torch.tensor(wn / un).float()) if adapted and wn > 0 and un > 0 else 1.0
    return p - lr * q * u, m1, v1, q, wn, un


def vector_step(p, g, m, v, ranges, adapt, **kw):
    """``tensor_step`` over the tensors ``ranges`` = [(start, numel)] of fp64 state vectors (new
    copies; only the tensors' elements change) and the per-tensor (q, wn, un) rows."""
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    rows = []
    for (s, n), ad in zip(ranges, adapt):
        sl = slice(s, s + n)
        p[sl], m[sl], v[sl], *row = tensor_step(p[sl], g[sl], m[sl], v[sl], adapted=bool(ad), **kw)
        rows.append(row)
    return p, m, v, rows


def engine_cfg(topo, V, eps):
    """``optim.name=lamb`` on the tiny MLP in fp32, mean over V virtual workers."""
    from consensusml_amd import TrainConfig
    cfg = TrainConfig()
    cfg.dtype, cfg.virtual_workers, cfg.batch_per_worker = "fp32", V, 16
    cfg.topology.kind, cfg.topology.bucket_mb = topo, 0.0004      # several buckets
    cfg.optim.name, cfg.optim.lr, cfg.optim.weight_decay, cfg.optim.eps = "lamb", 0.01, 0.01, eps
    cfg.model.extra = {"classes": 2}
    return cfg


def device_steps(dev, p0, gs, scale, wd, variant, adapt=ADAPT):
    """The three stages for every gradient row from zero moments; per step the CPU copies
    (pairs, q, stats, p, m, v, [parameter outputs], (p, m, v) before the step)."""
    from consensusml_amd.ops import kernels as K
    segs, pdtype, cap = VARIANTS[variant]
    plan = K.lars_plan(STARTS, SIZES, chunk=1024, total=TOTAL)
    assert plan.item_off.tolist() == [0, 1, 2, 3, 4, 4, 7, 12]
    p = p0.to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ad = torch.tensor(adapt, dtype=torch.uint8, device=dev)
    q = torch.full((plan.T,), -1.0, device=dev)
    stats = torch.zeros(plan.T, K.LARS_STATS, dtype=torch.float64, device=dev)
    out = []
    for k, g in enumerate(gs, 1):
        gd = g.to(dev)
        o = K.OptArgs(kind="lamb", lr=HYPER["lr"], weight_decay=wd, beta1=HYPER["b1"],
                      beta2=HYPER["b2"], eps=HYPER["eps"], step=k, first=k == 1)
        before = tuple(t.cpu().clone() for t in (p, m, v))
        plan.on(dev)[3].fill_(float("nan"))             # every slot that is read is written
        pairs = K.lamb_norms(p, gd, scale, plan, o, m, v, grid_cap=cap)
        K.lars_ratio(pairs, ad, 1.0, 0.0, 0.0, q, stats)
        pouts = [torch.zeros(n, dtype=pdtype, device=dev) for _, n in segs]
        K.lamb_update(gd, scale, plan, q, o, p, m, v,
                      segs=[(po, s, n) for po, (s, n) in zip(pouts, segs)], grid_cap=cap)
        out.append([t.cpu().clone() for t in (pairs, q, stats, p, m, v)]
                   + [[po.cpu() for po in pouts], before])
    return out


def check_step(got, g, k, scale, wd, adapt=ADAPT, skip=()):
    """Step ``k``'s results against the oracle's step from the fp32 state the kernels read,
    tensor by tensor; the tensors ``skip`` are the caller's."""
    pairs, q, stats, p, m, v, _, before = got
    want = vector_step(before[0], g, *before[1:], RANGES, adapt, k=k, scale=scale, wd=wd, **HYPER)
    for t, ((s, n), (wq, wn, un)) in enumerate(zip(RANGES, want[3])):
        if t in skip:
            continue
        print(f"step {k} tensor {t}: sum p^2 {float(pairs[t, 0]):.12g} ({wn * wn:.12g}) sum u^2 "
              f"{float(pairs[t, 1]):.9g} ({un * un:.9g}) q {float(q[t]):.8g} ({wq:.8g})")
        assert n == 0 or un > 0.1 * n ** 0.5            # the oracle's norm is no cancellation
        assert float(pairs[t, 0]) == pytest.approx(wn * wn, rel=RTOL_NORM)
        assert float(pairs[t, 1]) == pytest.approx(un * un, rel=RTOL_U)
        assert float(q[t]) == pytest.approx(wq, rel=RTOL_U)
        assert float(stats[t, 2]) == float(q[t]) and float(stats[t, 3]) == 0.0
        for a, b in zip((p, m, v), want[:3]):
            torch.testing.assert_close(a[s:s + n].double(), b[s:s + n], rtol=RTOL, atol=ATOL)
