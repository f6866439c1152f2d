"""An independent LARS oracle for the LARS tests: one parameter tensor at a time, plain fp64 torch
ops, nothing of ``ops.reference``'s LARS functions. The definition (``OptimConfig``): norms over
the tensor's own elements; q = 0 where a norm is not finite (a zero gradient), q = trust * wn /
(gn + wd * wn + eps) rounded to fp32 for an adapted tensor with both norms positive, else 1;
g <- q * (g + wd * p); then torch.optim.SGD's momentum / Nesterov step."""
import math

import pytest
import torch


def lars_tensor_step(p, g, buf, *, lr, momentum=0.0, wd=0.0, nesterov=False, first=False,
                     trust=0.001, eps=0.0, adapted=True):
    """One LARS step of one tensor in fp64. ``g``: the gradient as the optimizer sees it (already
    scaled). Returns (new p, new buf or None, q, wn, gn)."""
    p64 = p.detach().double().reshape(-1)
    g64 = g.detach().double().reshape(-1)
    sw = float((p64 * p64).sum())
    sg = float((g64 * g64).sum())
    if not (math.isfinite(sw) and math.isfinite(sg)):
        q = 0.0
        wn = math.sqrt(sw) if math.isfinite(sw) else sw
        gn = math.sqrt(sg) if math.isfinite(sg) else sg
        d = torch.zeros_like(p64)
    else:
        wn, gn = math.sqrt(sw), math.sqrt(sg)
        q = 1.0
        if adapted and wn > 0 and gn > 0:
            q = float(torch.tensor(trust * wn / (gn + wd * wn + eps), dtype=torch.float64).float())
        d = q * (g64 + wd * p64)
    b64 = None
    if momentum:
        b64 = d.clone() if first else momentum * buf.detach().double().reshape(-1) + d
        d = d + momentum * b64 if nesterov else b64
    return p64 - lr * d, b64, q, wn, gn


def lars_vector_step(master, g, buf, ranges, adapted, **kw):
    """``lars_tensor_step`` over the tensors ``ranges`` = [(start, numel)] of a state vector.
    Returns fp64 copies (master, buf) with only the tensors' elements changed, and the per-tensor
    (q, wn, gn) rows."""
    m = master.detach().double().clone().reshape(-1)
    b = buf.detach().double().clone().reshape(-1) if buf is not None else None
    rows = []
    for (s, n), ad in zip(ranges, adapted):
        p1, b1, q, wn, gn = lars_tensor_step(
            master[s:s + n], g[s:s + n], buf[s:s + n] if buf is not None else None,
            adapted=bool(ad), **kw)
        m[s:s + n] = p1
        if b1 is not None:
            b[s:s + n] = b1
        rows.append((q, wn, gn))
    return m, b, rows


def engine_aggregate(e):
    """The fp32 aggregate, in state-vector coordinates, that the engine's last LARS step used."""
    if e.gout is not None:
        return e.gout.detach().clone()
    scale = 1.0 / e.n if e.topo == "allreduce" else 1.0
    return e.flat.flat_grad[0].detach().float() * torch.tensor(scale, dtype=torch.float32)


def check_engine_against_oracle(tr, steps, rtol, atol):
    """``steps`` training steps of an ``optim.name=lars`` trainer against the oracle loop, which
    keeps its own fp64 state and is fed the aggregate the engine used in each step. One rank:
    the state vector is the flat vector."""
    e, o = tr.engine, tr.engine.cfg.optim
    fl = e.flat
    ranges = [(fl.param_offset[i], p.numel()) for i, p in enumerate(fl.params)]
    adapt = [not (o.lars_exclude_1d and p.dim() < 2) for p in fl.params]
    assert any(adapt) and not all(adapt)
    m = e.master.detach().double().clone()
    b = torch.zeros_like(m) if o.momentum else None
    for step in range(steps):
        tr.train_step()
        m, b, rows = lars_vector_step(
            m, engine_aggregate(e).double(), b, ranges, adapt, lr=o.lr, momentum=o.momentum,
            wd=o.weight_decay, nesterov=o.nesterov, first=step == 0, trust=o.trust_coef,
            eps=o.eps)
        st = e.lars_stats.cpu()
        assert st.shape == (len(fl.params), 4)
        for t, (q, wn, gn) in enumerate(rows):
            assert float(st[t, 2]) == pytest.approx(q, rel=1e-5)
            assert float(st[t, 0]) == pytest.approx(wn, rel=1e-5)
            assert float(st[t, 3]) == 0.0
            assert (q == 1.0) == (not adapt[t])
    got = e.master.detach().cpu().double()
    for s, n in ranges:
        torch.testing.assert_close(got[s:s + n], m[s:s + n].cpu(), rtol=rtol, atol=atol)
    for p, (s, n) in zip(fl.params, ranges):     # the parameters are the master, rounded
        assert torch.equal(p.detach().cpu().reshape(-1), e.master[s:s + n].cpu().to(p.dtype))
