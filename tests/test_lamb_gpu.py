"""LAMB on the MI355X (csrc/kernels/lamb.hip): ``lamb_norms``, the ratios and ``lamb_update``
against the independent fp64 oracle of tests/lamb_oracle.py over three steps from zero state,
bit-reproducibility, a NaN in the aggregate, the all-excluded step against the AdamW kernel, and
the engine and ``FusedLAMB`` on the device."""
import copy

import pytest
import torch

import lamb_oracle as LO

pytestmark = pytest.mark.gpu

RTOL, ATOL, RANGES, VARIANTS = LO.RTOL, LO.ATOL, LO.RANGES, LO.VARIANTS


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_kernels_against_oracle_and_twice(cuda, gdtype, scale, wd, variant):
    p0, gs = LO.inputs(gdtype)
    got = LO.device_steps(cuda, p0, gs, scale, wd, variant)
    segs, pdtype, _ = VARIANTS[variant]
    for k, (step, g) in enumerate(zip(got, gs), 1):
        LO.check_step(step, g, k, scale, wd)
        assert float(step[1][0]) == 1.0 and float(step[1][4]) == 1.0   # not adapted / empty
        for po, (s, n) in zip(step[6], segs):           # the parameters are the master, rounded
            assert torch.equal(po.float().nan_to_num(7.0),
                               step[3][s:s + n].to(pdtype).float().nan_to_num(7.0))
    again = LO.device_steps(cuda, p0, gs, scale, wd, variant)     # the same data, the same bits
    for a, b in zip(got, again):
        for x, y in zip(a[:2] + a[3:6], b[:2] + b[3:6]):
            assert torch.equal(x.nan_to_num(7.0), y.nan_to_num(7.0))


@pytest.mark.parametrize("variant", ["one-bf16", "two-fp32"])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_nan_in_the_aggregate_skips_exactly_one_tensor(cuda, gdtype, variant):
    """One NaN in the 2055 tensor's gradient on the second step: that tensor keeps p, m and v bit
    for bit, its parameters are the old master rounded, everything else follows the oracle."""
    p0, gs = LO.inputs(gdtype, steps=2)
    s5, n5 = RANGES[5]
    gs[1][s5 + 1500] = float("nan")
    got = LO.device_steps(cuda, p0, gs, 0.37, 0.01, variant)
    LO.check_step(got[0], gs[0], 1, 0.37, 0.01)
    LO.check_step(got[1], gs[1], 2, 0.37, 0.01, skip=(5,))
    pairs, q, stats, p, m, v, pouts, _ = got[1]
    assert int((q == 0).sum()) == 1 and float(q[5]) == 0.0
    assert stats[:, 3].tolist() == [0, 0, 0, 0, 0, 1, 0]
    for new, old in zip((p, m, v), got[0][3:6]):
        assert torch.equal(new[s5:s5 + n5], old[s5:s5 + n5])
    flat = torch.cat(pouts)
    assert torch.equal(flat[s5:s5 + n5], got[0][3][s5:s5 + n5].to(flat.dtype))


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_all_excluded_is_the_adamw_step(cuda, gdtype):
    """adapt all zero: q = 1 everywhere and the step is AdamW's (agg_update, n = 1); the two
    differ only in where the decay term is rounded."""
    from consensusml_amd.ops import kernels as K
    p0, gs = LO.inputs(gdtype)
    got = LO.device_steps(cuda, p0, gs, 0.37, 0.01, "one-bf16", adapt=[0] * 7)
    p = p0.to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    h = LO.HYPER
    for k, g in enumerate(gs, 1):
        o = K.OptArgs(kind="adamw", lr=h["lr"], weight_decay=0.01, beta1=h["b1"], beta2=h["b2"],
                      eps=h["eps"], step=k, gscale=0.37)
        K.agg_update(g.to(cuda)[None], combine="weighted", n=1, opt=o, master=p, s1=m, s2=v)
        assert bool((got[k - 1][1] == 1).all())
        for s, n in RANGES:
            for a, b in zip(got[k - 1][3:6], (p, m, v)):
                torch.testing.assert_close(a[s:s + n], b[s:s + n].cpu(), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("topo", ["allreduce", "sharded"])
def test_engine_step_matches_cpu_path(cuda, topo):
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    # the first step's direction is x / (|x| + eps): with eps far above the 1e-7 by which the two
    # devices' gradients differ, u moves by 1e-4 of that difference, not by a sign
    cfg = LO.engine_cfg(topo, 2, 1e-3)
    g = ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, cuda, "none"))
    c = ConsensusTrainer(copy.deepcopy(cfg), info=DistInfo(0, 1, 0, torch.device("cpu"), "none"))
    c.model.load_state_dict({k: v.cpu() for k, v in g.model.state_dict().items()})
    c.engine.master.copy_(g.engine.master.cpu())
    batches = [c.task.make_batch(16, gen) for gen in c.gens]
    for tr, dev in ((c, "cpu"), (g, cuda)):
        tr.engine.zero_grad()
        for w, (x, y) in enumerate(batches):
            tr.engine.bind_worker(w)
            tr.task.loss_fn(tr.model, (x.to(dev), y.to(dev))).backward()
        tr.engine.step()
    st = g.engine.lamb_stats.cpu()
    assert not bool((st[:, 2] == 1).all()) and float(st[:, 3].sum()) == 0.0
    torch.testing.assert_close(st[:, :3], c.engine.lamb_stats[:, :3], rtol=1e-4, atol=0)
    for a, b in zip((c.engine.master, c.engine.s1, c.engine.s2),
                    (g.engine.master, g.engine.s1, g.engine.s2)):
        torch.testing.assert_close(a, b.cpu(), rtol=RTOL, atol=ATOL)
    g.close()
    c.close()


def test_fused_lamb_against_oracle(cuda):
    """Two bf16 tensors with an fp32 master, three steps of explicit gradients."""
    from consensusml_amd.optim import FusedLAMB
    torch.manual_seed(0)
    lin = torch.nn.Linear(67, 9).to(device=cuda, dtype=torch.bfloat16)
    h = LO.HYPER
    opt = FusedLAMB(lin.parameters(), lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"],
                    weight_decay=0.01)
    params = list(lin.parameters())
    state = [[p.detach().cpu().reshape(-1), torch.zeros(p.numel()), torch.zeros(p.numel())]
             for p in params]
    gen = torch.Generator().manual_seed(3)
    for k in (1, 2, 3):
        qs = []
        for i, p in enumerate(params):
            g = torch.randn(p.shape, generator=gen).to(torch.bfloat16)
            p.grad = g.to(cuda)
            w, m, v = state[i]
            *state[i], q, _, _ = LO.tensor_step(w, g.reshape(-1), m, v, k=k, scale=0.5, wd=0.01,
                                                adapted=p.dim() >= 2, **h)
            qs.append(q)
        opt.step(grad_scale=0.5)
        st = opt.lamb_stats[0].cpu()
        assert qs[0] != 1.0 and qs[1] == 1.0
        assert st[:, 2].tolist() == pytest.approx(qs, rel=LO.RTOL_U)
    for p, (w, _, _) in zip(params, state):
        master = opt.state[p]["master"]
        torch.testing.assert_close(master.cpu().double().reshape(-1), w, rtol=RTOL, atol=ATOL)
        assert torch.equal(p.detach(), master.to(torch.bfloat16))
