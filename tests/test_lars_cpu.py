"""LARS (``optim.name=lars``, ``FusedLARS``) on the CPU paths: ``FlatModel.tensor_ranges``
against brute force, the reference functions and the engine against the independent per-tensor
oracle of tests/lars_oracle.py, the fused optimizer and the config."""
import json
import math

import pytest
import torch

import lars_oracle as LO
from consensusml_amd import TrainConfig
from consensusml_amd.config import _flatten
from consensusml_amd.ops import kernels as K
from consensusml_amd.ops import reference as ref
from consensusml_amd.optim import FusedLARS, build_optimizer
from consensusml_amd.parallel.dist import DistInfo
from consensusml_amd.parallel.flat import FlatModel
from consensusml_amd.trainer.trainer import ConsensusTrainer

CPU = DistInfo(0, 1, 0, torch.device("cpu"), "none")
RTOL, ATOL = 2e-5, 2e-6      # tests/test_clip_norm_gpu.py: a fused fp32 update against a reference
                             # path over a few steps


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17),
                               torch.nn.Linear(17, 70), torch.nn.Linear(70, 3, bias=False))


# ------------------------------------------------------------------------------- tensor_ranges
@pytest.mark.parametrize("bucket_mb,min_buckets", [(64.0, 1), (0.002, 3)])
@pytest.mark.parametrize("world", [1, 2, 4])
def test_tensor_ranges_against_brute_force(world, bucket_mb, min_buckets):
    fl = FlatModel(_net(), world, bucket_mb, param_dtype=torch.float32)
    assert len(fl.buckets) >= min_buckets and (min_buckets > 1 or len(fl.buckets) == 1)
    owner = torch.full((fl.total,), -1, dtype=torch.int64)
    for i, p in enumerate(fl.params):
        owner[fl.param_offset[i]:fl.param_offset[i] + p.numel()] = i
    full = fl.tensor_ranges()
    assert sorted(i for i, _, _ in full) == list(range(len(fl.params)))
    for i, s, n in full:
        assert (s, n) == (fl.param_offset[i], fl.params[i].numel())
    empties = 0
    for rank in range(world):
        want = fl.gather_shard_vector(owner, rank)
        got = torch.full_like(want, -1)
        rs = fl.tensor_ranges(rank)
        assert [i for i, _, _ in rs] == [i for i, _, _ in full]      # the same order on every rank
        prev = 0
        for i, s, n in rs:
            assert s % 8 == 0 and n >= 0 and s >= prev and s + n <= want.numel()
            assert bool((got[s:s + n] == -1).all())                 # ranges do not overlap
            got[s:s + n] = i
            prev = s
            empties += n == 0
        assert torch.equal(got, want)
        assert rs[0][1] == 0
    total = {i: 0 for i in range(len(fl.params))}
    for rank in range(world):
        for i, _, n in fl.tensor_ranges(rank):
            total[i] += n
    assert all(total[i] == p.numel() for i, p in enumerate(fl.params))
    if world == 4:
        assert empties > 0      # some rank holds nothing of some tensor


# ------------------------------------------------------------------------------- definitions
def _vector(gen, sizes, dtype=torch.float32):
    """A state vector with tensors of ``sizes`` at 8-aligned starts and garbage in the padding."""
    starts, off = [], 0
    for n in sizes:
        starts.append(off)
        off += -(-n // 8) * 8
    total = -(-max(off, 8) // 64) * 64
    p = torch.randn(total, generator=gen)
    g = torch.randn(total, generator=gen).to(dtype)
    return starts, total, p, g


def test_seg_sq_norm_reference_against_fp64_torch():
    gen = torch.Generator().manual_seed(0)
    sizes = [1, 7, 8, 9, 0, 63, 1000]
    for dtype in (torch.float32, torch.bfloat16):
        starts, total, p, g = _vector(gen, sizes, dtype)
        for sc in (1.0, 1.0 / 3.0):
            got = ref.seg_sq_norm(p, g, sc, starts, sizes)
            assert got.dtype == torch.float64 and got.shape == (len(sizes), 2)
            for t, (s, n) in enumerate(zip(starts, sizes)):
                gv = (g[s:s + n].float() * torch.tensor(sc, dtype=torch.float32)).double()
                torch.testing.assert_close(got[t, 0], (p[s:s + n].double() ** 2).sum(),
                                           rtol=1e-14, atol=0)
                torch.testing.assert_close(got[t, 1], (gv ** 2).sum(), rtol=1e-14, atol=0)
            # the dispatching wrapper, CPU path; padding garbage changes nothing
            plan = K.lars_plan(starts, sizes, chunk=64, total=total)
            out = K.seg_sq_norm(p, g, sc, plan)
            assert torch.equal(out, got)
            p2, g2 = p.clone(), g.clone()
            for s, n, e in zip(starts, sizes, starts[1:] + [total]):
                p2[s + n:e] = float("nan")
                g2[s + n:e] = float("inf")
            assert torch.equal(K.seg_sq_norm(p2, g2, sc, plan), got)


def test_lars_plan_tables_and_checks():
    plan = K.lars_plan([0, 8, 8, 1032], [5, 0, 1021, 64], chunk=512, total=1152)
    assert plan.T == 4 and plan.total == 1152 and plan.starts == [0, 8, 8, 1032, 1152]
    assert plan.items.tolist() == [[0, 0, 5], [2, 8, 512], [2, 520, 509], [3, 1032, 64]]
    assert plan.item_off.tolist() == [0, 1, 1, 3, 4]
    assert K.lars_plan([0], [9]).total == 16
    for bad in (dict(starts=[0, 4], numels=[4, 4]), dict(starts=[8], numels=[4]),
                dict(starts=[0, 8], numels=[9, 4]), dict(starts=[0], numels=[4], chunk=12),
                dict(starts=[0], numels=[40], total=32), dict(starts=[0], numels=[4], total=12),
                dict(starts=[], numels=[])):
        with pytest.raises(ValueError, match="lars_plan"):
            K.lars_plan(**bad)


# (sw, sg, adapted) -> which branch
BRANCHES = [
    (4.0, 0.25, True, "adapted"), (4.0, 0.25, False, "excluded"), (0.0, 0.25, True, "wn0"),
    (4.0, 0.0, True, "gn0"), (4.0, float("inf"), True, "bad"), (4.0, float("nan"), False, "bad"),
    (float("inf"), 1.0, True, "bad"),
]


@pytest.mark.parametrize("wd,eps", [(0.0, 0.0), (0.05, 1e-8)])
def test_lars_ratio_reference_every_branch(wd, eps):
    pairs = torch.tensor([[a, b] for a, b, _, _ in BRANCHES], dtype=torch.float64)
    adapt = torch.tensor([ad for _, _, ad, _ in BRANCHES], dtype=torch.uint8)
    q, st, bad = ref.lars_ratio(pairs, adapt, 0.02, wd, eps)
    assert q.dtype == torch.float32 and st.dtype == torch.float64
    for t, (sw, sg, ad, kind) in enumerate(BRANCHES):
        # the oracle on a one-element tensor with that norm
        _, _, want, wn, gn = LO.lars_tensor_step(
            torch.tensor([math.sqrt(sw) if math.isfinite(sw) else sw]),
            torch.tensor([math.sqrt(sg) if math.isfinite(sg) else sg], dtype=torch.float64),
            None, lr=0.1, wd=wd, trust=0.02, eps=eps, adapted=ad)
        assert float(q[t]) == pytest.approx(want, rel=1e-7), kind
        assert int(bad[t]) == (kind == "bad")
        if kind == "bad":
            assert float(q[t]) == 0.0
        elif kind == "adapted":
            assert float(q[t]) == float(torch.tensor(0.02 * 2.0 / (0.5 + wd * 2.0 + eps),
                                                     dtype=torch.float64).float())
            assert st[t].tolist() == [2.0, 0.5, float(q[t])]
        else:
            assert float(q[t]) == 1.0
    # the wrapper: stats filled, the counter accumulates, ``reduced`` replaces the pairs
    qo = torch.full((len(BRANCHES),), -1.0)
    stats = torch.zeros(len(BRANCHES), K.LARS_STATS, dtype=torch.float64)
    for k in (1, 2):
        K.lars_ratio(torch.zeros_like(pairs), adapt, 0.02, wd, eps, qo, stats, reduced=pairs)
        assert torch.equal(qo, q)
        assert stats[:, 3].tolist() == [float(k * b) for b in bad.tolist()]
    K.lars_ratio(pairs, adapt, 0.02, wd, eps, qo, stats)
    assert torch.equal(qo, q) and torch.equal(stats[:4, :3], st[:4])


@pytest.mark.parametrize("momentum,nesterov,first", [(0.0, False, False), (0.9, False, True),
                                                     (0.9, True, False)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_reference_update_against_oracle(dtype, momentum, nesterov, first):
    gen = torch.Generator().manual_seed(1)
    sizes = [64, 7, 9, 300, 1]
    starts, total, p, g = _vector(gen, sizes, dtype)
    buf = torch.randn(total, generator=gen) if momentum else None
    adapt = [True, False, True, True, False]
    kw = dict(lr=0.1, momentum=momentum, wd=0.01, nesterov=nesterov, first=first, trust=0.02,
              eps=1e-8)
    sc = 0.125
    plan = K.lars_plan(starts, sizes, total=total)
    pairs = K.seg_sq_norm(p, g, sc, plan)
    q = torch.zeros(plan.T)
    stats = torch.zeros(plan.T, K.LARS_STATS, dtype=torch.float64)
    K.lars_ratio(pairs, torch.tensor(adapt, dtype=torch.uint8), 0.02, 0.01, 1e-8, q, stats)
    want_m, want_b, rows = LO.lars_vector_step(p, g.double() * sc, buf, list(zip(starts, sizes)),
                                               adapt, **kw)
    assert q.tolist() == pytest.approx([r[0] for r in rows], rel=1e-6)
    m, b = p.clone(), (buf.clone() if buf is not None else None)
    pout = torch.zeros(total, dtype=torch.bfloat16)
    K.lars_update(g, sc, plan, q, K.OptArgs(kind="lars", lr=0.1, momentum=momentum,
                                            weight_decay=0.01, nesterov=nesterov, first=first),
                  m, b, segs=[(pout, 0, total)])
    for s, n in zip(starts, sizes):
        torch.testing.assert_close(m[s:s + n].double(), want_m[s:s + n], rtol=RTOL, atol=ATOL)
        if momentum:
            torch.testing.assert_close(b[s:s + n].double(), want_b[s:s + n], rtol=RTOL, atol=ATOL)
    assert torch.equal(pout, m.to(torch.bfloat16))


def test_zero_ratio_with_nan_gradient_poisons_nothing():
    gen = torch.Generator().manual_seed(2)
    sizes = [37, 24]
    starts, total, p, g = _vector(gen, sizes)
    g[3] = float("nan")
    g[38] = float("inf")        # the padding of tensor 0: no norm sees it
    buf = torch.randn(total, generator=gen)
    plan = K.lars_plan(starts, sizes, total=total)
    pairs = K.seg_sq_norm(p, g, 1.0, plan)
    assert not math.isfinite(float(pairs[0, 1])) and math.isfinite(float(pairs[1, 1]))
    q = torch.ones(2)
    stats = torch.zeros(2, K.LARS_STATS, dtype=torch.float64)
    K.lars_ratio(pairs, torch.ones(2, dtype=torch.uint8), 0.02, 0.01, 0.0, q, stats)
    assert float(q[0]) == 0.0 and float(q[1]) > 0 and stats[:, 3].tolist() == [1.0, 0.0]
    m, b = p.clone(), buf.clone()
    K.lars_update(g, 1.0, plan, q, K.OptArgs(kind="lars", lr=0.1, momentum=0.9,
                                             weight_decay=0.01), m, b)
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(b).all())
    # tensor 0 took a zero gradient: its buffer only decayed, its master moved by -lr * buffer
    torch.testing.assert_close(b[:37], 0.9 * buf[:37])
    torch.testing.assert_close(m[:37], p[:37] - 0.1 * b[:37])
    with pytest.raises(ValueError, match="lars"):
        K.OptArgs(kind="lars").opt_id()


# ------------------------------------------------------------------------------- engine
def make_cfg(rule, topo, V, f):
    cfg = TrainConfig()
    cfg.dtype = "fp32"
    cfg.virtual_workers = V
    cfg.agg.rule = rule
    cfg.agg.f = f
    cfg.topology.kind = topo
    cfg.topology.bucket_mb = 0.0004
    cfg.optim.name = "lars"
    cfg.optim.lr = 0.5
    cfg.optim.momentum = 0.9
    cfg.optim.weight_decay = 0.01
    cfg.optim.trust_coef = 0.02
    cfg.batch_per_worker = 32
    cfg.model.extra = {"classes": 2}
    return cfg


ENGINE_CASES = [(r, t, 4, f) for r, f in (("mean", 0), ("median", 1), ("krum", 1))
                for t in ("allgather", "sharded")] + [("mean", "allreduce", 1, 0),
                                                      ("mean", "gossip", 1, 0)]


@pytest.mark.parametrize("rule,topo,V,f", ENGINE_CASES,
                         ids=[f"{r}-{t}-V{v}" for r, t, v, _ in ENGINE_CASES])
def test_engine_against_oracle(rule, topo, V, f):
    tr = ConsensusTrainer(make_cfg(rule, topo, V, f), info=CPU)
    e = tr.engine
    assert e.lars and not e.early_update and e.s2 is None and e.s1 is not None
    assert (e.gout is None) == (V == 1)
    assert len(e.flat.buckets) >= 3
    LO.check_engine_against_oracle(tr, 4, RTOL, ATOL)
    tr.close()


def test_engine_lars_is_not_adamw_and_logs_early_update(caplog):
    """The parent's fall-through ran AdamW for ``lars``; and the one-time log line."""
    import logging
    cfg = make_cfg("mean", "gossip", 1, 0)
    with caplog.at_level(logging.INFO, logger="consensusml_amd.parallel.engine"):
        tr = ConsensusTrainer(cfg, info=CPU)
    assert sum("optim.name=lars" in r.message and "early_update" in r.message
               for r in caplog.records) == 1
    assert tr.engine._opt_args().kind == "lars"
    tr.close()


# ------------------------------------------------------------------------------- FusedLARS
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fused_lars_against_oracle(dtype):
    net = _net().to(dtype)
    params = list(net.parameters())
    kw = dict(lr=0.2, momentum=0.9, weight_decay=0.01, nesterov=True, trust_coef=0.02, eps=1e-9)
    opt = FusedLARS(params, **kw)
    assert isinstance(build_optimizer("lars", list(_net().parameters()), lr=0.1), FusedLARS)
    m = [p.detach().double().reshape(-1) for p in params]
    b = [None] * len(params)
    gen = torch.Generator().manual_seed(5)
    for step in range(3):
        for i, p in enumerate(params):
            g = torch.randn(p.shape, generator=gen).to(dtype)
            p.grad = g.clone()
            m[i], b[i], q, wn, gn = LO.lars_tensor_step(
                m[i], g.double() * 0.5, b[i], lr=0.2, momentum=0.9, wd=0.01, nesterov=True,
                first=step == 0, trust=0.02, eps=1e-9, adapted=p.dim() >= 2)
            assert (q == 1.0) == (p.dim() < 2)
        opt.step(grad_scale=0.5)
        st = opt.lars_stats[0]
        assert st.shape == (len(params), K.LARS_STATS) and float(st[:, 3].sum()) == 0.0
    for i, p in enumerate(params):
        state = opt.state[p]
        master = state["master"] if dtype != torch.float32 else p.detach()
        torch.testing.assert_close(master.double().reshape(-1), m[i], rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(state["momentum_buffer"].double().reshape(-1), b[i],
                                   rtol=RTOL, atol=ATOL)
        if dtype != torch.float32:
            assert torch.equal(p.detach(), master.to(dtype))


def test_fused_lars_state_dict_round_trips_with_torch_sgd():
    gen = torch.Generator().manual_seed(6)
    a, b = _net(), _net()
    sgd = torch.optim.SGD(a.parameters(), lr=0.2, momentum=0.9, weight_decay=0.01)
    for p in a.parameters():
        p.grad = torch.randn(p.shape, generator=gen)
    sgd.step()
    lars = FusedLARS(b.parameters(), lr=0.2, momentum=0.9, weight_decay=0.01, trust_coef=0.02)
    lars.load_state_dict(sgd.state_dict())
    g = lars.param_groups[0]
    assert g["trust_coef"] == 0.02 and g["exclude_1d"] is True and g["step"] == 1
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(lars.state[pb]["momentum_buffer"], sgd.state[pa]["momentum_buffer"])
    # a step from the loaded state uses the loaded buffer (first = False)
    before = [lars.state[p]["momentum_buffer"].clone() for p in b.parameters()]
    for p in b.parameters():
        p.grad = torch.zeros_like(p)
    for p in b.parameters():
        p.data.zero_()          # wn = 0: q = 1, a zero gradient, no decay term
    lars.step()
    for p, b0 in zip(b.parameters(), before):
        torch.testing.assert_close(lars.state[p]["momentum_buffer"], 0.9 * b0)
    # and back into torch.optim.SGD
    sgd2 = torch.optim.SGD(_net().parameters(), lr=0.2, momentum=0.9)
    sgd2.load_state_dict(lars.state_dict())
    for p2, pb in zip(sgd2.param_groups[0]["params"], b.parameters()):
        assert torch.equal(sgd2.state[p2]["momentum_buffer"], lars.state[pb]["momentum_buffer"])


def test_fused_lars_rejections():
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedLARS(_net().parameters(), lr=0.1, max_grad_norm=1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="trust_coef"):
            FusedLARS(_net().parameters(), lr=0.1, trust_coef=bad)
    with pytest.raises(ValueError, match="Nesterov"):
        FusedLARS(_net().parameters(), lr=0.1, nesterov=True)


# ------------------------------------------------------------------------------- config
def test_config_rejections_and_round_trip():
    for bad in (0.0, -0.001, float("inf"), float("nan")):
        cfg = TrainConfig()
        cfg.optim.trust_coef = bad
        with pytest.raises(ValueError, match="trust_coef"):
            cfg.validate(4)
    cfg = TrainConfig().override(["optim.name=lars", "optim.clip_norm=1.0"])
    with pytest.raises(ValueError, match="lars.*clip_norm.*not implemented"):
        cfg.validate(4)
    cfg = TrainConfig().override(["optim.name=lars", "optim.worker_momentum=true"])
    with pytest.raises(ValueError, match="worker_momentum.*lars"):
        cfg.validate(4)
    cfg = TrainConfig().override(["optim.name=lars"])
    assert cfg.optim.trust_coef == 0.001 and cfg.optim.lars_exclude_1d is True
    cfg.validate(4)
    back = TrainConfig.from_dict(_flatten(json.loads(cfg.to_json())))
    assert back.to_json() == cfg.to_json() and back.optim.name == "lars"
    assert json.loads(cfg.to_json())["optim"]["trust_coef"] == 0.001

