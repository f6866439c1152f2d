"""Global-norm clipping of the aggregate (``optim.clip_norm``, ``max_grad_norm``) on the CPU paths:
the fp64 definitions, the engine against ``torch.nn.utils.clip_grad_norm_``, the topologies
against each other, the off switch, the step bound and the fused optimizers."""
import copy
import logging
import math

import pytest
import torch

from consensusml_amd import TrainConfig
from consensusml_amd.ops import kernels as K
from consensusml_amd.ops import reference as ref
from consensusml_amd.optim import FusedAdamW, FusedSGD
from consensusml_amd.parallel.dist import DistInfo
from consensusml_amd.trainer.trainer import ConsensusTrainer

CPU = DistInfo(0, 1, 0, torch.device("cpu"), "none")


def make_cfg(rule="median", topo="sharded", V=5, f=1, opt="sgd", clip=0.0):
    """The construction of tests/test_engine_cpu.py::make_cfg plus ``optim.clip_norm``."""
    cfg = TrainConfig()
    cfg.dtype = "fp32"
    cfg.virtual_workers = V
    cfg.agg.rule = rule
    cfg.agg.f = f
    cfg.topology.kind = topo
    cfg.optim.name = opt
    cfg.optim.lr = 0.1 if opt == "sgd" else 0.01
    cfg.optim.clip_norm = clip
    cfg.batch_per_worker = 32
    cfg.model.extra = {"classes": 2}
    return cfg


def _flat(model):
    return torch.cat([p.detach().reshape(-1).float() for p in model.parameters()])


# ------------------------------------------------------------------------------- definitions
def test_sq_norm_reference_against_fp64_torch():
    g = torch.Generator().manual_seed(0)
    segs = [torch.randn(1000, generator=g), torch.randn(1, generator=g),
            torch.randn(77, generator=g).to(torch.bfloat16).float()]
    want = sum((s.double() ** 2).sum() for s in segs)
    got = ref.sq_norm(segs, 1.0)
    assert got.dtype == torch.float64
    torch.testing.assert_close(got, want, rtol=1e-14, atol=0)
    # scale: the product is rounded to fp32 first, the square and the sum are fp64
    sc = 1.0 / 3.0
    want = sum(((s * torch.tensor(sc, dtype=torch.float32)).double() ** 2).sum() for s in segs)
    torch.testing.assert_close(ref.sq_norm(segs, sc), want, rtol=1e-14, atol=0)
    bf = [s.to(torch.bfloat16) for s in segs]
    want = sum((s.double() ** 2).sum() for s in bf)
    torch.testing.assert_close(ref.sq_norm(bf, 1.0), want, rtol=1e-14, atol=0)
    out = torch.zeros(1, dtype=torch.float64)
    K.sq_norm(bf, 1.0, None, out)
    torch.testing.assert_close(out[0], want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("norm2,c,base,coef", [
    (4.0, 1.0, 1.0, 1.0 / (2.0 + 1e-6)),      # active clip
    (4.0, 1.0, 0.125, 1.0 / (2.0 + 1e-6)),    # ... times a gradient scale
    (0.25, 1.0, 1.0, 1.0),                    # norm < c: exactly 1
    (0.25, 1.0, 0.125, 1.0),
    (0.0, 1.0, 1.0, 1.0),                     # norm 0
    (0.0, 1e-9, 1.0, 1e-9 / 1e-6),            # ... with c below the 1e-6 floor
])
def test_clip_coef_reference(norm2, c, base, coef):
    w, norm, cf, bad = ref.clip_coef(torch.tensor([norm2], dtype=torch.float64), c, base)
    assert bad == 0
    assert float(norm) == math.sqrt(norm2)
    assert float(cf) == pytest.approx(coef, rel=1e-15)
    if coef == 1.0:
        assert float(cf) == 1.0
        assert float(w) == float(torch.tensor(base, dtype=torch.float32))    # bit-exact base
    assert w.dtype == torch.float32
    assert float(w) == float(torch.tensor(float(torch.tensor(base, dtype=torch.float32)) * coef,
                                          dtype=torch.float64).float())
    # the dispatching wrapper, CPU path: same numbers, stats filled, counter untouched
    w_out = torch.full((1,), -1.0)
    stats = torch.zeros(K.CLIP_STATS, dtype=torch.float64)
    K.clip_coef(torch.tensor([norm2], dtype=torch.float64), c, base, w_out, stats)
    assert float(w_out) == float(w)
    assert stats.tolist() == [math.sqrt(norm2), float(cf), 0.0, norm2]
    # reduced: the sum comes from there instead
    K.clip_coef(torch.tensor([123.0], dtype=torch.float64), c, base, w_out, stats,
                reduced=torch.tensor([norm2], dtype=torch.float64))
    assert float(w_out) == float(w) and stats[3] == norm2


@pytest.mark.parametrize("bad", [float("inf"), float("nan"), -1.0])
def test_clip_coef_non_finite_is_zero_and_counted(bad):
    w, norm, cf, flag = ref.clip_coef(torch.tensor([bad], dtype=torch.float64), 1.0, 0.5)
    assert flag == 1 and float(cf) == 0.0 and float(w) == 0.0
    w_out = torch.ones(1)
    stats = torch.zeros(K.CLIP_STATS, dtype=torch.float64)
    for k in (1, 2):
        K.clip_coef(torch.tensor([bad], dtype=torch.float64), 1.0, 0.5, w_out, stats)
        assert float(w_out) == 0.0 and stats[1] == 0.0 and stats[2] == k


def test_sq_norm_of_non_finite_input():
    for v in (float("inf"), float("nan")):
        x = torch.ones(10)
        x[3] = v
        n2 = ref.sq_norm([x], 1.0)
        assert not torch.isfinite(n2)
        assert ref.clip_coef(n2.reshape(1), 1.0, 1.0)[3] == 1


# ------------------------------------------------------------------------------- engine / torch
def _first_norm(cfg):
    """The first step's aggregate norm, measured with a huge threshold (an inactive clip)."""
    c = copy.deepcopy(cfg)
    c.optim.clip_norm = 1e30
    tr = ConsensusTrainer(c, info=CPU)
    tr.train_step()
    st = tr.engine.grad_stats.tolist()
    tr.close()
    assert st[1] == 1.0 and st[0] > 0
    return st[0]


def test_engine_matches_torch_sgd_with_clip():
    """tests/test_engine_cpu.py::test_engine_matches_torch_sgd with an active clip on both sides."""
    cfg = make_cfg("mean", "sharded", V=3)
    cfg.optim.weight_decay = 0.01
    cfg.optim.nesterov = True
    c = 0.5 * _first_norm(cfg)
    cfg.optim.clip_norm = c
    tr = ConsensusTrainer(cfg, info=CPU)
    ref_model = copy.deepcopy(tr.model)
    opt = torch.optim.SGD(ref_model.parameters(), lr=0.1, momentum=0.9, weight_decay=0.01,
                          nesterov=True)
    gens = [torch.Generator().manual_seed(cfg.seed * 1000 + v) for v in range(3)]
    coefs = []
    for _ in range(4):
        opt.zero_grad()
        for v in range(3):
            b = tr.task.make_batch(32, gens[v])
            (tr.task.loss_fn(ref_model, b) / 3).backward()
        total = torch.nn.utils.clip_grad_norm_(ref_model.parameters(), c)
        opt.step()
        tr.train_step()
        st = tr.engine.grad_stats.tolist()
        assert st[0] == pytest.approx(float(total), rel=1e-5)
        coefs.append(st[1])
    assert coefs[0] == pytest.approx(0.5, rel=1e-4) and min(coefs) < 1.0      # the clip is active
    for a, b in zip(ref_model.parameters(), tr.model.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_adam_engine_matches_torch_with_clip():
    """tests/test_engine_cpu.py::test_adam_engine_matches_torch with an active clip."""
    cfg = make_cfg("mean", "allgather", V=2, opt="adamw")
    cfg.optim.weight_decay = 0.05
    c = 0.5 * _first_norm(cfg)
    cfg.optim.clip_norm = c
    tr = ConsensusTrainer(cfg, info=CPU)
    ref_model = copy.deepcopy(tr.model)
    opt = torch.optim.AdamW(ref_model.parameters(), lr=0.01, weight_decay=0.05)
    gens = [torch.Generator().manual_seed(cfg.seed * 1000 + v) for v in range(2)]
    for _ in range(4):
        opt.zero_grad()
        for v in range(2):
            b = tr.task.make_batch(32, gens[v])
            (tr.task.loss_fn(ref_model, b) / 2).backward()
        torch.nn.utils.clip_grad_norm_(ref_model.parameters(), c)
        opt.step()
        tr.train_step()
        assert tr.engine.grad_stats[1] < 1.0
    for a, b in zip(ref_model.parameters(), tr.model.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.fixture(scope="module")
def clipped_allreduce():
    cfg = make_cfg("mean", "allreduce", V=4)
    c = 0.5 * _first_norm(cfg)
    cfg.optim.clip_norm = c
    tr = ConsensusTrainer(cfg, info=CPU)
    tr.fit(5, log_every=0)
    return c, [p.detach().clone() for p in tr.model.parameters()]


@pytest.mark.parametrize("topo", ["allreduce", "allgather", "sharded", "gossip"])
def test_mean_topologies_agree_under_clip(clipped_allreduce, topo):
    """The bar of tests/test_engine_cpu.py::test_mean_topologies_agree, every step clipped."""
    c, want = clipped_allreduce
    tr = ConsensusTrainer(make_cfg("mean", topo, V=4, clip=c), info=CPU)
    seen = []
    for _ in range(5):
        tr.train_step()
        seen.append(float(tr.engine.grad_stats[1]))
    assert min(seen) < 1.0
    for a, b in zip(want, tr.model.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


OFF_CASES = [
    ("mean", "allreduce", 0, "none"),
    ("median", "sharded", 1, "none"),
    ("krum", "allgather", 1, "none"),
    ("centered_clip", "sharded", 1, "none"),
    ("meamed", "sharded", 1, "nnm"),
    ("mean", "gossip", 0, "none"),
]


@pytest.mark.parametrize("rule,topo,f,pre", OFF_CASES, ids=[f"{r}-{t}" for r, t, _, _ in OFF_CASES])
@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_huge_clip_norm_is_bit_identical_to_off(rule, topo, f, pre, opt):
    """clip_norm = 1e30: coefficient exactly 1, so materialise + norm + weighted update gives
    the bits of the fused pass."""
    out = []
    for clip in (0.0, 1e30):
        cfg = make_cfg(rule, topo, V=5, f=f, opt=opt, clip=clip)
        cfg.agg.pre = pre
        cfg.topology.bucket_mb = 0.002          # several buckets
        tr = ConsensusTrainer(cfg, info=CPU)
        tr.fit(3, log_every=0)
        e = tr.engine
        out.append((_flat(tr.model), e.master.clone(),
                    None if e.s1 is None else e.s1.clone(),
                    None if e.gout is None or rule != "centered_clip" else e.gout.clone()))
        assert (e.grad_stats is None) == (clip == 0.0)
        if clip:
            assert e.grad_stats[1] == 1.0 and e.grad_stats[2] == 0.0
    for a, b in zip(*out):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


def test_clip_bounds_the_step_under_a_scaled_attacker():
    """mean under ``scaled`` (x100, one Byzantine of 5), plain SGD, fp32: every step of the
    clipped run moves the master by at most lr * c * (1 + 1e-5); the unclipped run does not."""
    c, lr = 0.05, 0.1

    def run(clip):
        cfg = make_cfg("mean", "sharded", V=5, f=0, clip=clip)
        cfg.optim.momentum = 0.0
        cfg.optim.weight_decay = 0.0
        cfg.optim.lr = lr
        cfg.fault.kind = "scaled"
        cfg.fault.scale = 100.0
        cfg.fault.ranks = [2]
        tr = ConsensusTrainer(cfg, info=CPU)
        steps = []
        for _ in range(5):
            before = tr.engine.master.clone()
            tr.train_step()
            steps.append(float((tr.engine.master - before).double().norm()))
        return steps
    clipped, free = run(c), run(0.0)
    assert all(s <= lr * c * (1 + 1e-5) for s in clipped), clipped
    assert all(s > 0 for s in clipped)
    assert max(free) > lr * c * (1 + 1e-5), free


def test_non_finite_aggregate_applies_a_zero_gradient():
    """A NaN row through the mean: coefficient 0, the counter moves, the parameters stay (plain
    SGD), nothing in the state turns non-finite."""
    cfg = make_cfg("mean", "allgather", V=3, f=0, clip=1.0)
    cfg.optim.momentum = 0.9
    cfg.fault.kind = "nan"
    cfg.fault.ranks = [1]
    cfg.fault.start_step = 1
    tr = ConsensusTrainer(cfg, info=CPU)
    tr.train_step()
    before = tr.engine.master.clone()
    s1 = tr.engine.s1.clone()
    tr.train_step()
    st = tr.engine.grad_stats.tolist()
    assert st[1] == 0.0 and st[2] == 1.0
    assert torch.isfinite(tr.engine.master).all() and torch.isfinite(tr.engine.s1).all()
    torch.testing.assert_close(tr.engine.s1, 0.9 * s1)                  # momentum of a zero gradient
    torch.testing.assert_close(tr.engine.master, before - 0.1 * 0.9 * s1)


def test_worker_momentum_clips_the_aggregate_of_momenta():
    """The clipped quantity is the rule's aggregate of the momenta: the step is bounded by
    lr * c (plus the fp32 rounding of the master itself, at most half an ulp per coordinate:
    2^-24 ||master||), while the unclipped momenta are far longer than c."""
    c = 0.05
    cfg = make_cfg("median", "sharded", V=5, f=1, clip=c)
    cfg.optim.worker_momentum = True
    cfg.optim.momentum = 0.9
    tr = ConsensusTrainer(cfg, info=CPU)
    for _ in range(3):
        before = tr.engine.master.clone()
        tr.train_step()
        slack = 2.0 ** -24 * float(before.double().norm())
        assert float((tr.engine.master - before).double().norm()) <= 0.1 * c * (1 + 1e-5) + slack
        assert tr.engine.grad_stats[0] > 2 * c and tr.engine.grad_stats[1] < 0.5


# ------------------------------------------------------------------------------- fused optimizers
class _Mixed(torch.nn.Module):
    """An fp32 trunk and a bf16 head: two param groups, mixed parameter dtypes."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.trunk = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(192, 32),
                                         torch.nn.GELU())
        self.head = torch.nn.Linear(32, 5).to(torch.bfloat16)

    def forward(self, x):
        return self.head(self.trunk(x).to(torch.bfloat16)).float()


def _mixed_groups(m, lr2):
    return [{"params": list(m.trunk.parameters())},
            {"params": list(m.head.parameters()), "lr": lr2}]


@pytest.mark.parametrize("fused_cls,torch_cls,kw", [
    (FusedSGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-2)),
    (FusedAdamW, torch.optim.AdamW, dict(lr=1e-2, weight_decay=0.05)),
])
@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 64])
def test_fused_optimizers_match_torch_with_clip_grad_norm(fused_cls, torch_cls, kw, grad_scale):
    """``max_grad_norm=c`` against the torch optimizer behind ``clip_grad_norm_``. The reference
    is an fp32 copy (the fused masters) fed the fused model's own gradients, so the comparison is
    of the clipping and the update alone: fp32 tolerances of
    tests/test_optim.py::test_param_groups_and_grad_scale for the masters, and bf16 parameters are
    the rounding of their master (``::test_bf16_master_weights_cpu``)."""
    a = _Mixed()
    b = copy.deepcopy(a).float()
    c = 0.3
    oa = fused_cls(_mixed_groups(a, kw["lr"] * 0.5), max_grad_norm=c, **kw)
    ob = torch_cls(_mixed_groups(b, kw["lr"] * 0.5), **kw)
    assert len(oa.flat_buffers()) == 2
    g = torch.Generator().manual_seed(1)
    coefs = []
    for _ in range(4):
        x = torch.randn(6, 3, 8, 8, generator=g)
        y = torch.randint(0, 5, (6,), generator=g)
        oa.zero_grad()
        (torch.nn.functional.cross_entropy(a(x), y) / grad_scale).backward()
        for p, q in zip(a.parameters(), b.parameters()):
            q.grad = p.grad.detach().float() * grad_scale    # (exact: a power of two)
        total = torch.nn.utils.clip_grad_norm_(b.parameters(), c)
        oa.step(grad_scale=grad_scale)
        ob.step()
        assert float(oa.grad_stats[0]) == pytest.approx(float(total), rel=1e-5)
        coefs.append(float(oa.grad_stats[1]))
    assert min(coefs) < 1.0
    for p, q in zip(a.parameters(), b.parameters()):
        master = oa.state[p]["master"] if p.dtype != torch.float32 else p
        torch.testing.assert_close(master.detach(), q.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(p.detach(), master.detach().to(p.dtype), rtol=0, atol=0)


def test_fused_max_grad_norm_off_and_invalid():
    m = _Mixed()
    with pytest.raises(ValueError):
        FusedSGD(m.parameters(), lr=0.1, max_grad_norm=-1.0)
    with pytest.raises(ValueError):
        FusedAdamW(m.parameters(), lr=0.1, max_grad_norm=float("nan"))
    assert FusedSGD(m.parameters(), lr=0.1).grad_stats is None


# ------------------------------------------------------------------------------- config
@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -1e-9])
def test_config_rejects_bad_clip_norm(bad):
    cfg = make_cfg("mean", "sharded", V=2, f=0, clip=bad)
    with pytest.raises(ValueError, match="clip_norm"):
        cfg.validate(2)
    with pytest.raises(ValueError, match="clip_norm"):
        ConsensusTrainer(cfg, info=CPU)


def test_config_key_and_cli_override():
    cfg = TrainConfig().override(["optim.clip_norm=1"])
    assert cfg.optim.clip_norm == 1.0 and isinstance(cfg.optim.clip_norm, float)
    assert TrainConfig().optim.clip_norm == 0.0


def test_early_update_is_off_under_gossip_with_clipping(caplog):
    """(CPU engines never run the early update; what is checked is the switch and its log line,
    on the configuration that would otherwise take it: gossip, one worker per rank.)"""
    cfg = make_cfg("mean", "gossip", V=1, f=0, clip=1.0)
    assert cfg.topology.early_update
    with caplog.at_level(logging.INFO, logger="consensusml_amd.parallel.engine"):
        tr = ConsensusTrainer(cfg, info=CPU)
    assert tr.engine.early_update is False and tr.engine._opt_stream is None
    assert sum("early_update" in r.getMessage() for r in caplog.records) == 1
    tr.train_step()
    assert tr.engine.gout is None            # the direct path keeps no aggregate buffer
    assert 0 < tr.engine.grad_stats[1] <= 1.0


def test_fit_result_and_log_carry_norm_and_coef(tmp_path):
    import json
    cfg = make_cfg("median", "sharded", V=5, f=1, clip=0.01)
    cfg.log_path = str(tmp_path / "log.jsonl")
    tr = ConsensusTrainer(cfg, info=CPU)
    r = tr.fit(4, log_every=2)
    tr.close()
    assert r["clip_coef"] < 1.0 and r["grad_norm"] > 0.01
    recs = [json.loads(l) for l in open(cfg.log_path)]
    assert [x["step"] for x in recs] == [2, 4]
    assert all(x["clip_coef"] == pytest.approx(0.01 / (x["grad_norm"] + 1e-6)) for x in recs)
    assert recs[-1]["grad_norm"] == r["grad_norm"]
    r0 = ConsensusTrainer(make_cfg("median", "sharded", V=5, f=1), info=CPU).fit(2, log_every=1)
    assert "grad_norm" not in r0 and "clip_coef" not in r0
