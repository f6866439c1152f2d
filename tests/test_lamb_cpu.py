"""LAMB (``optim.name=lamb``, ``FusedLAMB``) on the CPU paths: the torch reference functions and
the trainer's four topologies against the independent fp64 oracle of tests/lamb_oracle.py, the
config's rejections and the fused optimizer's construction and state dict."""
import logging

import pytest
import torch

import lamb_oracle as LO
from consensusml_amd import TrainConfig
from consensusml_amd.optim import FusedLAMB, build_optimizer
from consensusml_amd.parallel.dist import DistInfo
from consensusml_amd.trainer.trainer import ConsensusTrainer
from lars_oracle import engine_aggregate


@pytest.mark.parametrize("variant", ["one-bf16", "two-fp32"])
@pytest.mark.parametrize("scale,wd", [(1.0, 0.0), (0.37, 0.01)])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_reference_against_oracle(gdtype, scale, wd, variant):
    p0, gs = LO.inputs(gdtype)
    got = LO.device_steps("cpu", p0, gs, scale, wd, variant)
    for k, (step, g) in enumerate(zip(got, gs), 1):
        LO.check_step(step, g, k, scale, wd)


@pytest.mark.parametrize("topo,V", [("allreduce", 2), ("allgather", 2), ("sharded", 2),
                                    ("gossip", 1)])
def test_trainer_against_oracle(topo, V, caplog):
    """Three steps; the oracle keeps its own fp64 state and is fed the aggregate the engine used."""
    cfg = LO.engine_cfg(topo, V, 1e-6)
    with caplog.at_level(logging.INFO, logger="consensusml_amd.parallel.engine"):
        tr = ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, torch.device("cpu"), "none"))
    assert sum("optim.name=lamb" in r.message and "early_update" in r.message
               for r in caplog.records) == (topo == "gossip")
    e, o = tr.engine, cfg.optim
    assert e.lamb and not e.early_update and e._opt_args().kind == "lamb"
    fl = e.flat
    ranges = [(fl.param_offset[i], p.numel()) for i, p in enumerate(fl.params)]
    adapt = [p.dim() >= 2 for p in fl.params]
    assert any(adapt) and not all(adapt)
    p, m, v = e.master.clone(), torch.zeros_like(e.master), torch.zeros_like(e.master)
    for k in (1, 2, 3):
        tr.train_step()
        p, m, v, rows = LO.vector_step(p, engine_aggregate(e), m, v, ranges, adapt, k=k, scale=1.0,
                                       wd=o.weight_decay, lr=o.lr, b1=o.betas[0], b2=o.betas[1],
                                       eps=o.eps)
        st = e.lamb_stats
        assert st.shape == (len(ranges), 4) and float(st[:, 3].sum()) == 0.0
        assert st[:, 2].tolist() == pytest.approx([q for q, _, _ in rows], rel=LO.RTOL_U)
        assert [q == 1.0 for q, _, _ in rows] == [not a for a in adapt]
    for got, want in ((e.master, p), (e.s1, m), (e.s2, v)):
        for s, n in ranges:
            torch.testing.assert_close(got[s:s + n].double(), want[s:s + n], rtol=LO.RTOL,
                                       atol=LO.ATOL)
    tr.close()


def test_config_rejections():
    cfg = TrainConfig()
    cfg.optim.name = "lamb"
    assert cfg.optim.lamb_exclude_1d is True
    cfg.optim.validate()
    cfg.optim.clip_norm = 1.0
    with pytest.raises(ValueError, match="lamb with optim.clip_norm"):
        cfg.optim.validate()
    cfg.optim.clip_norm = 0.0
    cfg.optim.worker_momentum = True
    with pytest.raises(ValueError, match="worker_momentum is not implemented with optim.name=lamb"):
        cfg.optim.validate()


def test_fused_lamb_builds_loads_adamw_state_and_rejects():
    torch.manual_seed(0)
    a = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17))
    b = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17))
    adamw = torch.optim.AdamW(a.parameters(), lr=0.01, eps=1e-6, weight_decay=0.01)
    for p in a.parameters():
        p.grad = torch.randn(p.shape)
    adamw.step()
    lamb = build_optimizer("lamb", b.parameters(), lr=0.01, weight_decay=0.01)
    assert isinstance(lamb, FusedLAMB)
    lamb.load_state_dict(adamw.state_dict())
    assert lamb.param_groups[0]["exclude_1d"] is True and lamb.param_groups[0]["step"] == 1
    for pa, pb in zip(a.parameters(), b.parameters()):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(lamb.state[pb][key], adamw.state[pa][key])
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedLAMB(b.parameters(), max_grad_norm=1.0)
    with pytest.raises(TypeError, match="fp32 / bf16"):
        FusedLAMB(b.half().parameters())
