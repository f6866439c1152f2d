"""``agg.pre=nnm`` across ranks (gloo, CPU): R ranks x 1 worker give the parameters of 1 rank x R
virtual workers on the same per-worker data. For the coordinate rules this pins that a sharded
run takes the per-bucket Gram and the all-reduce of G, so that every rank mixes its shard with
the same M."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_dist_gloo import _cfg, _free_port


def _nnm_cfg(rule, topo, V, f, steps):
    cfg = _cfg(rule, topo, V, f, steps)
    cfg.agg.pre = "nnm"
    return cfg


def _worker(rank, world, port, rule, topo, f, steps, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from consensusml_amd.parallel import dist as D
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    D._INFO = None
    info = D.init_distributed("gloo")
    tr = ConsensusTrainer(_nnm_cfg(rule, topo, 1, f, steps), info=info)
    tr.engine._gram_eager = True
    tr.fit(steps, log_every=0)
    torch.save({"params": [p.detach().clone() for p in tr.model.parameters()],
                "M": tr.engine.M.clone(), "early_grams": tr.engine.early_grams},
               os.path.join(out_dir, f"r{rank}.pt"))
    D.monitored_barrier(30)
    dist.destroy_process_group()


@pytest.mark.parametrize("topo,rule", [("sharded", "trimmed_mean"), ("allgather", "median"),
                                       ("sharded", "krum")])
def test_nnm_distributed_equals_virtual(tmp_path, topo, rule):
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    world, f, steps = 4, 1, 5
    mp.spawn(_worker, args=(world, _free_port(), rule, topo, f, steps, str(tmp_path)),
             nprocs=world, join=True)
    res = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True)
           for r in range(world)]
    tr = ConsensusTrainer(_nnm_cfg(rule, topo, world, f, steps),
                          info=DistInfo(0, 1, 0, torch.device("cpu"), "none"))
    tr.fit(steps, log_every=0)
    single = [p.detach().clone() for p in tr.model.parameters()]
    for r in range(world):
        assert res[r]["early_grams"] > 0                    # the Gram ran for this rule
        assert torch.equal(res[r]["M"], res[0]["M"])        # one M on every rank
        for a, b in zip(res[r]["params"], res[0]["params"]):
            assert torch.equal(a, b)
        for a, b in zip(res[r]["params"], single):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    M = res[0]["M"]
    assert bool(((M > 0).sum(1) == world - f).all())
