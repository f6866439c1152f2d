"""MeaMed and Phocas across ranks (gloo, CPU): R ranks x 1 worker give the parameters of 1 rank x
R virtual workers on the same per-worker data, in the sharded and the allgather topology, and
with ``agg.pre=nnm`` every rank selects around the same mixed rows."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_dist_gloo import _cfg, _free_port


def _near_cfg(rule, topo, V, f, steps, pre):
    cfg = _cfg(rule, topo, V, f, steps)
    cfg.agg.pre = pre
    return cfg


def _worker(rank, world, port, rule, topo, f, steps, pre, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from consensusml_amd.parallel import dist as D
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    D._INFO = None
    info = D.init_distributed("gloo")
    tr = ConsensusTrainer(_near_cfg(rule, topo, 1, f, steps, pre), info=info)
    tr.engine._gram_eager = True
    tr.fit(steps, log_every=0)
    torch.save({"params": [p.detach().clone() for p in tr.model.parameters()],
                "early_grams": tr.engine.early_grams}, os.path.join(out_dir, f"r{rank}.pt"))
    D.monitored_barrier(30)
    dist.destroy_process_group()


@pytest.mark.parametrize("world,topo,rule,f,pre", [
    (2, "sharded", "meamed", 0, "none"),
    (2, "allgather", "phocas", 0, "none"),
    (4, "sharded", "phocas", 1, "none"),
    (4, "allgather", "meamed", 1, "none"),
    (4, "sharded", "meamed", 1, "nnm"),
])
def test_near_rules_distributed_equal_virtual(tmp_path, world, topo, rule, f, pre):
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    steps = 5
    mp.spawn(_worker, args=(world, _free_port(), rule, topo, f, steps, pre, str(tmp_path)),
             nprocs=world, join=True)
    res = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True)
           for r in range(world)]
    tr = ConsensusTrainer(_near_cfg(rule, topo, world, f, steps, pre),
                          info=DistInfo(0, 1, 0, torch.device("cpu"), "none"))
    tr.fit(steps, log_every=0)
    single = [p.detach().clone() for p in tr.model.parameters()]
    for r in range(world):
        assert (res[r]["early_grams"] > 0) == (pre == "nnm")    # the Gram runs for the mix only
        for a, b in zip(res[r]["params"], res[0]["params"]):
            assert torch.equal(a, b)                            # identical replicas
        for a, b in zip(res[r]["params"], single):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
