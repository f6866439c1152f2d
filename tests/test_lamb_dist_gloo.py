"""``optim.name=lamb`` across ranks (gloo, CPU), sharded topology: two ranks x 1 worker end at the
masters and ``lamb_stats`` of one rank x 2 virtual workers on the same global batch. What joins the
ranks' halves of every tensor is the one all-reduce of the fp64 [T, 2] per-tensor sums."""
import os

import torch
import torch.multiprocessing as mp

from test_dist_gloo import _cfg, _free_port

STEPS, WORLD = 3, 2
RTOL, ATOL = 2e-5, 2e-6      # tests/test_lamb_cpu.py


def _lamb_cfg(V):
    cfg = _cfg("mean", "sharded", V, 0, STEPS)
    cfg.optim.name, cfg.optim.lr, cfg.optim.weight_decay = "lamb", 0.01, 0.01
    # the ranks sum the workers' gradients in another order than one rank does: eps far above
    # that 1e-7 keeps the first step's x / (|x| + eps) from turning a rounding into a sign
    cfg.optim.eps = 1e-3
    return cfg


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from consensusml_amd.parallel import dist as D
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    D._INFO = None
    tr = ConsensusTrainer(_lamb_cfg(1), info=D.init_distributed("gloo", timeout_s=60))
    for _ in range(STEPS):
        tr.train_step()
    tr.engine.wait_params()
    torch.save({"params": [p.detach().clone() for p in tr.model.parameters()],
                "stats": tr.engine.lamb_stats.clone()}, os.path.join(out_dir, f"r{rank}.pt"))
    tr.close()
    D.monitored_barrier(60)
    dist.destroy_process_group()


def test_lamb_two_ranks_equal_one_rank(tmp_path):
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    ranks = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(WORLD)]
    tr = ConsensusTrainer(_lamb_cfg(WORLD), info=DistInfo(0, 1, 0, torch.device("cpu"), "none"))
    for _ in range(STEPS):
        tr.train_step()
    single = [p.detach().clone() for p in tr.model.parameters()]
    stats = tr.engine.lamb_stats
    for r in ranks:
        assert torch.equal(r["stats"], ranks[0]["stats"])      # the same bits on every rank
        assert float(r["stats"][:, 3].sum()) == 0.0
        assert [float(q) == 1.0 for q in r["stats"][:, 2]] == [p.dim() < 2 for p in single]
        torch.testing.assert_close(r["stats"][:, :3], stats[:, :3], rtol=RTOL, atol=ATOL)
        for a, b in zip(r["params"], single):
            torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)
    tr.close()
