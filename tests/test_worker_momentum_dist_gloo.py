"""``optim.worker_momentum`` across ranks (gloo, CPU): with overlap on, each bucket's momentum
runs in its flush, ahead of that bucket's collective; with overlap off, one launch covers the
whole row in step(). The momentum is elementwise, so the two must agree bit for bit, the
replicas must stay identical, and the sequence of collectives is unchanged."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_dist_gloo import _cfg, _free_port

STEPS = 3


def _wm_cfg(world, overlap):
    # Krum needs n > 2f: f = 1 at four workers, f = 0 at two
    cfg = _cfg("krum", "sharded", 1, 1 if world > 2 else 0, STEPS)
    cfg.topology.bucket_mb = 0.0004     # ~100 elements: at least three buckets for the MLP
    cfg.optim.momentum = 0.9
    cfg.optim.worker_momentum = True
    cfg.topology.overlap = overlap
    return cfg


def _worker(rank, world, port, overlap, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.parallel import dist as D
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    D._INFO = None
    info = D.init_distributed("gloo")
    tr = ConsensusTrainer(_wm_cfg(world, overlap), info=info)
    e = tr.engine
    shapes = []
    real = K.worker_momentum

    def spy(rows, mom, beta):
        shapes.append(tuple(rows.shape))
        real(rows, mom, beta)
    K.worker_momentum = spy
    tr.fit(STEPS, log_every=0)
    K.worker_momentum = real
    torch.save({"params": [p.detach().clone() for p in tr.model.parameters()],
                "wm": e.wm.clone(), "overlap": e.overlap, "shapes": shapes,
                "buckets": [b.length for b in e.flat.buckets], "s1": e.s1 is None},
               os.path.join(out_dir, f"r{rank}.pt"))
    D.monitored_barrier(30)
    dist.destroy_process_group()


def _run(world, overlap, tmp):
    os.makedirs(tmp, exist_ok=True)
    mp.spawn(_worker, args=(world, _free_port(), overlap, str(tmp)), nprocs=world, join=True)
    return [torch.load(os.path.join(tmp, f"r{r}.pt"), weights_only=True) for r in range(world)]


@pytest.mark.parametrize("world", [2, 4])
def test_worker_momentum_overlap_bit_identical(tmp_path, world):
    on = _run(world, True, tmp_path / "on")
    off = _run(world, False, tmp_path / "off")
    nb = len(on[0]["buckets"])
    assert nb >= 3
    for r in range(world):
        assert on[r]["overlap"] and not off[r]["overlap"] and on[r]["s1"] and off[r]["s1"]
        # one [1, L_b] launch per bucket and step against one [1, D] launch per step
        assert sorted(on[r]["shapes"]) == sorted([(1, L) for L in on[r]["buckets"]] * STEPS)
        assert off[r]["shapes"] == [(1, sum(off[r]["buckets"]))] * STEPS
        assert on[r]["wm"].abs().sum() > 0
        assert torch.equal(on[r]["wm"], off[r]["wm"])
        for a, b in zip(on[r]["params"], on[0]["params"]):      # replicas identical
            assert torch.equal(a, b)
        for a, b in zip(on[r]["params"], off[r]["params"]):     # bucket-wise == whole row
            assert torch.equal(a, b)
    # the workers differ (their own data), so do their states
    assert not torch.equal(on[0]["wm"], on[1]["wm"])
