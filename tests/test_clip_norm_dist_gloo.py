"""``optim.clip_norm`` across ranks (gloo, CPU): R ranks x 1 worker under an active clip give
identical replicas and the parameters of 1 rank x R virtual workers; every rank issues the same
collectives, and against the unclipped run exactly one more all-reduce per step in the sharded
topology (the fp64 squared norm) and none in allgather (every rank holds the full aggregate)."""
import json
import os

import pytest
import torch
import torch.multiprocessing as mp

import late_params as LP
from test_dist_gloo import _cfg, _free_port

STEPS = 4
CLIP = 0.05          # the MLP's aggregate norm is several times this: every step is clipped


def _clip_cfg(topo, V, clip):
    cfg = _cfg("median", topo, V, 1, STEPS)
    cfg.optim.clip_norm = clip
    return cfg


def _worker(rank, world, port, topo, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from consensusml_amd.parallel import dist as D
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    D._INFO = None
    info = D.init_distributed("gloo", timeout_s=60)
    calls = LP.record_collectives(dist)
    out = {}
    for name, clip in (("off", 0.0), ("on", CLIP)):
        del calls[:]
        tr = ConsensusTrainer(_clip_cfg(topo, 1, clip), info=info)
        coefs = []
        for _ in range(STEPS):
            tr.train_step()
            if clip:
                coefs.append(tr.engine.grad_stats.tolist())
        tr.engine.wait_params()
        out[name] = {"calls": list(calls), "stats": coefs}
        if clip:
            torch.save([p.detach().clone() for p in tr.model.parameters()],
                       os.path.join(out_dir, f"r{rank}.pt"))
        tr.close()
    with open(os.path.join(out_dir, f"calls_r{rank}.json"), "w") as fh:
        json.dump(out, fh)
    D.monitored_barrier(60)
    dist.destroy_process_group()


@pytest.mark.parametrize("world,topo", [(2, "sharded"), (2, "allgather"), (4, "sharded"),
                                        (4, "allgather")])
def test_clip_norm_distributed_equals_virtual(tmp_path, world, topo):
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    mp.spawn(_worker, args=(world, _free_port(), topo, str(tmp_path)), nprocs=world, join=True)
    params = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True)
              for r in range(world)]
    logs = []
    for r in range(world):
        with open(tmp_path / f"calls_r{r}.json") as fh:
            logs.append(json.load(fh))
    tr = ConsensusTrainer(_clip_cfg(topo, world, CLIP),
                          info=DistInfo(0, 1, 0, torch.device("cpu"), "none"))
    single_stats = []
    for _ in range(STEPS):
        tr.train_step()
        single_stats.append(tr.engine.grad_stats.tolist())
    single = [p.detach().clone() for p in tr.model.parameters()]
    for r in range(world):
        for a, b in zip(params[r], params[0]):
            assert torch.equal(a, b)                                    # identical replicas
        for a, b in zip(params[r], single):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)      # (test_meamed_dist_gloo's)
        st = logs[r]["on"]["stats"]
        assert st == logs[0]["on"]["stats"]          # the same norm and coefficient on every rank
        assert all(s[1] < 1.0 and s[2] == 0.0 for s in st)              # every step clipped
        for s, t in zip(st, single_stats):
            assert s[0] == pytest.approx(t[0], rel=1e-5)
    # collectives: the same sequence on every rank
    for name in ("off", "on"):
        for r in range(world):
            assert logs[r][name]["calls"] == logs[0][name]["calls"], (name, r)
    off, on = logs[0]["off"]["calls"], logs[0]["on"]["calls"]
    extra = ["all_reduce", 1, "torch.float64"]
    n_extra = sum(c == extra for c in on) - sum(c == extra for c in off)
    assert n_extra == (STEPS if topo == "sharded" else 0)
    rest = list(on)
    for _ in range(n_extra):
        rest.remove(extra)
    assert rest == off                       # nothing else moved: gathers and prefetch unchanged
    if topo == "sharded":
        # one per step: between two of them lies one step's exchange and parameter all-gather
        idx = [i for i, c in enumerate(on) if c == extra]
        assert all(b - a > 1 for a, b in zip(idx, idx[1:]))
