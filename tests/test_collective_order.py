"""Every rank issues the same sequence of collectives (CPU, gloo, world 2 and 4).

A rank whose sequence diverges -- one collective more, another size, another order -- leaves the
others waiting in a collective that never completes. Each spawned rank records
``(op, numel, dtype)`` of every collective it issues (``late_params.record_collectives``: the
five communication calls the engine uses plus ``barrier``; send/recv batches without peer ids,
which differ by design) over four steps of every topology, and all logs must equal rank 0's.
"""
import json
import os

import pytest
import torch.multiprocessing as mp

import late_params as LP
from test_dist_gloo import _cfg, _free_port

STEPS = 4
# (id, topology, rule, gossip graph, force early Gram, log + checkpoints)
CASES = [
    ("sharded-krum-prefetch-eager", "sharded", "krum", None, True, False),
    ("sharded-median", "sharded", "median", None, False, False),
    ("allgather-multi_krum", "allgather", "multi_krum", None, False, False),
    ("allreduce-mean", "allreduce", "mean", None, False, False),
    ("gossip-ring", "gossip", "mean", "ring", False, False),
    ("gossip-exp", "gossip", "mean", "exp", False, False),
    ("gossip_async-ring", "gossip_async", "mean", "ring", False, False),
    ("gossip_async-exp", "gossip_async", "mean", "exp", False, False),
    ("sharded-krum-log-ckpt", "sharded", "krum", None, False, True),
]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from consensusml_amd.parallel import dist as D
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    D._INFO = None
    info = D.init_distributed("gloo", timeout_s=60)
    calls = LP.record_collectives(dist)
    logs = {}
    for cid, topo, rule, graph, eager, log_ckpt in CASES:
        cfg = _cfg(rule, topo, 1, 0, STEPS)
        cfg.topology.param_prefetch = True
        if graph:
            cfg.topology.gossip_graph = graph
        if log_ckpt:
            cfg.log_path = os.path.join(out_dir, cid + ".jsonl")
            cfg.ckpt_dir = os.path.join(out_dir, cid + "_ckpt")
            cfg.ckpt_every = 2
        del calls[:]
        tr = ConsensusTrainer(cfg, info=info)     # (the initial parameter broadcast included)
        tr.engine._gram_eager = eager
        tr.fit(STEPS, log_every=1 if log_ckpt else 0)
        tr.close()
        logs[cid] = {"calls": list(calls), "prefetch": tr.engine.param_prefetch,
                     "early_grams": tr.engine.early_grams}
    with open(os.path.join(out_dir, f"order_r{rank}.json"), "w") as fh:
        json.dump(logs, fh)
    D.monitored_barrier(60)
    dist.destroy_process_group()


@pytest.fixture(scope="module", params=[2, 4], ids=["world2", "world4"])
def logs(request, tmp_path_factory):
    world = request.param
    d = tmp_path_factory.mktemp(f"order_w{world}")
    mp.spawn(_worker, args=(world, _free_port(), str(d)), nprocs=world, join=True)
    out = []
    for r in range(world):
        with open(d / f"order_r{r}.json") as fh:
            out.append(json.load(fh))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_collective_sequence_identical_on_every_rank(logs, case):
    cid, topo, rule, graph, eager, log_ckpt = case
    ref = logs[0][cid]["calls"]
    ops = {c[0] for c in ref}
    for r, lg in enumerate(logs):
        calls = lg[cid]["calls"]
        assert calls, f"rank {r} recorded no collective"
        if calls != ref:
            k = next((i for i, (a, b) in enumerate(zip(calls, ref)) if a != b),
                     min(len(calls), len(ref)))
            pytest.fail(f"rank {r} diverges from rank 0 at call {k} of {len(calls)} / "
                        f"{len(ref)}: {calls[k:k + 3]} vs {ref[k:k + 3]}")
    # the case ran what it names
    assert "broadcast" in ops
    if topo == "sharded":
        assert {"all_to_all_single", "all_gather_into_tensor"} <= ops
        assert logs[0][cid]["prefetch"]
    if topo == "allgather":
        assert "all_gather_into_tensor" in ops
    if topo == "allreduce" or rule == "krum":
        assert "all_reduce" in ops              # gradients / the Gram
    if topo.startswith("gossip"):
        assert "batch_isend_irecv" in ops
    if eager:
        assert logs[0][cid]["early_grams"] > 0
    if log_ckpt:
        assert "barrier" in ops                 # the checkpoint's barriers
        plain = logs[0]["sharded-krum-prefetch-eager"]["calls"]
        n_ar = lambda cs: sum(c[0] == "all_reduce" for c in cs)
        assert n_ar(ref) > n_ar(plain)          # the statistics all-reduces
