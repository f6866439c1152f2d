"""No forward may read a parameter before its exchange has landed.

The sharded topology's parameter all-gather and delayed gossip's mix are not waited for at the
end of ``step()``: the next forward waits per unit in forward pre-hooks. These tests let every
bucket arrive at the last legal moment (``late_params.arm_late_params``: NaN until the owning
wait) on a 1-rank loopback group and require bit-identical results to a run that waited for
everything up front, and to a run that never overlapped at all.

CPU cases: fp32 on gloo. The GPU cases (bf16, RCCL loopback) run the HIP kernels on the same
harness; NaN weights are ordinary data to every kernel.
"""
import os

import pytest
import torch
import torch.multiprocessing as mp

import late_params as LP

# (id, model, mode, model kwargs)
CPU_CASES = [
    ("mlp", "mlp", "train", dict(bucket_mb=0.0002)),
    ("resnet_tiny", "resnet_tiny", "train", dict(image=32, batch=4)),
    ("bert_tiny", "bert_tiny", "train", dict(seq=16, batch=2)),
    ("llama_tiny", "llama_tiny", "train", dict(seq=16, batch=2)),
    ("resnet_tiny-evaluate", "resnet_tiny", "evaluate", dict(image=32, batch=4)),
    ("bert_tiny-evaluate", "bert_tiny", "evaluate", dict(seq=16, batch=2)),
    ("mlp-save", "mlp", "save", dict(bucket_mb=0.0002)),
    ("resnet_tiny-save", "resnet_tiny", "save", dict(image=32, batch=4)),
]
# (id, model, topology, V, model kwargs)
GPU_CASES = [
    ("resnet_tiny", "resnet_tiny", "sharded", 1, dict(image=32, batch=4)),
    ("resnet50", "resnet50", "sharded", 1, dict(image=64, batch=2, bucket_mb=4.0)),
    ("bert_tiny-V1", "bert_tiny", "sharded", 1, dict(seq=16, batch=2)),
    ("bert_tiny-V2", "bert_tiny", "sharded", 2, dict(seq=16, batch=2)),
    ("llama_tiny", "llama_tiny", "sharded", 1, dict(seq=64, batch=2)),
    ("bert_tiny-gossip", "bert_tiny", "gossip_async", 1, dict(seq=16, batch=2)),
    ("llama_tiny-gossip", "llama_tiny", "gossip_async", 1, dict(seq=64, batch=2)),
]


def _init(backend, device):
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    from consensusml_amd.parallel import dist as D
    D._INFO = None
    info = D.init_distributed(backend, device=device, loopback=True)
    assert info.loopback and info.distributed
    return info


def _spy_case(info, cfg, gpu):
    """Wrap ops.conv.prefetch_wlayouts for two unarmed steps and one armed step: how often it
    was entered, what it returned and how many of its weights were still poisoned."""
    from consensusml_amd.ops import conv as fconv
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    calls = []
    orig = fconv.prefetch_wlayouts

    def spy(ws):
        ws = list(ws)
        bad = sum(LP.poisoned(w) for w in ws)
        ret = orig(ws)
        calls.append({"weights": len(ws), "poisoned": bad, "ret": bool(ret)})
        return ret
    fconv.prefetch_wlayouts = spy
    try:
        tr = ConsensusTrainer(cfg, info=info)
        tr.train_step()
        tr.train_step()
        before = list(calls)
        del calls[:]
        log = LP.arm_late_params(tr.engine)
        loss = tr.train_step()
        tr.engine.wait_params()
        armed = list(calls)
        del calls[:]
        tr.train_step()                     # nothing pending again (one rank: no all-gather)
        after = list(calls)
        res = {"before": before, "armed": armed, "after": after, "log": log,
               "loss": float(loss), "buckets": len(tr.engine.flat.buckets),
               "pending_after": len(tr.engine._ag_works),
               "prefetch": tr.engine.param_prefetch}
        tr.close()
    finally:
        fconv.prefetch_wlayouts = orig
    return res


def _cpu_worker(_rank, out_dir):
    import torch.distributed as dist
    info = _init("gloo", "cpu")
    for cid, model, mode, kw in CPU_CASES:
        fn = lambda prefetch, m=model, k=kw: LP.make_cfg(m, "fp32", "gloo", prefetch=prefetch, **k)
        res = LP.run_late_case(info, fn, mode, tmp=os.path.join(out_dir, "ckpt_" + cid))
        torch.save(res, os.path.join(out_dir, cid + ".pt"))
    spy = _spy_case(info, LP.make_cfg("resnet_tiny", "fp32", "gloo", image=32, batch=4), False)
    torch.save(spy, os.path.join(out_dir, "spy.pt"))
    dist.destroy_process_group()


def _gpu_worker(_rank, out_dir):
    import torch.distributed as dist
    info = _init("nccl", "cuda:0")
    # MIOpen's default weight-gradient algorithms are not run-to-run reproducible at the resnet50
    # shapes (two identical trainers with no overlap at all already differ in the last bits), so
    # a bitwise comparison needs its deterministic mode -- in all three runs of every case
    torch.backends.cudnn.deterministic = True
    for cid, model, topo, V, kw in GPU_CASES:
        fn = lambda prefetch, m=model, t=topo, v=V, k=kw: LP.make_cfg(
            m, "bf16", "nccl", topo=t, V=v, prefetch=prefetch, **k)
        res = LP.run_late_case(info, fn, "train")
        torch.save(res, os.path.join(out_dir, cid + ".pt"))
    spy = _spy_case(info, LP.make_cfg("resnet50", "bf16", "nccl", image=64, batch=2,
                                      bucket_mb=4.0), True)
    torch.save(spy, os.path.join(out_dir, "spy.pt"))
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def cpu_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("late_cpu")
    mp.spawn(_cpu_worker, args=(str(d),), nprocs=1, join=True)
    return d


@pytest.fixture(scope="module")
def gpu_results(cuda, tmp_path_factory):
    d = tmp_path_factory.mktemp("late_gpu")
    mp.spawn(_gpu_worker, args=(str(d),), nprocs=1, join=True)
    return d


def _load(d, cid):
    return torch.load(os.path.join(d, cid + ".pt"), weights_only=True)


@pytest.mark.parametrize("cid,model,mode", [(c[0], c[1], c[2]) for c in CPU_CASES],
                         ids=[c[0] for c in CPU_CASES])
def test_late_params_cpu(cpu_results, cid, model, mode):
    """fp32 / gloo: an armed train step, evaluate() or save() equals the control bit for bit."""
    LP.check_late_case(_load(cpu_results, cid), mode, resnet=model.startswith("resnet"))


def test_layout_prefetch_never_sees_pending_weights_cpu(cpu_results):
    """ResNet.forward batches every block's conv weight layouts before layer1 is called, i.e.
    before any layer's pre-hook has waited: it must not do so while those weights are pending.
    (On the CPU prefetch_wlayouts filters on is_cuda and would read nothing; the spy looks at the
    weights it is handed.)"""
    s = _load(cpu_results, "spy")
    assert s["prefetch"] and s["buckets"] >= 4
    assert len(s["before"]) == 2 and all(c["poisoned"] == 0 for c in s["before"]), s["before"]
    assert all(c["weights"] == 8 for c in s["before"]), s["before"]   # the spy sees the batch
    assert sum(c["poisoned"] for c in s["armed"]) == 0, s["armed"]
    assert sorted(s["log"]) == list(range(s["buckets"]))
    assert s["loss"] == s["loss"]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,model", [(c[0], c[1]) for c in GPU_CASES],
                         ids=[c[0] for c in GPU_CASES])
def test_late_params_gpu(gpu_results, cid, model):
    """bf16 / RCCL loopback on the HIP kernels: sharded + Krum for every model (bert_tiny also
    with two batched virtual workers), delayed gossip for the transformers."""
    LP.check_late_case(_load(gpu_results, cid), "train", resnet=model.startswith("resnet"))


@pytest.mark.gpu
def test_layout_prefetch_batched_when_nothing_pending_gpu(gpu_results):
    """resnet50, sharded on a 1-rank RCCL group (the 1-GPU headline set-up: prefetch on, nothing
    ever in flight): every training forward still makes its one batched layout launch; only the
    forward of the armed step, with buckets pending, leaves the layouts to the convs."""
    s = _load(gpu_results, "spy")
    assert s["prefetch"] and s["pending_after"] == 0
    for c in s["before"] + s["after"]:
        assert c["ret"] and c["poisoned"] == 0 and c["weights"] == 32, c
    assert len(s["before"]) == 2 and len(s["after"]) == 1
    assert s["armed"] == [], s["armed"]
    assert s["loss"] == s["loss"]
