"""Test helpers for the multi-rank engine (not collected: no ``test_`` prefix).

``arm_late_params`` -- every parameter bucket "arrives" at the last legal moment. The engine
does not wait for the parameter exchange at the end of ``step()``; the next forward waits per
unit through forward pre-hooks (``ConsensusEngine._setup_prefetch``). That is only correct if no
parameter is read before the hook of the unit that owns it has fired. A real race would fail
only when a collective happens to be slow, so the worst case is simulated instead: each bucket
of the flat parameter buffer is filled with NaN and a work-like object whose ``wait()`` restores
it is put where the engine keeps its in-flight work. Parameters are views of the flat buffer,
so a read before the owning wait sees NaN, a read after it sees the true value (the restore is
an ordinary copy on the current stream). It needs only the hooks, no second rank.

``record_collectives`` -- logs every collective a rank issues, for comparing the sequences of
the ranks of one run.
"""
import os

import torch


class _LateWork:
    """Stands in for a bucket's in-flight exchange: ``wait()`` lands it (once)."""

    def __init__(self, dst, saved, index, log):
        self.dst, self.saved, self.index, self.log = dst, saved, index, log

    def wait(self):
        if self.saved is not None:
            self.dst.copy_(self.saved)      # on the current stream, like a collective's wait
            self.saved = None
            self.log.append(self.index)


def arm_late_params(engine):
    """Poison every bucket of ``engine``'s flat parameters and leave the restore to whoever
    waits for that bucket. Returns the wait log (bucket indices, in the order waited for)."""
    engine.wait_params()                    # real work (all-gather / gossip mix events) first
    log = []
    fp = engine.flat.flat_param
    with torch.no_grad():
        for b in engine.flat.buckets:
            dst = fp[b.offset:b.offset + b.length]
            saved = dst.clone()
            dst.fill_(float("nan"))
            engine._ag_works[b.index] = _LateWork(dst, saved, b.index, log)
    return log


def poisoned(t):
    return bool(torch.isnan(t.detach()).any())


# ------------------------------------------------------------------------- late-arrival runs
def make_cfg(model, dtype, backend, topo="sharded", V=1, bucket_mb=0.002, prefetch=True,
             **model_kw):
    from consensusml_amd import TrainConfig
    cfg = TrainConfig()
    cfg.model.name = model
    cfg.dtype = dtype
    cfg.backend = backend
    cfg.virtual_workers = V
    cfg.topology.bucket_mb = bucket_mb
    cfg.topology.param_prefetch = prefetch
    if topo == "gossip_async":
        cfg.topology.kind = "gossip"
        cfg.topology.gossip_async = True
        cfg.agg.rule = "mean"
    else:
        cfg.topology.kind = topo
        cfg.agg.rule = "krum"
    cfg.agg.f = 0
    cfg.optim.lr = 0.05
    if model == "mlp":
        cfg.model.extra = {"classes": 2}
        cfg.batch_per_worker = 16
    elif model in ("resnet_tiny", "resnet50"):
        cfg.model.num_classes = 10
        cfg.model.image_size = model_kw.get("image", 32)
        cfg.batch_per_worker = model_kw.get("batch", 4)
    else:
        cfg.model.seq_len = model_kw.get("seq", 16)
        cfg.batch_per_worker = model_kw.get("batch", 2)
    return cfg


def _state(tr, loss):
    e = tr.engine
    e.wait_params()
    if e.device.type == "cuda":
        torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.detach().cpu().clone()
    return {"loss": cpu(loss), "params": [cpu(p) for p in tr.model.parameters()],
            "buffers": [cpu(b) for b in tr.model.buffers()],
            "master": cpu(e.master), "s1": cpu(e.s1), "s2": cpu(e.s2)}


def _conv_bucket_span(engine):
    """Number of buckets holding the layer1-4 conv weights of a ResNet (0 for other models)."""
    fl = engine.flat
    pid = {id(p): i for i, p in enumerate(fl.params)}
    return len({fl.bucket_of[pid[id(p)]] for n, p in fl.model.named_parameters()
                if n.startswith("layer") and p.dim() == 4})


def run_late_case(info, cfg_fn, mode="train", tmp=None):
    """One late-arrival case in an initialised 1-rank loopback group. Three trainers from the
    same seed: ``late`` (armed after two steps, the waits left to the hooks), ``control`` (armed
    and waited for at once: version counters and weight-derived caches as in ``late``) and
    ``plain`` (prefetch off, never armed). ``mode``: what runs armed -- a train step, an
    evaluate() or a save()."""
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    out = {}
    for name in ("control", "late", "plain"):
        cfg = cfg_fn(prefetch=name != "plain")
        tr = ConsensusTrainer(cfg, info=info)
        e = tr.engine
        for _ in range(2):                  # the hooks learn which units are called
            tr.train_step()
        res = {"prefetch": e.param_prefetch, "buckets": len(e.flat.buckets),
               "conv_span": _conv_bucket_span(e), "learned": getattr(e, "_learned", None)}
        log = None
        if name != "plain":
            log = arm_late_params(e)
            if name == "control":
                e.wait_params()
        loss = extra = None
        if mode == "train":
            loss = tr.train_step()
        elif mode == "evaluate":
            extra = tr.evaluate(batches=2)
        else:
            d = tr.save(os.path.join(tmp, name))
            extra = torch.load(os.path.join(d, "rank0.pt"), map_location="cpu",
                               weights_only=True)
        res.update(_state(tr, loss))
        res["log"] = log
        res["extra"] = extra
        tr.close()
        out[name] = res
    return out


def same_bits(a, b):
    """Bitwise equality of two (nested) results; NaN equals NaN of the same bits."""
    if torch.is_tensor(a):
        if not torch.is_tensor(b) or a.shape != b.shape or a.dtype != b.dtype:
            return False
        if not a.dtype.is_floating_point:
            return torch.equal(a, b)
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k])
                                                                    for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and \
            all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (a != a and b != b)
    return a == b


def any_nan(x):
    if torch.is_tensor(x):
        return x.dtype.is_floating_point and bool(torch.isnan(x).any())
    if isinstance(x, dict):
        return any(any_nan(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return any(any_nan(v) for v in x)
    return isinstance(x, float) and x != x


STATE_KEYS = ("params", "buffers", "master", "s1", "s2")


def check_late_case(res, mode="train", resnet=False):
    """The assertions of one late-arrival case (``run_late_case``'s result)."""
    c, l, p = res["control"], res["late"], res["plain"]
    assert c["prefetch"] and l["prefetch"] and not p["prefetch"]   # not vacuous
    assert l["learned"], "the hooks never learned: every wait would be up front"
    nb = l["buckets"]
    assert nb >= 4, nb
    if resnet:
        assert l["conv_span"] >= 2, l["conv_span"]
    # every bucket waited for exactly once, by the hooks / the public entry point itself
    assert sorted(l["log"]) == list(range(nb)), l["log"]
    assert sorted(c["log"]) == list(range(nb)), c["log"]
    if mode == "train":
        assert torch.isfinite(l["loss"]).all(), l["loss"]
        assert same_bits(l["loss"], c["loss"]), (l["loss"], c["loss"])
        assert same_bits(p["loss"], c["loss"]), (p["loss"], c["loss"])
    for k in STATE_KEYS:
        assert not any_nan(l[k]), k
        assert same_bits(l[k], c[k]), f"late != control: {k}"
        assert same_bits(p[k], c[k]), f"plain != control: {k} (the harness is not neutral)"
    if mode == "evaluate":
        assert l["extra"]["loss"] == l["extra"]["loss"], l["extra"]
        assert l["extra"] == c["extra"] == p["extra"], (l["extra"], c["extra"], p["extra"])
    if mode == "save":
        for part in ("engine", "buffers", "gens"):
            assert not any_nan(l["extra"][part]), part
            assert same_bits(l["extra"][part], c["extra"][part]), part
            assert same_bits(p["extra"][part], c["extra"][part]), part


# ------------------------------------------------------------------------- collective order
COLLECTIVES = ("all_to_all_single", "all_gather_into_tensor", "all_reduce", "broadcast",
               "batch_isend_irecv", "barrier")


def record_collectives(dist):
    """Wrap ``dist``'s collectives; returns the list that receives one ``(op, numel, dtype)``
    per call. ``batch_isend_irecv`` logs its sorted ``(isend | irecv, numel)`` list, no peers
    (those differ between ranks by design); ``barrier`` logs no size."""
    calls = []

    def describe(name, a, k):
        if name == "batch_isend_irecv":
            ops = a[0] if a else k["p2p_op_list"]
            return (name, sorted((o.op.__name__, o.tensor.numel()) for o in ops), "")
        if name == "barrier":
            return (name, 0, "")
        t = a[0] if a else next(iter(k.values()))
        return (name, t.numel(), str(t.dtype))

    for name in COLLECTIVES:
        orig = getattr(dist, name)

        def wrap(*a, _o=orig, _n=name, **k):
            calls.append(describe(_n, a, k))
            return _o(*a, **k)
        setattr(dist, name, wrap)
    return calls
