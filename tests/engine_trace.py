"""What ``ConsensusEngine`` launches, and in which order, must not move (not collected: no
``test_`` prefix).

``run_world1`` / ``run_world2`` train a thin 2-layer MLP (4 -> 32 -> 2: four buckets) for three
steps per case, the last one with ``record_stats``, and log one record per call of

* the ``ops.kernels`` functions the engine drives (``K_FUNCS``) and ``apply_faults``: the
  arguments bound to the function's signature, those equal to their default left out, so a
  default passed explicitly and one omitted give the same record. Calls nested inside a logged
  call (``agg_update_multi``'s per-segment ``agg_update`` on CPU) are not logged;
* the native methods the engine calls directly (``LIB_FUNCS``), positional and keyword;
* every collective (``late_params.record_collectives``), interleaved where it was issued.

A tensor argument is logged as ``[engine buffer, element offset, shape, stride, dtype]``, its
``data_ptr`` resolved against the engine's named buffers (``_buffers``), or as ``["other", shape,
dtype]``; ``OptArgs`` and the fault config as dicts.

Cases (``world1_cases``, CPU and GPU, one process, no process group): sharded and allgather x
{mean, median, meamed, bulyan, krum, centered_clip, nnm + median, nnm + krum} at n = 7, f = 1 x
``optim.clip_norm`` 0 and 1e-3 (which clips: asserted); sharded Krum over 18 buckets (no fused
launch); allreduce and gossip (V = 1, 3) with and without clipping; worker momentum under a
Gaussian fault. ``WORLD2_CASES`` (CPU, two gloo ranks, both logged): sharded Krum with the
parameter prefetch, sharded median with clipping, sharded centered clipping, allgather
Multi-Krum; every bucket's Gram is taken in its hook (``_gram_eager``), so the order does not
depend on when an exchange lands.

``tests/golden/engine_trace_cpu.json`` and ``tests/golden/engine_trace_gpu.json`` (+ the final
``master`` and ``flat_param`` of every GPU case in ``engine_trace_gpu.pt``) hold what the commit
BEFORE the engine's rule ladders were folded into ``ops.kernels.rule_combine`` produced, the GPU
files on an MI355X:

    python tests/engine_trace.py cpu tests/golden/engine_trace_cpu.json
    python tests/engine_trace.py gpu tests/golden/engine_trace_gpu.json tests/golden/engine_trace_gpu.pt

run in a checkout of that commit (7f85c02, with this file copied in).
``test_engine_trace_cpu.py`` / ``test_engine_trace_gpu.py`` compare record for record (and the
tensors bit for bit).

File format: ``atoms`` is the table of distinct ``[key, value]`` pairs, a record the list of its
pairs' indices (``decode`` gives the dicts back).
"""
import contextlib
import dataclasses
import inspect
import json
import os
import sys

import torch

import late_params as LP

STEPS = 3
CLIP = 1e-3
K_FUNCS = ("agg_update", "agg_update_multi", "gram", "gram_center", "gram_sum", "robust_weights",
           "sq_norm", "clip_coef", "worker_momentum", "gossip_mix_k")
LIB_FUNCS = ("gram_partial", "gram_reduce_multi", "multi_copy")
RULES = [("mean", "none"), ("median", "none"), ("meamed", "none"), ("bulyan", "none"),
         ("krum", "none"), ("centered_clip", "none"), ("median", "nnm"), ("krum", "nnm")]
# (id, topology, rule, clip_norm, param_prefetch)
WORLD2_CASES = [("w2-sharded-krum-prefetch", "sharded", "krum", 0.0, True),
                ("w2-sharded-median-clip", "sharded", "median", CLIP, False),
                ("w2-sharded-centered_clip", "sharded", "centered_clip", 0.0, True),
                ("w2-allgather-multi_krum", "allgather", "multi_krum", 0.0, True)]


# --------------------------------------------------------------------------- cases
def make_cfg(dtype, topo, rule, V=7, f=1, pre="none", clip=0.0):
    from consensusml_amd import TrainConfig
    cfg = TrainConfig()
    cfg.dtype = dtype
    cfg.virtual_workers = V
    cfg.agg.rule = rule
    cfg.agg.f = f
    cfg.agg.pre = pre
    cfg.topology.kind = topo
    # buckets of 64 elements: [fc2.bias], [fc2.weight], [fc1.bias], [fc1.weight]
    cfg.topology.bucket_mb = 64 * (2 if dtype == "bf16" else 4) / 2 ** 20
    cfg.optim.lr = 0.1
    cfg.optim.clip_norm = clip
    cfg.batch_per_worker = 16
    cfg.model.in_features = 4
    cfg.model.hidden = 32
    cfg.model.extra = {"classes": 2}
    return cfg


def world1_cases(dtype):
    """(id, config, deep) of every one-process case; ``deep``: the 18-parameter model."""
    out = []
    for topo in ("sharded", "allgather"):
        for rule, pre in RULES:
            for clip in (0.0, CLIP):
                cid = f"{topo}-{rule}" + ("-nnm" if pre == "nnm" else "")
                out.append((cid + ("-clip" if clip else ""),
                            make_cfg(dtype, topo, rule, pre=pre, clip=clip), False))
    out.append(("sharded-krum-18buckets", make_cfg(dtype, "sharded", "krum"), True))
    for clip in (0.0, CLIP):
        tag = "-clip" if clip else ""
        out.append(("allreduce-mean" + tag, make_cfg(dtype, "allreduce", "mean", V=3, f=0,
                                                     clip=clip), False))
        for V in (1, 3):
            out.append((f"gossip-V{V}" + tag, make_cfg(dtype, "gossip", "mean", V=V, f=0,
                                                       clip=clip), False))
    cfg = make_cfg(dtype, "sharded", "median")
    cfg.optim.worker_momentum = True
    cfg.fault.kind = "gaussian"
    cfg.fault.ranks = [3]
    out.append(("sharded-median-worker_momentum-gaussian", cfg, False))
    return out


def _deep_task(device, dtype, seed):
    """Nine 8 x 8 linear layers: 18 parameters, one bucket each."""
    from consensusml_amd.models import Task
    torch.manual_seed(seed)
    layers = []
    for _ in range(8):
        layers += [torch.nn.Linear(8, 8), torch.nn.ReLU()]
    model = torch.nn.Sequential(*layers, torch.nn.Linear(8, 8)).to(device, dtype)

    def make(b, gen):
        x = torch.randn(b, 8, generator=gen, device=device)
        return x.to(dtype), x[:, :8].argmax(1)

    def loss(m, batch):
        return torch.nn.functional.cross_entropy(m(batch[0]).float(), batch[1])
    return Task("deep", model, make, loss)


# --------------------------------------------------------------------------- the recorder
def _buffers(e):
    """(name, tensor) of every persistent buffer of the engine (some appear during the run)."""
    named = [("flat_grad", e.flat.flat_grad), ("flat_param", e.flat.flat_param)]
    for name in ("master", "s1", "s2", "gout", "w", "w_clip", "sel", "M", "G", "Gb", "center",
                 "wm", "_send_buf", "scores", "sel_counts", "grad_stats", "_norm2", "_norm2_red",
                 "_clip_work"):
        named.append((name, getattr(e, name, None)))
    named += [(f"recv[{i}]", t) for i, t in enumerate(e.recv)]
    named += [(f"nb_bufs[{i}]", t) for i, t in enumerate(e.nb_bufs)]
    named += [(f"gram_ws[{i}]", hit[2]) for i, hit in sorted(e._gram_arg_cache.items()) if hit]
    return [(n, t) for n, t in named if t is not None and t.numel()]


class Tracer:
    def __init__(self, engine, collectives):
        self.e, self.coll, self.seen = engine, collectives, 0
        self.records, self.depth = [], 0

    def tensor(self, t):
        p = t.data_ptr()
        for name, buf in _buffers(self.e):
            lo = buf.data_ptr()
            if t.numel() and lo <= p < lo + buf.numel() * buf.element_size():
                return [name, (p - lo) // t.element_size(), list(t.shape), list(t.stride()),
                        str(t.dtype)]
        return ["other", list(t.shape), str(t.dtype)]

    def value(self, v):
        if torch.is_tensor(v):
            return self.tensor(v)
        if dataclasses.is_dataclass(v):
            return dataclasses.asdict(v)
        if isinstance(v, slice):
            return ["slice", v.start, v.stop]
        if isinstance(v, (list, tuple)):
            return [self.value(x) for x in v]
        if isinstance(v, dict):
            return {k: self.value(x) for k, x in v.items()}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"engine_trace: cannot log a {type(v).__name__}")

    def flush(self):
        for op, numel, dtype in self.coll[self.seen:]:
            self.records.append({"fn": "dist." + op, "numel": numel, "dtype": dtype})
        self.seen = len(self.coll)

    def wrap(self, name, orig, bind):
        sig = inspect.signature(orig) if bind else None

        def traced(*a, **k):
            if self.depth == 0:
                self.flush()
                rec = {"fn": name}
                if sig is None:
                    rec["args"] = self.value(a)
                    rec.update(self.value(k))
                else:
                    for key, v in sig.bind(*a, **k).arguments.items():
                        v, d = self.value(v), sig.parameters[key].default
                        if d is inspect.Parameter.empty or v != self.value(d):
                            rec[key] = v
                self.records.append(rec)
            self.depth += 1
            try:
                return orig(*a, **k)
            finally:
                self.depth -= 1
        return traced


class _Lib:
    """The native module with ``LIB_FUNCS`` traced (everything else passes through)."""

    def __init__(self, real, tracer):
        self._real, self._tracer, self._wrapped = real, tracer, {}

    def __getattr__(self, name):
        if name not in LIB_FUNCS:
            return getattr(self._real(), name)
        if name not in self._wrapped:
            self._wrapped[name] = self._tracer.wrap("lib." + name, getattr(self._real(), name),
                                                    bind=False)
        return self._wrapped[name]


@contextlib.contextmanager
def tracing(engine, collectives):
    """Log ``engine``'s launches (and the collectives that ``collectives`` receives)."""
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.parallel import engine as E
    tr = Tracer(engine, collectives)
    saved = [(K, n, getattr(K, n)) for n in K_FUNCS]
    saved += [(E, "apply_faults", E.apply_faults), (E, "lib", E.lib)]
    try:
        for mod, name, orig in saved[:-1]:
            setattr(mod, name, tr.wrap(name, orig, bind=True))
        proxy = _Lib(E.lib, tr)
        E.lib = lambda: proxy
        yield tr
        tr.flush()
    finally:
        for mod, name, orig in saved:
            setattr(mod, name, orig)


def run_case(cfg, info, deep=False, eager=False, collectives=None):
    """Three steps of one case -> (records, final master, final flat_param)."""
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[cfg.dtype]
    task = _deep_task(info.device, dtype, cfg.seed) if deep else None
    coll = collectives if collectives is not None else []
    del coll[:]
    tr = ConsensusTrainer(cfg, task=task, info=info)
    e = tr.engine
    e._gram_eager = eager
    assert len(e.flat.buckets) == (18 if deep else 4), len(e.flat.buckets)
    with tracing(e, coll) as t:
        for step in range(STEPS):
            e.record_stats = step == STEPS - 1
            tr.train_step()
        e.wait_params()
    if e.device.type == "cuda":
        torch.cuda.synchronize()
    if cfg.optim.clip_norm:
        assert 0 < float(e.grad_stats[1]) < 1, e.grad_stats    # the case clips
    out = (json.loads(json.dumps(t.records)), e.master.detach().cpu().clone(),
           e.flat.flat_param.detach().cpu().clone())
    tr.close()
    return out


def run_world1(device):
    """Every one-process case on ``device`` -> ({id: records}, {id-master | id-flat_param:
    final tensor})."""
    import torch.distributed as dist
    from consensusml_amd.parallel.dist import DistInfo
    info = DistInfo(0, 1, 0, device, "none")
    saved = {n: getattr(dist, n) for n in LP.COLLECTIVES}
    coll = LP.record_collectives(dist)
    traces, tensors = {}, {}
    try:
        for cid, cfg, deep in world1_cases("bf16" if device.type == "cuda" else "fp32"):
            traces[cid], tensors[cid + "-master"], tensors[cid + "-flat_param"] = run_case(
                cfg, info, deep, collectives=coll)
    finally:
        for n, f in saved.items():
            setattr(dist, n, f)
    return traces, tensors


def _world2_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from consensusml_amd.parallel import dist as D
    D._INFO = None
    info = D.init_distributed("gloo", timeout_s=60)
    coll = LP.record_collectives(dist)
    traces = {}
    for cid, topo, rule, clip, prefetch in WORLD2_CASES:
        cfg = make_cfg("fp32", topo, rule, V=1, f=0, clip=clip)
        cfg.backend = "gloo"
        cfg.topology.param_prefetch = prefetch
        traces[f"{cid}-r{rank}"] = run_case(cfg, info, eager=True, collectives=coll)[0]
    with open(os.path.join(out_dir, f"trace_r{rank}.json"), "w") as fh:
        json.dump(traces, fh)
    D.monitored_barrier(60)
    dist.destroy_process_group()


def run_world2(out_dir):
    """The two-rank gloo cases, spawned -> {id-r<rank>: records}."""
    import torch.multiprocessing as mp
    from test_dist_gloo import _free_port
    mp.spawn(_world2_worker, args=(2, _free_port(), str(out_dir)), nprocs=2, join=True)
    traces = {}
    for r in range(2):
        with open(os.path.join(out_dir, f"trace_r{r}.json")) as fh:
            traces.update(json.load(fh))
    return traces


# --------------------------------------------------------------------------- the files
def encode(traces):
    atoms, index, cases = [], {}, {}
    for cid, recs in traces.items():
        rows = []
        for rec in recs:
            row = []
            for pair in rec.items():
                key = json.dumps(pair, sort_keys=True)
                if key not in index:
                    index[key] = len(atoms)
                    atoms.append(list(pair))
                row.append(index[key])
            rows.append(row)
        cases[cid] = rows
    return {"atoms": atoms, "cases": cases}


def decode(doc):
    atoms = doc["atoms"]
    return {cid: [{atoms[i][0]: atoms[i][1] for i in row} for row in rows]
            for cid, rows in doc["cases"].items()}


def save_traces(traces, path):
    doc = encode(traces)
    js = lambda v: json.dumps(v, separators=(",", ":"))   # noqa: E731
    with open(path, "w") as fh:
        fh.write('{"atoms":[\n' + ",\n".join(js(a) for a in doc["atoms"]) + '\n],"cases":{\n')
        fh.write(",\n".join(f"{js(c)}:{js(r)}" for c, r in doc["cases"].items()) + "\n}}\n")


def load_traces(path):
    with open(path) as fh:
        return decode(json.load(fh))


def pack(tensors):
    """Every tensor of one dtype as a view of one storage: one record per dtype in the file."""
    out = dict(tensors)
    for dtype in {t.dtype for t in out.values()}:
        keys = [k for k in out if out[k].dtype == dtype]
        flat = torch.cat([out[k].flatten() for k in keys])
        o = 0
        for k in keys:
            out[k] = flat[o:o + out[k].numel()]
            o += out[k].numel()
    return out


def first_difference(got, want):
    """None, or a message naming the first record of ``got`` that is not ``want``'s."""
    if got == want:
        return None
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return (f"diverges at record {k} of {len(got)} / {len(want)}: got {got[k:k + 1]}, "
            f"recorded {want[k:k + 1]}")


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "cpu":
        traces, _ = run_world1(torch.device("cpu"))
        with tempfile.TemporaryDirectory() as tmp:
            traces.update(run_world2(tmp))
        save_traces(traces, sys.argv[2])
    else:
        traces, tensors = run_world1(torch.device("cuda", 0))
        save_traces(traces, sys.argv[2])
        torch.save(pack(tensors), sys.argv[3])
