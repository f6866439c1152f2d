"""Typed configuration for the consensus engine.

The reference has no config system: hyper-parameters, seeds and paths are globals at the top of
each notebook (`composite_code/rnotebook/cml_targetaml_seanalysis.Rmd:370-406`), knitr chunk
options (`...seanalysis.Rmd:10-22`) and literals inside calls (`scripts/model_comp.py:7-9`).
Here one dataclass tree covers model, aggregation rule, topology, optimizer, fault injection and
profiling, with YAML files and ``key.sub=value`` CLI overrides on top.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import yaml

RULES = ("mean", "median", "trimmed_mean", "meamed", "phocas", "krum", "multi_krum", "geomed", "bulyan",
         "centered_clip")
COORD_RULES = ("median", "trimmed_mean", "meamed", "phocas")
TOPOLOGIES = ("allreduce", "allgather", "sharded", "gossip")
GOSSIP_GRAPHS = ("ring", "exp", "exp_all")
PRE = ("none", "nnm")
FAULTS = ("none", "sign_flip", "gaussian", "scaled", "zero", "nan", "alie", "ipm")


@dataclass
class AggConfig:
    """Robust aggregation rule and its parameters.

    rule          one of RULES
    f             number of Byzantine workers tolerated (Krum / Multi-Krum / Bulyan); meamed and
                  phocas average the n - f values nearest to their centre per coordinate (the
                  median / the trimmed mean)
    trim          number trimmed from each side per coordinate (trimmed mean, and the centre of
                  phocas); ``None`` -> f
    m             number of workers averaged by Multi-Krum; ``None`` -> n - f
    iters, eps    Weiszfeld iterations and distance floor (geometric median)
    tau, clip_iters  radius / iterations of centered clipping. With ``optim.worker_momentum`` the
                  clipped rows are momenta, about 1 / (1 - momentum) larger than gradients; tau
                  is taken as given, never rescaled
    centered_gram Gram-space rules: the Gram of the rows relative to a medoid worker row, so
                  near-duplicate workers' distances do not cancel (ops.kernels.gram). ONE pass
                  per step, centered at the medoid picked from the previous step's Gram; the
                  first step (and a restore from a checkpoint that has no center) runs an
                  uncentered pass first to pick it
    gram_two_pass every step: uncentered pass -> medoid -> centered pass (+ a second Gram
                  all-reduce in the sharded topology); the round-3 scheme
    pre           pre-aggregation, one of PRE. ``nnm``: nearest-neighbour mixing (Allouah et al.
                  2023) -- each worker row is replaced by the mean of its n - f nearest rows
                  (itself included, distances from the Gram matrix) before the rule runs.
                  allgather / sharded topologies; every rule but mean and bulyan; coordinate
                  rules with n <= 32
    """
    rule: str = "mean"
    f: int = 0
    trim: Optional[int] = None
    m: Optional[int] = None
    iters: int = 8
    eps: float = 1e-6
    tol: float = 1e-7
    tau: float = 10.0
    clip_iters: int = 3
    centered_gram: bool = True
    gram_two_pass: bool = False
    pre: str = "none"

    def validate(self, n: int) -> None:
        if self.rule not in RULES:
            raise ValueError(f"unknown aggregation rule {self.rule!r}; choose from {RULES}")
        if self.pre not in PRE:
            raise ValueError(f"unknown pre-aggregation {self.pre!r}; choose from {PRE}")
        if self.pre == "nnm":
            if self.rule in ("mean", "bulyan"):
                raise ValueError(f"agg.pre=nnm is not implemented for rule {self.rule!r}")
            if n <= 2 * self.f:
                raise ValueError(f"agg.pre=nnm needs n > 2f (n={n}, f={self.f})")
            if self.rule in COORD_RULES and n > 32:
                raise ValueError(f"agg.pre=nnm with {self.rule} supports at most 32 workers "
                                 f"(n={n})")
        # the HIP kernels keep one worker row per lane of a 64-wide wave; centered clipping adds
        # the previous aggregate as row n
        limit = 63 if self.rule == "centered_clip" else 64
        if n > limit:
            raise ValueError(f"{self.rule} supports at most {limit} workers (n={n})")
        if self.rule in ("meamed", "phocas") and n <= 2 * self.f:
            raise ValueError(f"{self.rule} needs n > 2f (n={n}, f={self.f})")
        if self.rule in ("krum", "multi_krum") and n > 1 and n <= 2 * self.f:
            # Krum's guarantee needs n >= 2f+3; smaller n runs (nearest-neighbour scoring) but
            # f < n/2 is the hard floor.
            raise ValueError(f"{self.rule} needs n > 2f (n={n}, f={self.f})")
        if self.rule == "bulyan" and n > 1 and n < 4 * self.f + 3:
            raise ValueError(f"bulyan needs n >= 4f+3 (n={n}, f={self.f})")
        b = self.trim if self.trim is not None else self.f
        if self.rule in ("trimmed_mean", "phocas") and 2 * b >= n:
            raise ValueError(f"{self.rule} needs n > 2*trim (n={n}, trim={b})")


@dataclass
class OptimConfig:
    """Optimizer of the fused aggregate-and-update step.

    worker_momentum  SGD only (Karimireddy, He, Jaggi 2021, "Learning from History"): the
                     momentum ``momentum`` is applied per worker BEFORE the exchange instead of
                     to the aggregate. Every local worker keeps an fp32 buffer m_i <- momentum *
                     m_i + g_i (no dampening, torch.optim.SGD's buffer) and sends m_i rounded to
                     the comm dtype in place of its gradient; the server applies plain SGD to
                     rule(m_1..m_n), so there is one momentum, never two. With the mean rule the
                     trajectory is that of server momentum; every non-linear rule sees rows whose
                     variance is reduced over the momentum window. Order within a step: capture
                     -> momentum -> fault injection -> exchange, so a Byzantine worker's state
                     advances from its own honest gradient and ALIE / IPM statistics are taken
                     over the honest workers' momenta. allgather / sharded topologies. Weight
                     decay stays on the server, outside the momentum. The rows are about
                     1 / (1 - momentum) larger than gradients: ``agg.tau`` is not rescaled
    clip_norm        global-norm clipping of the AGGREGATE (0 = off: the fused step as it is).
                     With clip_norm = c > 0 every step scales the aggregated gradient g -- the
                     mean over workers or the rule's output, over all parameters of the model
                     (all buckets; sharded topology: all ranks, one fp64 all-reduce) -- by
                     min(1, c / (||g||_2 + 1e-6)) before weight decay, momentum and Adam see it:
                     the arithmetic of ``torch.nn.utils.clip_grad_norm_``. The norm stays on
                     the device (``engine.grad_stats``). A non-finite norm gives coefficient 0:
                     the step applies a ZERO gradient (weight decay and the moments' decay still
                     act) and counts the event in ``engine.grad_stats[2]``; no state is poisoned.
                     Gossip: every rank clips its own local gradient. centered_clip: v0 is the
                     unclipped aggregate. With ``worker_momentum`` the clipped quantity is the
                     aggregate of the momenta (about 1 / (1 - momentum) the gradient scale);
                     nothing is rescaled
    name=lars        layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017) on the
                     AGGREGATE, in the LARC form: the gradient of every adapted tensor is scaled
                     by its trust ratio, then SGD-momentum runs unchanged. Per parameter tensor,
                     over exactly its elements, with p the fp32 master and g the aggregate (the
                     mean over workers or the rule's output): wn = ||p||, gn = ||g|| (fp64 sums);
                     q = trust_coef * wn / (gn + weight_decay * wn + eps) when the tensor is
                     adapted and wn > 0 and gn > 0, else q = 1; then per element g <- g +
                     weight_decay * p, g <- q * g, and SGD's momentum / Nesterov / p <- p - lr * g.
                     The step of an adapted tensor has length lr * trust_coef * wn whatever the
                     aggregate's magnitude. A non-finite norm gives q = 0 for that tensor: it
                     takes a ZERO gradient this step (counted in ``engine.lars_stats[t, 3]``), no
                     state is poisoned. Like clip_norm it runs as three device stages (aggregate
                     -> per-tensor norms -> update; sharded topology: ONE all-reduce of the fp64
                     [T, 2] sums), so ``topology.early_update`` is off. ``engine.lars_stats``
                     (fp64 [T, 4]) = [wn, gn, q, non-finite steps] per tensor. Not implemented
                     together with ``clip_norm`` or ``worker_momentum``; one weight decay for all
                     tensors
    trust_coef       LARS trust coefficient (> 0)
    lars_exclude_1d  LARS: tensors with fewer than 2 dimensions (biases, BatchNorm / LayerNorm
                     affine) are not adapted (q = 1): they take the plain SGD step, weight decay
                     included
    eps              Adam's denominator term; LARS: the term added to the ratio's denominator
    """
    name: str = "sgd"            # sgd | adam | adamw | lars
    lr: float = 0.1
    momentum: float = 0.9
    nesterov: bool = False
    weight_decay: float = 0.0
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    worker_momentum: bool = False
    clip_norm: float = 0.0
    trust_coef: float = 0.001
    lars_exclude_1d: bool = True

    def validate(self) -> None:
        c = self.clip_norm
        if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c < 0:
            raise ValueError(f"optim.clip_norm must be a finite number >= 0 (got {c!r})")
        t = self.trust_coef
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or t <= 0:
            raise ValueError(f"optim.trust_coef must be a finite number > 0 (got {t!r})")
        if self.name == "lars" and c > 0:
            raise ValueError("optim.name=lars with optim.clip_norm > 0 is not implemented")
        if not self.worker_momentum:
            return
        if self.name == "lars":
            raise ValueError("optim.worker_momentum is not implemented with optim.name=lars "
                             "(it needs optim.name=sgd)")
        if self.name != "sgd":
            raise ValueError(f"optim.worker_momentum needs optim.name=sgd (got {self.name!r})")
        if self.momentum == 0:
            raise ValueError("optim.worker_momentum needs optim.momentum != 0: it moves that "
                             "momentum to the workers")
        if self.nesterov:
            raise ValueError("optim.worker_momentum is not implemented with optim.nesterov")


@dataclass
class TopologyConfig:
    """Exchange topology and its overlap switches (one comment per field below).

    ``early_update`` (gossip, one worker per rank: each bucket's optimizer step runs during
    backward) is forced off while ``optim.clip_norm`` > 0: the update of the first bucket would
    need the gradient norm over all of them. The engine logs the switch once. The same holds for
    ``optim.name=lars``, whose update waits for the per-tensor norms.
    """
    kind: str = "sharded"        # allreduce | allgather | sharded | gossip
    bucket_mb: float = 64.0      # bucket size in MB of gradient (bf16 on the wire)
    comm_dtype: str = "bf16"     # dtype of exchanged gradients
    overlap: bool = True         # launch bucket collectives during backward
    gossip_graph: str = "ring"   # ring | exp (one rotating peer 2^(t mod log2 N)) | exp_all
    gossip_chunk_mb: float = 256.0   # gossip exchange pipeline chunk (MB of bf16)
    gossip_weights: tuple = (1 / 3, 1 / 3, 1 / 3)   # ring: self, left, right
    gossip_clip: float = 0.0     # 0 disables neighbour-delta clipping; > 0 also drops a neighbour
                                 # whose distance is not finite (NaN / Inf / fp32 overflow): its
                                 # mixing weight stays with the local parameters
    gossip_async: bool = False   # delayed gossip: exchange overlaps the next step's compute
    early_update: bool = True    # gossip, 1 local worker: per-bucket optimizer step in backward
                                 # (forced off while optim.clip_norm > 0: the update of the first
                                 # bucket needs the norm over all of them)
    param_prefetch: bool = True  # sharded: bf16 parameter all-gather overlaps the next forward
    early_gram: bool = True      # Gram-space rules: per-bucket Gram as each exchange lands
    gram_lag: int = 1            # GPU runs: bucket b's Gram is enqueued on the compute stream at
                                 # the flush of bucket b + gram_lag (its exchange has had one
                                 # bucket of backward to land); the last ones run in step()
    direct_grads: bool = True    # one worker per rank: ops with a per-worker gradient path
                                 # (ops.worker_grads: transformer linears, norms, embeddings) write
                                 # their parameter gradients straight into the flat gradient row
                                 # during backward instead of autograd tensors + the capture copy

    def validate(self) -> None:
        if self.kind not in TOPOLOGIES:
            raise ValueError(f"unknown topology {self.kind!r}; choose from {TOPOLOGIES}")
        if self.gossip_graph not in GOSSIP_GRAPHS:
            raise ValueError(f"unknown gossip graph {self.gossip_graph!r}; choose from "
                             f"{GOSSIP_GRAPHS}")
        if self.gossip_chunk_mb <= 0:
            raise ValueError("gossip_chunk_mb must be positive")


@dataclass
class FaultConfig:
    kind: str = "none"
    ranks: List[int] = field(default_factory=list)   # Byzantine ranks / virtual workers
    scale: float = 10.0
    sigma: float = 1.0
    z: float = 1.0               # ALIE z-score
    start_step: int = 0

    def validate(self) -> None:
        if self.kind not in FAULTS:
            raise ValueError(f"unknown fault {self.kind!r}; choose from {FAULTS}")


@dataclass
class ModelConfig:
    name: str = "mlp"            # mlp | resnet50 | bert_base | llama3_8b | llama_tiny | bert_tiny
    num_classes: int = 1000
    image_size: int = 224
    seq_len: int = 128
    in_features: int = 32
    hidden: int = 64
    extra: Dict[str, Any] = field(default_factory=dict)


@dataclass
class TrainConfig:
    model: ModelConfig = field(default_factory=ModelConfig)
    agg: AggConfig = field(default_factory=AggConfig)
    optim: OptimConfig = field(default_factory=OptimConfig)
    topology: TopologyConfig = field(default_factory=TopologyConfig)
    fault: FaultConfig = field(default_factory=FaultConfig)
    batch_per_worker: int = 32
    virtual_workers: int = 1     # >1: each rank simulates this many workers (micro-batches)
    steps: int = 10
    seed: int = 2019             # the reference's split seed (DEL:159)
    dtype: str = "bf16"
    backend: str = "auto"        # auto | nccl | gloo
    data_path: Optional[str] = None   # record file for the native loader (else synthetic)
    loader_threads: int = 4
    log_path: Optional[str] = None
    ckpt_dir: Optional[str] = None
    ckpt_every: int = 0
    profile: bool = False

    # ------------------------------------------------------------------ io
    def to_dict(self) -> Dict[str, Any]:
        return dataclasses.asdict(self)

    def to_json(self) -> str:
        return json.dumps(self.to_dict(), sort_keys=True)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "TrainConfig":
        cfg = cls()
        for k, v in (d or {}).items():
            _set_path(cfg, k, v)
        return cfg

    @classmethod
    def from_yaml(cls, path: str) -> "TrainConfig":
        with open(path) as fh:
            return cls.from_dict(_flatten(yaml.safe_load(fh) or {}))

    def override(self, items: List[str]) -> "TrainConfig":
        """Apply ``a.b=value`` overrides (value parsed as YAML scalar/list)."""
        for it in items:
            if "=" not in it:
                raise ValueError(f"override {it!r} must look like key.sub=value")
            k, v = it.split("=", 1)
            _set_path(self, k, yaml.safe_load(v))
        return self

    def validate(self, n_workers: int) -> "TrainConfig":
        self.agg.validate(n_workers)
        self.topology.validate()
        if self.agg.pre != "none" and self.topology.kind in ("gossip", "allreduce"):
            raise ValueError(f"agg.pre={self.agg.pre} needs the allgather or sharded topology "
                             f"(got {self.topology.kind!r}: no worker rows to mix)")
        self.optim.validate()
        if self.optim.worker_momentum and self.topology.kind in ("gossip", "allreduce"):
            raise ValueError("optim.worker_momentum needs the allgather or sharded topology "
                             f"(got {self.topology.kind!r}: no worker rows to aggregate)")
        self.fault.validate()
        return self


def _flatten(d: Dict[str, Any], prefix: str = "") -> Dict[str, Any]:
    out: Dict[str, Any] = {}
    for k, v in d.items():
        key = f"{prefix}{k}"
        if isinstance(v, dict) and k != "extra":
            out.update(_flatten(v, key + "."))
        else:
            out[key] = v
    return out


def _set_path(obj: Any, path: str, value: Any) -> None:
    parts = path.split(".")
    for p in parts[:-1]:
        if not hasattr(obj, p):
            raise KeyError(f"unknown config key {path!r}")
        obj = getattr(obj, p)
    last = parts[-1]
    if not hasattr(obj, last):
        raise KeyError(f"unknown config key {path!r}")
    cur = getattr(obj, last)
    if isinstance(cur, tuple) and isinstance(value, list):
        value = tuple(value)
    if isinstance(cur, float) and isinstance(value, int):
        value = float(value)
    setattr(obj, last, value)


def add_cli(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("--config", type=str, default=None, help="YAML config file")
    parser.add_argument("--set", nargs="*", default=[], help="overrides key.sub=value")
    return parser


def from_cli(args: argparse.Namespace) -> TrainConfig:
    cfg = TrainConfig.from_yaml(args.config) if args.config else TrainConfig()
    return cfg.override(args.set or [])
