"""What a ResNet bottleneck launches, with which tensors and in which order, must not move (not
collected: no ``test_`` prefix).

``run_cases`` runs a forward and a backward of short bottleneck chains and of ResNet-50 and logs
one record per call of

* any function of the native module, reached through ``ops.native.lib()``: a proxy stands in for
  the loaded module, so every caller (``ops/conv.py``, ``ops/bn.py``, ``ops/pool.py``,
  ``ops/stem.py``, ``models/resnet.py``) sees it;
* every library convolution or GEMM (``ATEN``: aten ``convolution``, ``convolution_backward``,
  ``mm``, ``addmm``, ``addmm_``), through a ``TorchDispatchMode``. The backward runs with
  ``torch.autograd.set_multithreading_enabled(False)``, so that the mode, which is thread-local,
  also sees what the autograd engine would run on its device thread.

A record is the function name and every argument (``a0``, ``a1``, ... and the keywords). A tensor
is logged as the first of these that applies:

* ``[parameter or buffer name, element offset, shape, stride, dtype]`` of the model;
* ``["x", ...]`` / ``["gy", ...]``: the case's input or output gradient;
* ``["out", r, k, offset, shape, stride, dtype]``: output ``k`` (leaf index) of the earlier record
  ``r``, matched by storage. The tracer keeps every output alive until the case ends, so no
  address is reused;
* ``["other", shape, stride, dtype]``.

Scalars, ``None``, lists and dtypes are logged as they are: the trace is a dataflow graph, and a
tensor wired to the wrong argument fails it even where the shapes agree. No tensor values are
stored (MIOpen is not bit-reproducible between runs; the numeric tests hold the values).

Cases (``case_list``): bf16, channels_last, batch 2, ``x = randn(...).relu()`` (a block input is
a ReLU output), BN weights uniform(0.5, 1.5). ``L1`` .. ``L4`` are a downsample block and an
identity block of each ResNet-50 stage at the smallest input that still reaches the rungs the
full model reaches (``fused_conv1x1_policy`` switches at 784 output pixels, ``conv1x1_policy`` at
196 pixels and 1024 channels). Each runs under the default policy, with one ``VARIANTS`` entry
changed at a time, and once in ``eval()`` under ``no_grad``; ``R50`` is ``resnet50`` at 224 x 224
under the default policy (pool link, batched weight layouts, every block of the benchmark).

``tests/golden/resnet_trace_gpu.json`` holds what commit 0092209 (the one BEFORE the 3x3
Functions and ``Bottleneck._forward_fused`` were folded) produced on an MI355X:

    python tests/resnet_trace.py gpu tests/golden/resnet_trace_gpu.json

run twice in a checkout of that commit with this file copied in; the two recordings were equal.
``test_resnet_trace_gpu.py`` compares record for record (``compare_cases``: a case stops at its
first call that is not the recorded one, before that call is made).
"""
import contextlib
import json
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from engine_trace import decode, encode, first_difference, load_traces, save_traces  # noqa: F401

ATEN = ("convolution", "convolution_backward", "mm", "addmm", "addmm_")
CHAINS = {  # id -> ((inplanes, planes, stride) of the downsample block, input size)
    "L1": ((64, 64, 1), 28),
    "L2": ((256, 128, 2), 56),
    "L3": ((512, 256, 2), 28),
    "L4": ((1024, 512, 2), 14),
}
VARIANTS = [
    {"bn1_dgrad_sums": False},
    {"bn1_sums_lib_conv1": True},
    {"conv3x3_bn_stats": False},
    {"own_dgrad3x3": False},
    {"own_conv3x3_s2": False},
    {"recompute_tail": False},
    {"recompute_tail": False, "fused_bn3_bwd": False},
    {"recompute_down_tail": False},
    {"recompute_down_tail_s2": False},
    {"down_s2_compact": False},
    {"fuse_down_bn": False},
    {"residual_link": False},
    {"fin_affine": False},
    {"gram_stats": False},
    {"fused_conv1x1": False},
]
N_CASES = len(CHAINS) * (len(VARIANTS) + 2) + 1


def case_list():
    """(id, chain or None for ResNet-50, policy fields changed, train) of every case."""
    out = []
    for cid in CHAINS:
        out.append((cid, cid, {}, True))
        for kw in VARIANTS:
            tag = ",".join(f"{k}={v}" for k, v in kw.items())
            out.append((f"{cid}-{tag}", cid, kw, True))
        out.append((f"{cid}-eval", cid, {}, False))
    out.append(("R50", None, {}, True))
    return out


def init_bn(model):
    """BN weights uniform(0.5, 1.5), small biases (as ``test_bwd_fusion_gpu._chain``)."""
    with torch.no_grad():
        for mod in model.modules():
            if mod.__class__.__name__ == "BatchNormAct2d":
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.1, 0.1)
    return model


def make_chain(cid, device):
    """(model, x) of a ``CHAINS`` entry: its downsample block, then an identity block."""
    from consensusml_amd.models.resnet import Bottleneck
    (cin, planes, stride), size = CHAINS[cid]
    torch.manual_seed(0)
    m = init_bn(torch.nn.Sequential(Bottleneck(cin, planes, stride, True),
                                    Bottleneck(planes * 4, planes)))
    m = m.to(device=device, dtype=torch.bfloat16, memory_format=torch.channels_last)
    gen = torch.Generator(device=device).manual_seed(1)
    x = torch.randn(2, cin, size, size, device=device, generator=gen).relu().bfloat16()
    return m, x.contiguous(memory_format=torch.channels_last)


def make_resnet50(device):
    from consensusml_amd.models.resnet import resnet50
    torch.manual_seed(0)
    m = init_bn(resnet50(num_classes=10))
    m = m.to(device=device, dtype=torch.bfloat16, memory_format=torch.channels_last)
    gen = torch.Generator(device=device).manual_seed(1)
    x = torch.randn(2, 3, 224, 224, device=device, generator=gen).relu().bfloat16()
    return m, x.contiguous(memory_format=torch.channels_last)


# --------------------------------------------------------------------------- the recorder
def _leaves(v):
    if isinstance(v, (list, tuple)):
        for x in v:
            yield from _leaves(x)
    else:
        yield v


def _storage(t):
    return t.untyped_storage().data_ptr() if t.numel() else 0


class Diverged(AssertionError):
    """A call that is not the recorded one (raised before the call is made)."""


class Tracer:
    def __init__(self, named, expect=None):
        """``named``: (name, tensor) of the model's parameters and buffers and the case's x.
        ``expect``: the recorded trace; the first call that differs from it raises ``Diverged``
        instead of running (a mis-wired kernel is never launched)."""
        self.records, self.depth, self.expect = [], 0, expect
        self.known = {}    # storage address -> (reference head, base tensor, kept alive)
        for name, t in named:
            self.name(name, t)

    def name(self, name, t):
        self.known.setdefault(_storage(t), ([name], t))

    def tensor(self, t):
        desc = [list(t.shape), list(t.stride()), str(t.dtype)]
        hit = self.known.get(_storage(t)) if t.numel() else None
        if hit is None:
            return ["other"] + desc
        head, base = hit
        return head + [(t.data_ptr() - base.data_ptr()) // t.element_size()] + desc

    def value(self, v):
        if torch.is_tensor(v):
            return self.tensor(v)
        if isinstance(v, (list, tuple)):
            return [self.value(x) for x in v]
        if isinstance(v, torch.dtype):
            return str(v)
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"resnet_trace: cannot log a {type(v).__name__}")

    def call(self, name, fn, args, kwargs):
        if self.depth:
            return fn(*args, **kwargs)
        rec = {"fn": name}
        rec.update({f"a{i}": self.value(v) for i, v in enumerate(args)})
        rec.update({k: self.value(v) for k, v in kwargs.items()})
        r = len(self.records)
        if self.expect is not None and rec != (self.expect[r:r + 1] or [None])[0]:
            raise Diverged(f"diverges at record {r} of {len(self.expect)} recorded: got {rec}, "
                           f"recorded {self.expect[r:r + 1]}")
        self.records.append(rec)
        self.depth += 1
        try:
            out = fn(*args, **kwargs)
        finally:
            self.depth -= 1
        for k, t in enumerate(_leaves(out)):
            if torch.is_tensor(t) and t.numel():
                self.known.setdefault(_storage(t), (["out", r, k], t))
        return out


class _Lib:
    """The native module with every function traced (attributes pass through)."""

    def __init__(self, real, tracer):
        self._real, self._tracer, self._wrapped = real, tracer, {}

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if not callable(v):
            return v
        if name not in self._wrapped:
            tr = self._tracer
            self._wrapped[name] = lambda *a, **k: tr.call("lib." + name, v, a, k)
        return self._wrapped[name]


class _Aten(TorchDispatchMode):
    def __init__(self, tracer):
        super().__init__()
        self.tracer = tracer

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func.namespace == "aten" and func._overloadpacket.__name__ in ATEN:
            return self.tracer.call(str(func), func, args, kwargs)
        return func(*args, **kwargs)


@contextlib.contextmanager
def tracing(named, expect=None):
    """Log every native call and library conv / GEMM; ``named``, ``expect`` as for ``Tracer``."""
    from consensusml_amd.ops import native
    real = native.lib()
    tr = Tracer(named, expect)
    native._C = _Lib(real, tr)
    try:
        with torch.autograd.set_multithreading_enabled(False), _Aten(tr):
            yield tr
    finally:
        native._C = real


def run_model(model, x, train=True, gy_seed=2, expect=None):
    """One forward (+ backward when ``train``) of ``model`` on ``x`` -> records."""
    named = list(model.named_parameters()) + list(model.named_buffers()) + [("x", x)]
    model.train(train)
    with tracing(named, expect) as tr:
        if train:
            x.requires_grad_(x.shape[1] != 3)    # a block input carries a gradient, an image none
            y = model(x)
            gen = torch.Generator(device=x.device).manual_seed(gy_seed)
            gy = torch.randn(y.shape, device=x.device, generator=gen).to(y.dtype)
            if gy.dim() == 4:
                gy = gy.contiguous(memory_format=torch.channels_last)
            tr.name("gy", gy)
            y.backward(gy)
        else:
            with torch.no_grad():
                model(x)
        if x.is_cuda:
            torch.cuda.synchronize()
    return json.loads(json.dumps(tr.records))


def run_case(chain, kw, train, device, expect=None):
    from consensusml_amd import perf
    model, x = make_resnet50(device) if chain is None else make_chain(chain, device)
    with perf.use_policy(perf.policy().replace(**kw)):
        return run_model(model, x, train, expect=expect)


def run_cases(device):
    """Every case on ``device`` -> {id: records}."""
    return {cid: run_case(chain, kw, train, device) for cid, chain, kw, train in case_list()}


def compare_cases(device, want):
    """Run every case against its recorded trace -> ["<id> <first difference>"] of those that
    differ (each stops at its first call that is not the recorded one)."""
    bad = []
    for cid, chain, kw, train in case_list():
        try:
            diff = first_difference(run_case(chain, kw, train, device, want[cid]), want[cid])
        except Diverged as e:
            diff = str(e)
        if diff is not None:
            bad.append(f"{cid} {diff}")
    return bad


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    traces = run_cases(torch.device("cuda", 0))
    assert len(traces) == N_CASES
    fns = {r["fn"] for r in traces["R50"]}
    assert "aten.convolution_backward.default" in fns, "the backward's calls are not logged"
    save_traces(traces, sys.argv[2])
