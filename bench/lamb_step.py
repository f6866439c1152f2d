#!/usr/bin/env python3
"""What LAMB (optim.name=lamb, FusedLAMB) costs on the update side, on one MI355X.

On BERT-base's and ResNet-50's parameter lists (bf16 parameters with an fp32 master for the fused
optimizers, fp32 parameters for the foreach baseline), alternating all of them within every
repetition (HIP events after a warm-up of three calls each; median, min and max over the
repetitions):
  fused_lamb_ms    FusedLAMB.step(): norms of the Adam direction + ratios + update
                   (csrc/kernels/lamb.hip, the ratio kernel of lars.hip)
  norm_ms          ``lamb_norms`` alone on FusedLAMB's flat buffer: the read-only pass (14 bytes
                   per element: bf16 gradient, fp32 master and both moments) and the item fold
  update_ms        ``lamb_update`` alone (28 bytes per element: the same reads, master and
                   moments written, bf16 parameters out)
  fused_adamw_ms   FusedAdamW.step() of the same commit: one fused launch (28 bytes per element)
  foreach_lamb_ms  the same LAMB step written with torch._foreach_* ops on fp32 tensors
and the ratio fused_lamb / fused_adamw next to the byte ratio 42 / 28 = 1.5. One JSON line per
model.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lars_step import alternate, shapes_of  # noqa: E402


def foreach_lamb(params, grads, ms, vs, adapted, lr, b1, b2, eps, wd, k):
    """LAMB as FusedLAMB defines it, with multi-tensor ops and no host read."""
    torch._foreach_mul_(ms, b1)
    torch._foreach_add_(ms, grads, alpha=1 - b1)
    torch._foreach_mul_(vs, b2)
    torch._foreach_addcmul_(vs, grads, grads, value=1 - b2)
    den = torch._foreach_sqrt(vs)
    torch._foreach_mul_(den, 1 / math.sqrt(1 - b2 ** k))
    torch._foreach_add_(den, eps)
    u = torch._foreach_div(ms, den)
    torch._foreach_mul_(u, 1 / (1 - b1 ** k))
    torch._foreach_add_(u, params, alpha=wd)
    wn = torch._foreach_norm(params)
    un = torch._foreach_norm(u)
    qs, us = [], []
    for w, n, ui, ad in zip(wn, un, u, adapted):
        if ad:
            qs.append(torch.where((w > 0) & (n > 0), w / n, torch.ones_like(w)))
            us.append(ui)
    torch._foreach_mul_(us, qs)
    torch._foreach_add_(params, u, alpha=-lr)


def run_steps(model: str, reps: int, dev) -> dict:
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.optim import FusedAdamW, FusedLAMB
    shapes = shapes_of(model)
    gen = torch.Generator(device=dev).manual_seed(0)

    def params(dtype):
        return [torch.nn.Parameter((torch.randn(s, generator=gen, device=dev) * 0.05).to(dtype))
                for s in shapes]

    hp = dict(lr=1e-3, eps=1e-6, weight_decay=0.01)
    pl, pa, pf = params(torch.bfloat16), params(torch.bfloat16), params(torch.float32)
    lamb = FusedLAMB(pl, **hp)
    adamw = FusedAdamW(pa, **hp)
    for group in (pl, pa):
        for p in group:
            p.grad.copy_((torch.randn(p.shape, generator=gen, device=dev) * 1e-3).to(p.dtype))
    gf = [torch.randn(p.shape, generator=gen, device=dev) * 1e-3 for p in pf]
    mf, vf = [torch.zeros_like(p) for p in pf], [torch.zeros_like(p) for p in pf]
    adapted = [p.dim() >= 2 for p in pf]
    fl = lamb.flat_buffers()[0]
    plan, _, pairs, q, _ = lamb._lamb[0]
    m, v = fl.states
    o = K.OptArgs(kind="lamb", lr=1e-3, weight_decay=0.01, eps=1e-6, step=10)
    with torch.no_grad():
        t = alternate({
            "fused_lamb": lamb.step,
            "norm": lambda: K.lamb_norms(fl.master, fl.grad, 1.0, plan, o, m, v, out=pairs),
            "update": lambda: K.lamb_update(fl.grad, 1.0, plan, q, o, fl.master, m, v,
                                            segs=[(fl.param, 0, fl.total)]),
            "fused_adamw": adamw.step,
            "foreach_lamb": lambda: foreach_lamb(pf, gf, mf, vf, adapted, 1e-3, 0.9, 0.999, 1e-6,
                                                 0.01, 10)}, reps)
    numel = sum(p.numel() for p in pl)
    res = {"mode": "step", "model": model, "tensors": len(shapes), "numel": numel,
           "adamw_bytes_per_elem": 28, "lamb_bytes_per_elem": 42, "byte_ratio": 1.5}
    for k, (med, lo, hi) in t.items():
        res[f"{k}_ms"], res[f"{k}_min_ms"], res[f"{k}_max_ms"] = med, lo, hi
    res["lamb_over_adamw"] = round(t["fused_lamb"][0] / t["fused_adamw"][0], 3)
    res["foreach_over_lamb"] = round(t["foreach_lamb"][0] / t["fused_lamb"][0], 3)
    res["norm_GBps"] = round(numel * 14 / (t["norm"][0] * 1e-3) / 1e9, 1)
    res["update_GBps"] = round(numel * 28 / (t["update"][0] * 1e-3) / 1e9, 1)
    res["lamb_GBps"] = round(numel * 42 / (t["fused_lamb"][0] * 1e-3) / 1e9, 1)
    res["adamw_GBps"] = round(numel * 28 / (t["fused_adamw"][0] * 1e-3) / 1e9, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*", default=["bert_base", "resnet50"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for model in a.models:
        line = json.dumps(run_steps(model, a.reps, dev))
        print(line, flush=True)
        if a.json_out:
            with open(a.json_out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
