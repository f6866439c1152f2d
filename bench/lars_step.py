#!/usr/bin/env python3
"""What LARS (optim.name=lars, FusedLARS) costs on the update side, on one MI355X.

Default mode, on ResNet-50's and BERT-base's parameter lists (bf16 parameters with an fp32 master
for the fused optimizers, fp32 parameters for the foreach baseline), alternating the three within
every repetition (HIP events; median, min and max over the repetitions):
  fused_lars_ms    FusedLARS.step(): segmented norms + ratios + update (csrc/kernels/lars.hip)
  fused_sgd_ms     FusedSGD.step() of the same commit: one fused launch
  foreach_lars_ms  the same LARS step written with torch._foreach_* ops
  small_ms         two ``lars_ratio`` launches (one wave per tensor), timed alone: a stand-in for
                   the two small launches of a LARS step, the finalize of the norm pass and the
                   ratios. The real finalize also sums a tensor's item partials (37 for 2.4 M
                   elements at C = 65536), so this is a lower bound where single tensors are large
and the bytes per element each fused step moves, for the byte ratio next to the measured one.

--sweep: the kernels alone over one state vector of D elements (the project's two standard sizes),
as ONE tensor and cut like ResNet-50's tensor list, per work-item size C:
  norm_ms[C]       seg_sq_norm (fp32 master + fp32 / bf16 row: 8 / 6 bytes per element)
  update_ms        lars_update over the fp32 row with bf16 parameters out (22 bytes per element)
  sgd_kernel_ms    agg_update's weighted n = 1 SGD kernel on the same rows (22 bytes per element)
  staged_ms[C]     norms + ratios + update as one sequence (30 bytes per element), and its ratio
                   to sgd_kernel_ms next to the byte ratio 30 / 22
One JSON line per case.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns: dict, reps: int) -> dict:
    """Every function once per repetition, in turn; {name: (median, min, max)} in ms."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_time(fn))
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = (round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4))
    return out


def shapes_of(model: str):
    from consensusml_amd.models import bert_base, resnet50
    m = resnet50(1000) if model == "resnet50" else bert_base()
    return [tuple(p.shape) for p in m.parameters() if p.requires_grad]


def foreach_lars(params, grads, bufs, adapted, lr, momentum, wd, trust, eps):
    """LARS as FusedLARS defines it, with multi-tensor ops and no host read."""
    wn = torch._foreach_norm(params)
    gn = torch._foreach_norm(grads)
    d = torch._foreach_add(grads, params, alpha=wd)
    qs, ds = [], []
    for w, g, di, ad in zip(wn, gn, d, adapted):
        if ad:
            qs.append(torch.where((w > 0) & (g > 0), trust * w / (g + wd * w + eps),
                                  torch.ones_like(w)))
            ds.append(di)
    torch._foreach_mul_(ds, qs)
    torch._foreach_mul_(bufs, momentum)
    torch._foreach_add_(bufs, d)
    torch._foreach_add_(params, bufs, alpha=-lr)


def run_steps(model: str, reps: int, dev) -> dict:
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.optim import FusedLARS, FusedSGD
    shapes = shapes_of(model)
    gen = torch.Generator(device=dev).manual_seed(0)

    def params(dtype):
        ps = [torch.nn.Parameter((torch.randn(s, generator=gen, device=dev) * 0.05).to(dtype))
              for s in shapes]
        return ps

    hp = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)
    pl, ps, pf = params(torch.bfloat16), params(torch.bfloat16), params(torch.float32)
    lars = FusedLARS(pl, trust_coef=0.001, **hp)
    sgd = FusedSGD(ps, **hp)
    for group in (pl, ps):
        for p in group:
            p.grad.copy_((torch.randn(p.shape, generator=gen, device=dev) * 1e-3).to(p.dtype))
    gf = [torch.randn(p.shape, generator=gen, device=dev) * 1e-3 for p in pf]
    bf = [torch.zeros_like(p) for p in pf]
    adapted = [p.dim() >= 2 for p in pf]
    T = len(shapes)
    pairs = torch.ones(T, 2, dtype=torch.float64, device=dev)
    adapt = torch.ones(T, dtype=torch.uint8, device=dev)
    q = torch.ones(T, device=dev)
    stats = torch.zeros(T, K.LARS_STATS, dtype=torch.float64, device=dev)

    def small():
        K.lars_ratio(pairs, adapt, 0.001, 1e-4, 0.0, q, stats)
        K.lars_ratio(pairs, adapt, 0.001, 1e-4, 0.0, q, stats)

    with torch.no_grad():
        t = alternate({"fused_lars": lars.step, "fused_sgd": sgd.step,
                       "foreach_lars": lambda: foreach_lars(pf, gf, bf, adapted, 0.1, 0.9, 1e-4,
                                                            0.001, 0.0),
                       "small": small}, reps)
    numel = sum(p.numel() for p in pl)
    res = {"mode": "step", "model": model, "tensors": T, "numel": numel,
           # bf16 gradient 2, fp32 master + momentum read and written 16, bf16 parameters 2; LARS
           # reads master and gradient once more for the norms
           "sgd_bytes_per_elem": 20, "lars_bytes_per_elem": 26, "byte_ratio": round(26 / 20, 3)}
    for k, (med, lo, hi) in t.items():
        res[f"{k}_ms"], res[f"{k}_min_ms"], res[f"{k}_max_ms"] = med, lo, hi
    res["lars_over_sgd"] = round(t["fused_lars"][0] / t["fused_sgd"][0], 3)
    res["foreach_over_lars"] = round(t["foreach_lars"][0] / t["fused_lars"][0], 3)
    res["lars_GBps"] = round(numel * 26 / (t["fused_lars"][0] * 1e-3) / 1e9, 1)
    res["sgd_GBps"] = round(numel * 20 / (t["fused_sgd"][0] * 1e-3) / 1e9, 1)
    return res


def run_sweep(D: int, cut: str, chunks, reps: int, dev) -> dict:
    from consensusml_amd.ops import kernels as K
    D = -(-D // 64) * 64
    if cut == "one":
        starts, sizes = [0], [D]
    else:       # ResNet-50's tensor sizes, repeated until the vector is full
        base = [math_prod(s) for s in shapes_of("resnet50")]
        starts, sizes, off = [], [], 0
        k = 0
        while True:
            n = base[k % len(base)]
            if off + n > D:
                break
            starts.append(off)
            sizes.append(n)
            off += -(-n // 8) * 8
            k += 1
    gen = torch.Generator(device=dev).manual_seed(0)
    master = torch.randn(D, generator=gen, device=dev)
    mom = torch.zeros(D, device=dev)
    row = torch.randn(D, generator=gen, device=dev) * 1e-3
    row16 = row.to(torch.bfloat16)
    pout = torch.empty(D, dtype=torch.bfloat16, device=dev)
    T = len(sizes)
    adapt = torch.ones(T, dtype=torch.uint8, device=dev)
    q = torch.ones(T, device=dev)
    stats = torch.zeros(T, K.LARS_STATS, dtype=torch.float64, device=dev)
    pairs = torch.zeros(T, 2, dtype=torch.float64, device=dev)
    opt = K.OptArgs(kind="lars", lr=1e-3, momentum=0.9, weight_decay=1e-4)
    sgd = K.OptArgs(kind="sgd", lr=1e-3, momentum=0.9, weight_decay=1e-4)
    plans = {c: K.lars_plan(starts, sizes, chunk=c, total=D) for c in chunks}
    fns = {}
    for c, plan in plans.items():
        fns[f"norm_f32_C{c}"] = lambda plan=plan: K.seg_sq_norm(master, row, 1.0, plan, out=pairs)
        fns[f"norm_bf16_C{c}"] = lambda plan=plan: K.seg_sq_norm(master, row16, 1.0, plan,
                                                                 out=pairs)

        def staged(plan=plan):
            K.seg_sq_norm(master, row, 1.0, plan, out=pairs)
            K.lars_ratio(pairs, adapt, 0.001, 1e-4, 0.0, q, stats)
            K.lars_update(row, 1.0, plan, q, opt, master, mom, segs=[(pout, 0, D)])
        fns[f"staged_C{c}"] = staged
    p0 = plans[chunks[0]]
    fns["update"] = lambda: K.lars_update(row, 1.0, p0, q, opt, master, mom,
                                          segs=[(pout, 0, D)])
    fns["sgd_kernel"] = lambda: K.agg_update(row, combine="weighted", n=1, opt=sgd, master=master,
                                             s1=mom, param_out=pout)
    t = alternate(fns, reps)
    res = {"mode": "sweep", "D": D, "cut": cut, "tensors": T, "byte_ratio": round(30 / 22, 3)}
    for k, (med, lo, hi) in t.items():
        res[f"{k}_ms"] = med
        res[f"{k}_spread_ms"] = round(hi - lo, 4)
    for c in chunks:
        res[f"norm_f32_C{c}_GBps"] = round(8 * D / (t[f"norm_f32_C{c}"][0] * 1e-3) / 1e9, 1)
        res[f"norm_bf16_C{c}_GBps"] = round(6 * D / (t[f"norm_bf16_C{c}"][0] * 1e-3) / 1e9, 1)
        res[f"staged_C{c}_over_sgd"] = round(t[f"staged_C{c}"][0] / t["sgd_kernel"][0], 3)
    res["update_GBps"] = round(22 * D / (t["update"][0] * 1e-3) / 1e9, 1)
    res["sgd_kernel_GBps"] = round(22 * D / (t["sgd_kernel"][0] * 1e-3) / 1e9, 1)
    return res


def math_prod(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*", default=["resnet50", "bert_base"])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--D", type=int, nargs="*", default=[25_557_032, 109_514_304])
    ap.add_argument("--chunks", type=int, nargs="*",
                    default=[4096, 8192, 16384, 32768, 65536, 131072, 262144])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.sweep:
        cases = [lambda D=D, cut=cut: run_sweep(D, cut, a.chunks, a.reps, dev)
                 for D in a.D for cut in ("one", "resnet50")]
    else:
        cases = [lambda m=m: run_steps(m, a.reps, dev) for m in a.models]
    for case in cases:
        line = json.dumps(case())
        print(line, flush=True)
        if a.json_out:
            with open(a.json_out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
