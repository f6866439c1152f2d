#!/usr/bin/env python3
"""What global-norm clipping (optim.clip_norm) costs on the update side, on one MI355X.

For n bf16 worker rows x D coordinates and the mean, median and Krum-weights rules, times (HIP
events, median of reps, as bench/agg_kernels.py):
  fused_ms      the rule fused with SGD-momentum: the step without clipping (the parent's path)
  stage1_ms     the same rule kernel with no optimizer, writing the fp32 aggregate (materialise)
  stage2_ms     sq_norm over the fp32 aggregate + clip_coef (norm, device weight)
  stage3_ms     the weighted kernel, n = 1, over the fp32 aggregate with the device weight
  staged_ms     stages 1 + 2 + 3 timed as ONE sequence (what a clipped step runs), and its ratio
                to fused_ms
and once per D, independent of the rule:
  sq_norm_f32 / sq_norm_bf16   sq_norm alone over one fp32 / bf16 row of D elements, with the
                achieved read bandwidth (4 D / 2 D bytes), per --grid-caps entry (0 = default)
  direct_*      the direct path (allreduce, gossip V = 1, FusedSGD): n = 1 fused update of one
                bf16 row against sq_norm(row) + clip_coef + the same update with the device weight
Compare the bandwidths with the one-pass copy rate tools/diag/hbm_copy.py reports on the same
box in the same session. One JSON line per D.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, reps: int = 20) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--D", type=int, nargs="*", default=[25_557_032, 109_514_304])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grid-caps", type=int, nargs="*", default=[0, 512, 2048, 4096, 8192])
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    from consensusml_amd.ops import kernels as K
    dev = torch.device("cuda", 0)
    n = a.n
    gbs = lambda byt, ms: round(byt / (ms * 1e-3) / 1e9, 1)    # noqa: E731
    for D in a.D:
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(n, D, generator=g, device=dev).to(torch.bfloat16)
        master = torch.randn(D, device=dev)
        mom = torch.zeros(D, device=dev)
        p = torch.empty(D, dtype=torch.bfloat16, device=dev)
        gout = torch.empty(D, device=dev)
        opt = K.OptArgs(kind="sgd", lr=0.1, momentum=0.9)
        none = K.OptArgs(kind="none")
        w_clip = torch.ones(1, device=dev)
        norm2 = torch.zeros(1, dtype=torch.float64, device=dev)
        stats = torch.zeros(K.CLIP_STATS, dtype=torch.float64, device=dev)
        work = K.sq_norm_workspace([gout])
        res = {"n": n, "D": D, "dtype": "bf16"}

        G = K.gram(X)
        wk = K.robust_weights(G, "krum", n, f=max(0, (n - 3) // 2))
        lo, cnt = K.sorted_range("median", n)
        rules = {"mean": dict(combine="weighted", w=torch.full((n,), 1.0 / n, device=dev)),
                 "median": dict(combine="sorted", lo=lo, cnt=cnt),
                 "krum": dict(combine="weighted", w=wk)}

        def stage2(row, scale, wsp):
            K.sq_norm([row], scale, wsp, norm2)
            K.clip_coef(norm2, 1.0, scale, w_clip, stats)

        def stage3(row):
            K.agg_update(row, combine="weighted", w=w_clip, n=1, opt=opt, master=master, s1=mom,
                         param_out=p)

        for name, kw in rules.items():
            fused = lambda: K.agg_update(X, opt=opt, master=master, s1=mom, param_out=p, **kw)  # noqa: E731
            s1 = lambda: K.agg_update(X, opt=none, gout=gout, **kw)                             # noqa: E731

            def staged():
                s1()
                stage2(gout, 1.0, work)
                stage3(gout)
            res[f"{name}_fused_ms"] = timeit(fused, a.reps)
            res[f"{name}_stage1_ms"] = timeit(s1, a.reps)
            res[f"{name}_staged_ms"] = timeit(staged, a.reps)
            res[f"{name}_staged_over_fused"] = round(res[f"{name}_staged_ms"]
                                                     / res[f"{name}_fused_ms"], 3)
        res["stage2_ms"] = timeit(lambda: stage2(gout, 1.0, work), a.reps)
        res["stage3_ms"] = timeit(lambda: stage3(gout), a.reps)
        # stage 3 moves: aggregate read, master + momentum read + write, bf16 parameters written
        res["stage3_GBps"] = gbs(D * (4 + 16 + 2), res["stage3_ms"])

        row = X[0]
        wrow = K.sq_norm_workspace([row])
        big = torch.empty(max(a.grid_caps + [2048]) + 16, dtype=torch.float64, device=dev)
        for cap in a.grid_caps:
            t = timeit(lambda: K.sq_norm([gout], 1.0, big, norm2, grid_cap=cap), a.reps)
            res[f"sq_norm_f32_cap{cap}_ms"] = t
            res[f"sq_norm_f32_cap{cap}_GBps"] = gbs(4 * D, t)
            t = timeit(lambda: K.sq_norm([row], 1.0, big, norm2, grid_cap=cap), a.reps)
            res[f"sq_norm_bf16_cap{cap}_ms"] = t
            res[f"sq_norm_bf16_cap{cap}_GBps"] = gbs(2 * D, t)

        def direct():
            stage2(row, 1.0 / n, wrow)
            stage3(row)
        res["direct_fused_ms"] = timeit(lambda: K.agg_update(
            row, combine="weighted", n=1, opt=K.OptArgs(kind="sgd", lr=0.1, momentum=0.9,
                                                        gscale=1.0 / n),
            master=master, s1=mom, param_out=p), a.reps)
        res["direct_clipped_ms"] = timeit(direct, a.reps)
        res["direct_clipped_over_fused"] = round(res["direct_clipped_ms"] / res["direct_fused_ms"], 3)
        for k in list(res):
            if isinstance(res[k], float):
                res[k] = round(res[k], 4)
        line = json.dumps(res)
        print(line, flush=True)
        if a.json_out:
            with open(a.json_out, "a") as fh:
                fh.write(line + "\n")
        del X, master, mom, p, gout


if __name__ == "__main__":
    main()
