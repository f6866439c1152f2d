#!/usr/bin/env python3
"""Micro-benchmark of the aggregation hot path at ResNet-50 / BERT sizes on one MI355X.

For n workers x D coordinates (bf16), times (HIP events, median of reps):
  gram           G = X X^T (MFMA split-K + fp64 reduce)
  weights        Krum / Weiszfeld weights on G (one wave)
  median_sgd     coordinate median fused with SGD-momentum (master, momentum, bf16 params)
  trimmed_sgd    trimmed mean (trim f) fused with SGD-momentum
  meamed_sgd / phocas_sgd  the n - f values nearest to the median / to the trimmed mean per
                 coordinate (f at least 1), fused with SGD-momentum, and their ratio to median_sgd
  krum_sgd       weighted combine (one-hot Krum weights: 1 row read) fused with SGD-momentum
  mean_sgd       weighted combine of all n rows fused with SGD-momentum
  --mixed adds   nnm_matrix (the mixing matrix from G, one wave) and median_mixed_sgd /
                 trimmed_mixed_sgd: the same fused updates with the nearest-neighbour pre-mix
                 y = M x per coordinate ahead of the sort (agg.pre=nnm), and their ratio to the
                 plain sorted kernels from the same process; meamed_mixed_sgd / phocas_mixed_sgd likewise
  --worker-momentum  times only worker_momentum (m <- beta m + g in place over [n, D], the rows
                 replaced by bf16(m); optim.worker_momentum) and reports bytes / time with the
                 12 B per element the kernel must move (2 + 4 read, 2 + 4 written)
and the PyTorch equivalents (torch.median / sort / matmul / foreach) for comparison. Reports
achieved HBM GB/s from the bytes each kernel must move. One JSON line per (n, D).
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
    ap.add_argument("--n", type=int, nargs="*", default=[4, 8, 16])
    # ResNet-50 / BERT-base parameter counts, rounded up to the engine's 64-element bucket padding
    # (a row stride that is not a multiple of 8 bf16 would make gram() copy X to a padded buffer)
    ap.add_argument("--D", type=int, nargs="*", default=[25_557_032, 109_514_304])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--mixed", action="store_true",
                    help="also time the mixed sorted kernel (agg.pre=nnm) next to the plain one")
    ap.add_argument("--worker-momentum", action="store_true",
                    help="time only the worker-momentum kernel (optim.worker_momentum) over "
                         "[n, D]; use --n 1 8")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    from consensusml_amd.ops import kernels as K
    dev = torch.device("cuda", 0)
    for D in a.D:
        for n in a.n:
            g = torch.Generator(device=dev).manual_seed(0)
            X = torch.randn(n, D, generator=g, device=dev).to(torch.bfloat16)
            if a.worker_momentum:
                # in place over [n, D]: bf16 row read + written, fp32 state read + written
                state = torch.zeros(n, D, device=dev)
                ms = timeit(lambda: K.worker_momentum(X, state, 0.9), a.reps)
                res = {"n": n, "D": D, "dtype": "bf16", "worker_momentum_ms": round(ms, 4),
                       "worker_momentum_bytes": 12 * n * D,
                       "worker_momentum_GBps": round(12 * n * D / (ms * 1e-3) / 1e9, 1)}
                if not a.no_torch:   # the reference op: three elementwise passes, 20 B / element
                    def torch_wm():
                        state.mul_(0.9).add_(X)
                        X.copy_(state)
                    res["torch_worker_momentum_ms"] = round(timeit(torch_wm, max(3, a.reps // 4)), 4)
                line = json.dumps(res)
                print(line, flush=True)
                if a.json_out:
                    with open(a.json_out, "a") as fh:
                        fh.write(line + "\n")
                del X, state
                continue
            master = torch.randn(D, device=dev)
            mom = torch.zeros(D, device=dev)
            p = torch.empty(D, dtype=torch.bfloat16, device=dev)
            opt = K.OptArgs(kind="sgd", lr=0.1, momentum=0.9)
            G = torch.empty(n, n, dtype=torch.float64, device=dev)
            w = torch.zeros(n, device=dev)
            f = max(0, (n - 3) // 2)
            res = {"n": n, "D": D, "dtype": "bf16"}
            res["gram_ms"] = timeit(lambda: K.gram(X, out=G), a.reps)
            # the engine's second, centered pass (rows relative to the medoid row)
            c = K.gram_center(G, n)
            res["gram_centered_ms"] = timeit(lambda: K.gram(X, out=G, center=c), a.reps)
            res["weights_krum_ms"] = timeit(lambda: K.robust_weights(G, "krum", n, f=f, w_out=w), a.reps)
            res["weights_geomed_ms"] = timeit(lambda: K.robust_weights(G, "geomed", n, iters=8, w_out=w), a.reps)
            lo, cnt = K.sorted_range("median", n)
            res["median_sgd_ms"] = timeit(lambda: K.agg_update(
                X, combine="sorted", lo=lo, cnt=cnt, opt=opt, master=master, s1=mom, param_out=p), a.reps)
            lo2, cnt2 = K.sorted_range("trimmed_mean", n, f if 2 * f < n else 0)
            res["trimmed_sgd_ms"] = timeit(lambda: K.agg_update(
                X, combine="sorted", lo=lo2, cnt=cnt2, opt=opt, master=master, s1=mom, param_out=p), a.reps)
            fn = max(1, f)   # the nearest-to-centre rules at f = 0 are the mean
            near = {r: K.near_range(r, n, fn) for r in ("meamed", "phocas")} if 2 * fn < n else {}
            for r, (lo3, cnt3, keep3) in near.items():
                res[f"{r}_sgd_ms"] = timeit(lambda: K.agg_update(
                    X, combine="sorted", lo=lo3, cnt=cnt3, keep=keep3, opt=opt, master=master,
                    s1=mom, param_out=p), a.reps)
                res["near_f"] = fn
            if a.mixed:
                K.gram(X, out=G)
                fm = max(0, (n - 1) // 3)
                M = torch.empty(n, n, device=dev)
                res["nnm_matrix_ms"] = timeit(lambda: K.robust_weights(
                    G, "nnm_only", n, f=fm, w_out=w, pre="nnm", mix_out=M), a.reps)
                res["nnm_f"] = fm
                res["median_mixed_sgd_ms"] = timeit(lambda: K.agg_update(
                    X, combine="sorted", lo=lo, cnt=cnt, opt=opt, master=master, s1=mom,
                    param_out=p, mix=M), a.reps)
                res["trimmed_mixed_sgd_ms"] = timeit(lambda: K.agg_update(
                    X, combine="sorted", lo=lo2, cnt=cnt2, opt=opt, master=master, s1=mom,
                    param_out=p, mix=M), a.reps)
                for r, (lo3, cnt3, keep3) in near.items():
                    res[f"{r}_mixed_sgd_ms"] = timeit(lambda: K.agg_update(
                        X, combine="sorted", lo=lo3, cnt=cnt3, keep=keep3, opt=opt, master=master,
                        s1=mom, param_out=p, mix=M), a.reps)
            K.robust_weights(G, "krum", n, f=f, w_out=w)
            res["krum_sgd_ms"] = timeit(lambda: K.agg_update(
                X, combine="weighted", w=w, opt=opt, master=master, s1=mom, param_out=p), a.reps)
            wm = torch.full((n,), 1.0 / n, device=dev)
            res["mean_sgd_ms"] = timeit(lambda: K.agg_update(
                X, combine="weighted", w=wm, opt=opt, master=master, s1=mom, param_out=p), a.reps)
            # bytes that must move (HBM): X rows read, master+momentum read+write, params write
            state = D * (4 + 4) * 2 + D * 2
            gbs = lambda byt, ms: round(byt / (ms * 1e-3) / 1e9, 1)
            res["gram_GBps"] = gbs(n * D * 2, res["gram_ms"])
            res["gram_centered_GBps"] = gbs(n * D * 2, res["gram_centered_ms"])
            res["median_sgd_GBps"] = gbs(n * D * 2 + state, res["median_sgd_ms"])
            res["trimmed_sgd_GBps"] = gbs(n * D * 2 + state, res["trimmed_sgd_ms"])
            res["krum_sgd_GBps"] = gbs(D * 2 + state, res["krum_sgd_ms"])
            res["mean_sgd_GBps"] = gbs(n * D * 2 + state, res["mean_sgd_ms"])
            for r in near:
                res[f"{r}_sgd_GBps"] = gbs(n * D * 2 + state, res[f"{r}_sgd_ms"])
                res[f"{r}_over_median"] = round(res[f"{r}_sgd_ms"] / res["median_sgd_ms"], 3)
                if a.mixed:
                    res[f"{r}_mixed_over_median_mixed"] = round(
                        res[f"{r}_mixed_sgd_ms"] / res["median_mixed_sgd_ms"], 3)
            if a.mixed:
                for k in ("median", "trimmed"):
                    res[f"{k}_mixed_sgd_GBps"] = gbs(n * D * 2 + state, res[f"{k}_mixed_sgd_ms"])
                    res[f"{k}_mixed_over_plain"] = round(
                        res[f"{k}_mixed_sgd_ms"] / res[f"{k}_sgd_ms"], 3)
                # the mix: n^2 fp32 FMAs per coordinate
                res["median_mixed_mix_TFLOPs"] = round(
                    2.0 * n * n * D / (res["median_mixed_sgd_ms"] * 1e-3) / 1e12, 2)
            g2 = res["gram_ms"] + res["gram_centered_ms"]   # both Gram passes (engine default)
            res["krum_total_ms"] = round(g2 + res["weights_krum_ms"] + res["krum_sgd_ms"], 4)
            res["geomed_total_ms"] = round(g2 + res["weights_geomed_ms"] + res["mean_sgd_ms"], 4)
            if not a.no_torch:
                Xf = X
                res["torch_median_ms"] = timeit(lambda: torch.median(Xf, dim=0), max(3, a.reps // 4))
                res["torch_sort_ms"] = timeit(lambda: torch.sort(Xf, dim=0), max(3, a.reps // 4))
                res["torch_gram_ms"] = timeit(lambda: (Xf.float() @ Xf.float().t()), max(3, a.reps // 4))
            for k in list(res):
                if isinstance(res[k], float):
                    res[k] = round(res[k], 4)
            line = json.dumps(res)
            print(line, flush=True)
            if a.json_out:
                with open(a.json_out, "a") as fh:
                    fh.write(line + "\n")
            del X


if __name__ == "__main__":
    main()
