#!/usr/bin/env python3
"""Gram passes of the recompute tails (ops.conv._RecomputeTailFn / _RecomputeDownTailFn) at the
ResNet-50 bench shapes: the one-read symmetric kernel (gram1x1.hip) against the weight-gradient
path (CML_GRAM_SYRK=0), A/B in alternating child processes.

Each child times every shape with HIP events (median of --iters launches after warm-up, the input
rotated over copies so a tensor near the last-level cache's size is not served from it). The parent
first measures the read-only HBM rate (bench/hbm_rates.py) and prints, per shape, both paths' times
next to bytes-read-once / that rate. A shape counts as faster only if the new median beats the
old by more than the old path's own spread (max - min) over the alternations.

  python bench/gram.py --batch 2560 --alternations 3            # markdown table + JSON lines
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, channels p, image side at 224 px input, BN + ReLU prologue)
SHAPES = [
    ("layer1 tail y2", 64, 56, True),
    ("layer2 tail y2", 128, 28, True),
    ("layer3 tail y2", 256, 14, True),
    ("layer1 down x", 64, 56, False),
    ("layer2 down x", 256, 28, False),
    ("layer3 down x", 512, 14, False),   # p = 512: not routed to the Gram kernel
]


def child(a):
    import torch
    from consensusml_amd.ops.native import lib
    L = lib()
    dev = torch.device("cuda", 0)
    g0 = torch.Generator(device=dev).manual_seed(0)
    for name, p, H, pro in SHAPES:
        M = a.batch * H * H
        ncopy = max(2, min(4, int(1.2e9 // (M * p * 2)) + 1))
        zs = [torch.randn(a.batch, p, H, H, device=dev, generator=g0).bfloat16().contiguous(
            memory_format=torch.channels_last) for _ in range(ncopy)]
        sc = torch.rand(p, device=dev, generator=g0) + 0.5
        bi = torch.randn(p, device=dev, generator=g0) * 0.1 + 0.2

        def run(z):
            if pro:
                return L.wgrad1x1_ex(z, z, sc, bi, 3, None, sc, bi, None, True)
            return L.wgrad1x1_ex(z, z, None, None, 0, None, None, None, None, True)

        for i in range(3):
            run(zs[i % ncopy])
        torch.cuda.synchronize()
        ts = []
        for i in range(a.iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run(zs[i % ncopy])
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) * 1e3)
        print(json.dumps({"shape": name, "p": p, "M": M, "pro": pro,
                          "syrk": os.environ.get("CML_GRAM_SYRK", "1"),
                          "us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1)}),
              flush=True)
        del zs
        torch.cuda.empty_cache()


def _spawn(args, env):
    r = subprocess.run([sys.executable, *args], env=env, capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child failed ({r.returncode}): {args}")
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2560)
    ap.add_argument("--iters", type=int, default=24, help="timed launches per shape (>= 20)")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    base = dict(os.environ, PYTHONPATH=ROOT)
    rate = next(r["tb_s"] for r in _spawn([os.path.join(ROOT, "bench", "hbm_rates.py")], base)
                if r["case"] == "read_sum")
    print(json.dumps({"read_only_tb_s": rate}), flush=True)
    me = [os.path.abspath(__file__), "--child", "--batch", str(a.batch), "--iters", str(a.iters)]
    runs = {"0": [], "1": []}
    for _ in range(a.alternations):
        for flag in ("0", "1"):
            rows = _spawn(me, dict(base, CML_GRAM_SYRK=flag))
            runs[flag].append({r["shape"]: r for r in rows})
            for r in rows:
                print(json.dumps(r), flush=True)
    print("\n| shape | p | M | read-once floor us | old us (runs) | new us (runs) | old spread | "
          "verdict |\n|---|---|---|---|---|---|---|---|")
    for name, p, H, pro in SHAPES:
        old = [r[name]["us"] for r in runs["0"]]
        new = [r[name]["us"] for r in runs["1"]]
        M = a.batch * H * H
        floor = M * p * 2 / (rate * 1e12) * 1e6
        spread = max(old) - min(old)
        gain = statistics.median(old) - statistics.median(new)
        if p > 256:
            verdict = "old path (p > 256 is not routed)"
        elif gain > spread:
            verdict = f"new kernel, {gain:.0f} us faster"
        else:
            verdict = "NOT faster beyond the old path's spread: keep on the old path"
        print(f"| {name}{' (BN+ReLU)' if pro else ''} | {p} | {M} | {floor:.0f} | "
              f"{statistics.median(old):.0f} ({', '.join(f'{v:.0f}' for v in old)}) | "
              f"{statistics.median(new):.0f} ({', '.join(f'{v:.0f}' for v in new)}) | "
              f"{spread:.0f} | {verdict} |")


if __name__ == "__main__":
    main()
