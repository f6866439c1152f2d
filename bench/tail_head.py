#!/usr/bin/env python3
"""A layer-1 recompute tail with the next block's conv1 inside (tail_head.hip) against the two
launches it replaces (conv1x1_bnres / conv1x1_cat_bnres, then conv1x1_bn_fwd on y), for the three
layer-1 pairs of ResNet-50, A/B in alternating child processes (CML_FUSED_TAIL_HEAD = 0 / 1).

Each child times every pair with HIP events (median of --iters after warm-up, the operands rotated
over two sets, each far beyond the 256 MB last-level cache). The parent first measures the HBM
stream rates (bench/hbm_rates.py) and prints, per pair, both paths' times next to the fused byte
count at the copy (1 read : 1 write) rate. A pair counts as faster only if the new median beats
the old by more than the old path's own spread (max - min) over the alternations.

  python bench/tail_head.py --batch 2560 256 --alternations 3     # markdown table + JSON lines
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

H = 56
# (name, tail kind, p')
PAIRS = [
    ("layer1.0 down tail -> layer1.1 conv1 (256->64)", "down", 64),
    ("layer1.1 identity tail -> layer1.2 conv1 (256->64)", "identity", 64),
    ("layer1.2 identity tail -> layer2.0 conv1 (256->128)", "identity", 128),
]


def model_bytes(M, kind, p2):
    """(two launches, fused) bytes, U = M x 64 ch x 2 B: the tail reads z2 (+ x, or the 4 U
    residual) and writes y (4 U), the mask (U / 4) and z1n (p' / 64 U); as two launches y is read
    back (4 U)."""
    U = M * 64 * 2
    fused = (2 * U if kind == "down" else 5 * U) + 4 * U + U // 4 + p2 // 64 * U
    return fused + 4 * U, fused


def child(a):
    import torch
    from consensusml_amd.ops.native import lib
    L = lib()
    fused = os.environ.get("CML_FUSED_TAIL_HEAD", "1") == "1"
    dev = torch.device("cuda", 0)
    g0 = torch.Generator(device=dev).manual_seed(0)
    nhwc = lambda t: t.contiguous(memory_format=torch.channels_last)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g0)
    for B in a.batch:
        for name, kind, p2 in PAIRS:
            M = B * H * H
            sets = []
            for _ in range(2):
                d = {"z": nhwc(rn(B, 64, H, H).bfloat16())}
                if kind == "down":
                    d["x"] = nhwc(rn(B, 64, H, H).relu_().bfloat16())
                else:
                    d["res"] = nhwc(rn(B, 256, H, H).relu_().bfloat16())
                sets.append(d)
            sc = torch.rand(64, device=dev, generator=g0) + 0.5
            bi = rn(64) * 0.1
            esc = torch.ones(256, device=dev) if kind == "down" else \
                torch.rand(256, device=dev, generator=g0) + 0.5
            ebi = rn(256) * 0.1
            K = 128 if kind == "down" else 64
            w = (rn(256, K) * K ** -0.5).bfloat16()
            if kind == "identity":
                w = w.view(256, 64, 1, 1)
            w1n = (rn(p2, 256, 1, 1) * 256 ** -0.5).bfloat16()
            rm, rv = torch.zeros(p2, device=dev), torch.ones(p2, device=dev)

            def run(d):
                if fused and kind == "down":
                    return L.conv1x1_cat_bnres_head(d["z"], d["x"], sc, bi, w, esc, ebi, w1n, rm,
                                                    rv, 1e-5, 0.1)
                if fused:
                    return L.conv1x1_bnres_head(d["z"], w, sc, bi, esc, ebi, d["res"], w1n, rm, rv,
                                                1e-5, 0.1)
                if kind == "down":
                    y, m = L.conv1x1_cat_bnres(d["z"], d["x"], sc, bi, None, None, w, esc, ebi)
                else:
                    y, m = L.conv1x1_bnres(d["z"], w, sc, bi, esc, ebi, d["res"])
                return (y, m) + tuple(L.conv1x1_bn_fwd(y, w1n, None, None, rm, rm, rv, 1, True,
                                                       1e-5, 0.1))

            for i in range(3):
                run(sets[i % 2])
            torch.cuda.synchronize()
            ts = []
            for i in range(a.iters):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                run(sets[i % 2])
                e.record()
                torch.cuda.synchronize()
                ts.append(s.elapsed_time(e) * 1e3)
            print(json.dumps({"pair": name, "kind": kind, "p2": p2, "batch": B, "M": M,
                              "fused": int(fused), "us": round(statistics.median(ts), 1),
                              "min_us": round(min(ts), 1)}), flush=True)
            del sets
            torch.cuda.empty_cache()


def _spawn(args, env):
    r = subprocess.run([sys.executable, *args], env=env, capture_output=True, text=True,
                       cwd=ROOT, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child failed ({r.returncode}): {args}")
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[2560, 256])
    ap.add_argument("--iters", type=int, default=20, help="timed launches per pair (>= 20)")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    base = dict(os.environ, PYTHONPATH=ROOT)
    rates = {r["case"]: r["tb_s"] for r in
             _spawn([os.path.join(ROOT, "bench", "hbm_rates.py")], base)}
    print(json.dumps({"hbm_tb_s": rates}), flush=True)
    rate = rates["copy"]
    me = [os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--batch",
          *[str(b) for b in a.batch]]
    runs = {"0": [], "1": []}
    for _ in range(a.alternations):
        for flag in ("0", "1"):
            rows = _spawn(me, dict(base, CML_FUSED_TAIL_HEAD=flag))
            runs[flag].append({(r["pair"], r["batch"]): r for r in rows})
            for r in rows:
                print(json.dumps(r), flush=True)
    print("\n| pair | batch | bytes 2 launches -> fused (GB) | fused floor us | 2 launches us (runs) "
          "| fused us (runs) | old spread | verdict |\n|---|---|---|---|---|---|---|---|")
    for B in a.batch:
        for name, kind, p2 in PAIRS:
            old = [r[(name, B)]["us"] for r in runs["0"]]
            new = [r[(name, B)]["us"] for r in runs["1"]]
            b2, b1 = model_bytes(B * H * H, kind, p2)
            floor = b1 / (rate * 1e12) * 1e6
            spread = max(old) - min(old)
            gain = statistics.median(old) - statistics.median(new)
            verdict = f"fused, {gain:.0f} us faster" if gain > spread \
                else "NOT faster beyond the old path's spread: keep the two launches"
            print(f"| {name} | {B} | {b2 / 1e9:.2f} -> {b1 / 1e9:.2f} | {floor:.0f} | "
                  f"{statistics.median(old):.0f} ({', '.join(f'{v:.0f}' for v in old)}) | "
                  f"{statistics.median(new):.0f} ({', '.join(f'{v:.0f}' for v in new)}) | "
                  f"{spread:.0f} | {verdict} |")


if __name__ == "__main__":
    main()
