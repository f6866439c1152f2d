#!/usr/bin/env python3
"""Backward of a bottleneck's conv1 with bn1's apply pass inside (conv1_bwd.hip) against the three
launches it replaces (bn_bwd_apply + the link data gradient + the weight gradient), at the
ResNet-50 bench shapes, A/B in alternating child processes (CML_FUSED_CONV1_BWD = 0 / 1).

Each child times every shape with HIP events (median of --iters after warm-up, the operands
rotated over two sets, each far beyond the 256 MB last-level cache). The parent first measures the
HBM stream rates (bench/hbm_rates.py) and prints, per shape, both paths' times next to the fused
byte count / the 2-reads : 1-write rate. A shape counts as faster only if the new median beats
the old by more than the old path's own spread (max - min) over the alternations.

  python bench/conv1_bwd.py --batch 2560 --alternations 3       # markdown table + JSON lines
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

# (name, p, Cin, image side at 224 px input, link kind)
SHAPES = [
    ("layer1.1-2 256->64 masked", 64, 256, 56, "mask"),
    ("layer2.1-3 512->128 masked", 128, 512, 28, "mask"),
    ("layer2.0 256->128 s2 link", 128, 256, 56, "s2"),
]


def model_bytes(M, p, Cin, kind):
    """(three launches, fused) bytes: the issue's 17.25 / 14.25 Mp accounting."""
    mp, mc = M * p * 2, M * Cin * 2
    link = {"mask": mc + mc // 16, "s2": mc // 4, "none": 0}[kind]
    return 3 * mp + (mp + mc + link) + (mp + mc), 2 * mp + mc + link + mc


def child(a):
    import torch
    from consensusml_amd.models.resnet import own_wgrad_ok
    from consensusml_amd.ops import conv as fconv
    from consensusml_amd.ops.native import lib
    L = lib()
    fused = os.environ.get("CML_FUSED_CONV1_BWD", "1") == "1"
    dev = torch.device("cuda", 0)
    g0 = torch.Generator(device=dev).manual_seed(0)
    nhwc = lambda t: t.contiguous(memory_format=torch.channels_last)
    for name, p, Cin, H, kind in SHAPES:
        B, M = a.batch, a.batch * H * H
        sets = []
        for _ in range(2):
            d = {"dy": nhwc(torch.randn(B, p, H, H, device=dev, generator=g0).bfloat16()),
                 "z": nhwc(torch.randn(B, p, H, H, device=dev, generator=g0).bfloat16()),
                 "x": nhwc(torch.randn(B, Cin, H, H, device=dev, generator=g0).bfloat16())}
            if kind == "mask":
                d["g"] = nhwc(torch.randn(B, Cin, H, H, device=dev, generator=g0).bfloat16())
                d["m"] = torch.randint(0, 256, (M, Cin // 8), device=dev, generator=g0,
                                       dtype=torch.uint8)
            else:
                d["g"] = nhwc(torch.randn(B, Cin, H // 2, H // 2, device=dev,
                                          generator=g0).bfloat16())
            sets.append(d)
        w = (torch.randn(p, Cin, 1, 1, device=dev, generator=g0) * Cin ** -0.5).bfloat16()
        w2, wt = w.view(p, Cin), w.view(p, Cin).t().contiguous()
        gamma = (torch.rand(p, device=dev, generator=g0) + 0.5).bfloat16()
        beta = (torch.randn(p, device=dev, generator=g0) * 0.1).bfloat16()
        mean = torch.zeros(p, device=dev)
        invstd = torch.ones(p, device=dev)
        s1 = torch.randn(p, device=dev, generator=g0) * M ** 0.5
        q1 = torch.randn(p, device=dev, generator=g0) * M ** 0.5
        own = own_wgrad_ok(Cin, p)

        def run(d):
            if fused:
                kw = dict(link=d["g"], lmask=d["m"]) if kind == "mask" \
                    else dict(link=d["g"], link_s2=True)
                return L.conv1_bn_bwd(d["dy"], d["z"], gamma, beta, mean, invstd, s1, q1, d["x"],
                                      w2, torch.bfloat16, **kw)
            dz = L.bn_bwd_apply(d["dy"], d["z"], gamma, beta, mean, invstd, s1, q1)
            dw = fconv._wgrad(dz, d["x"], w, 1, own)
            dx = L.conv1x1_link(dz, wt, d["g"], d["m"])[0] if kind == "mask" \
                else L.conv1x1_link_s2(dz, wt, d["g"])
            return dx, dw

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
        print(json.dumps({"shape": name, "p": p, "Cin": Cin, "M": M, "link": kind,
                          "fused": int(fused), "own_wgrad": bool(own),
                          "us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1)}),
              flush=True)
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
    ap.add_argument("--batch", type=int, default=2560)
    ap.add_argument("--iters", type=int, default=20, help="timed launches per shape (>= 20)")
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
    rate = rates["add_2r1w"]
    me = [os.path.abspath(__file__), "--child", "--batch", str(a.batch), "--iters", str(a.iters)]
    runs = {"0": [], "1": []}
    for _ in range(a.alternations):
        for flag in ("0", "1"):
            rows = _spawn(me, dict(base, CML_FUSED_CONV1_BWD=flag))
            runs[flag].append({r["shape"]: r for r in rows})
            for r in rows:
                print(json.dumps(r), flush=True)
    print("\n| shape | M | bytes 3 launches -> fused (GB) | fused floor us | 3 launches us (runs) | "
          "fused us (runs) | old spread | verdict |\n|---|---|---|---|---|---|---|---|")
    for name, p, Cin, H, kind in SHAPES:
        old = [r[name]["us"] for r in runs["0"]]
        new = [r[name]["us"] for r in runs["1"]]
        M = a.batch * H * H
        b3, b1 = model_bytes(M, p, Cin, kind)
        floor = b1 / (rate * 1e12) * 1e6
        spread = max(old) - min(old)
        gain = statistics.median(old) - statistics.median(new)
        verdict = f"fused, {gain:.0f} us faster" if gain > spread \
            else "NOT faster beyond the old path's spread: keep the three launches"
        print(f"| {name} | {M} | {b3 / 1e9:.2f} -> {b1 / 1e9:.2f} | {floor:.0f} | "
              f"{statistics.median(old):.0f} ({', '.join(f'{v:.0f}' for v in old)}) | "
              f"{statistics.median(new):.0f} ({', '.join(f'{v:.0f}' for v in new)}) | "
              f"{spread:.0f} | {verdict} |")


if __name__ == "__main__":
    main()
