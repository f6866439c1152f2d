#!/usr/bin/env python3
"""Head-dim-64 flash attention from the fused QKV layout (csrc/kernels/flash_attn64.hip) vs what
``fused_qkv_attention`` ran for the same call before it: qkv_split (three head-major copies) +
ROCm SDPA (AOTriton) + the output's transpose / reshape copy, and autograd's backward of that
composition (the gather of dq / dk / dv into the fused layout included) -- the copies are part of
what is replaced, so they are timed.

One JSON line per (shape, impl, pass): ms per call (median over --rounds interleaved rounds of the
median of --iters HIP-event timings) and TFLOP/s of useful attention work (forward 4 B H S^2 hd,
halved when causal; backward 2.5x). ``flash64_nq1`` / ``flash64_nq2`` force the forward's form
(32 / 64 queries per wave; ``flash64`` lets the launcher choose); their backward is the same one.

  python bench/flash_attn64.py                 # BERT-base 256 / 384 / 512 + causal 1024
  python bench/flash_attn64.py --impl flash64_nq1,flash64_nq2 --bscale 4
  python bench/flash_attn64.py --lens          # padded batches: the kernels' length variants

``--lens``: 12 heads, 8192 tokens at S = 128 / 256 / 512, non-causal, four settings per shape:
``none`` (no lengths), ``full`` (lens all S: the cost of the variant), ``ragged`` (lengths uniform
in [S/2, S], fixed seed: the work padding no longer costs) and ``sdpa_mask`` (qkv_split + SDPA
under a key-padding mask on the same lengths, what a padded batch runs without the kernels).
TFLOP/s there counts the full-length work, so it is comparable across the settings of a shape.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [  # B, H, S, causal: BERT-base at 8192 tokens per step, and one causal line
    (32, 12, 256, False),
    (21, 12, 384, False),
    (16, 12, 512, False),
    (8, 12, 1024, True),
]


def timed(fn, iters, warmup, calls):
    """Median ms per call over ``iters`` event pairs, each around ``calls`` back-to-back calls (the
    queue stays full, so a composition of several launches is not charged its launch latency)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    ts.sort()
    return ts[len(ts) // 2]


def lens_fns(L, a):
    """((B, H, S, causal), {setting: (fwd, bwd)}) per shape of the --lens mode; a shape's closures
    are timed before the next shape rebinds their tensors."""
    from consensusml_amd.ops.transformer import _lens_attention
    H, hd = 12, 64
    scale = hd ** -0.5
    for S in (128, 256, 512):
        B = 8192 // S * a.bscale
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3 * H * hd, device="cuda", generator=g).bfloat16()
        do = torch.randn(B, S, H * hd, device="cuda", generator=g).bfloat16()
        full = torch.full((B,), S, dtype=torch.int32, device="cuda")
        ragged = torch.randint(S // 2, S + 1, (B,), device="cuda", generator=g).int()
        fns = {}
        for name, lens in (("none", None), ("full", full), ("ragged", ragged)):
            o, lse = L.flash64_fwd(qkv, H, False, scale, lens=lens)
            fns[name] = (lambda lens=lens: L.flash64_fwd(qkv, H, False, scale, lens=lens),
                         lambda o=o, lse=lse, lens=lens: L.flash64_bwd(qkv, o, do, lse, H, False,
                                                                       scale, lens=lens))
        x = qkv.clone().requires_grad_()
        run_f = lambda: _lens_attention(x, H, hd, False, ragged)   # noqa: E731
        y = run_f()
        fns["sdpa_mask"] = (run_f, lambda: torch.autograd.grad(y, (x,), do, retain_graph=True))
        yield (B, H, S, False), fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--bscale", type=int, default=1, help="multiply every shape's batch")
    ap.add_argument("--impl", default="flash64,sdpa")
    ap.add_argument("--lens", action="store_true", help="padded-batch settings (see above)")
    a = ap.parse_args()
    from consensusml_amd.ops.native import lib
    from consensusml_amd.ops.transformer import qkv_split
    L = lib()
    hd = 64
    scale = hd ** -0.5
    if a.lens:
        for shape, fns in lens_fns(L, a):
            report(a, *shape, fns)
        return
    for B, H, S, causal in SHAPES:
        B *= a.bscale
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3 * H * hd, device="cuda", generator=g).bfloat16()
        do = torch.randn(B, S, H * hd, device="cuda", generator=g).bfloat16()
        fns = {}
        for impl in a.impl.split(","):
            if impl.startswith("flash64"):
                nq = int(impl[-1]) if "_nq" in impl else 0
                o, lse = L.flash64_fwd(qkv, H, causal, scale, 8.0, nq)
                fns[impl] = (lambda nq=nq: L.flash64_fwd(qkv, H, causal, scale, 8.0, nq),
                             lambda o=o, lse=lse: L.flash64_bwd(qkv, o, do, lse, H, causal, scale))
            else:
                x = qkv.clone().requires_grad_()

                def run_f(x=x):
                    q, k, v = qkv_split(x, H, H, hd)
                    return F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(
                        1, 2).reshape(B, S, H * hd)
                out = run_f()
                fns[impl] = (run_f, lambda out=out, x=x: torch.autograd.grad(
                    out, (x,), do, retain_graph=True))
        report(a, B, H, S, causal, fns)


def report(a, B, H, S, causal, fns, hd=64):
    # interleaved rounds in one process (variants share the clock / thermal state)
    res = {(i, p): [] for i in fns for p in ("fwd", "bwd")}
    for _ in range(a.rounds):
        for impl, (fwd, bwd) in fns.items():
            for name, fn in (("fwd", fwd), ("bwd", bwd)):
                res[(impl, name)].append(timed(fn, a.iters, a.warmup, a.calls))
    fwd_flop = 4.0 * B * H * S * S * hd * (0.5 if causal else 1.0)
    for (impl, name), ts in res.items():
        ts.sort()
        med = ts[len(ts) // 2]
        flop = fwd_flop * (1.0 if name == "fwd" else 2.5)
        print(json.dumps({"bench": "flash_attn64", "impl": impl, "pass": name, "B": B,
                          "H": H, "S": S, "causal": causal, "ms": round(med, 4),
                          "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                          "rounds": a.rounds, "tflops": round(flop / med / 1e9, 1)}),
              flush=True)


if __name__ == "__main__":
    main()
