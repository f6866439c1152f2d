#!/usr/bin/env python3
"""Head-dim-64 grouped-query flash attention (csrc/kernels/flash_attn64_gqa.hip) on the
Llama-3.2-1B layer (B 4, 32 q / 8 kv heads, causal, S 512 / 2048 / 8192) vs what ``qkv_attention``
ran for the same call before it: qkv_split (RoPE + three head-major copies) + ROCm SDPA (AOTriton,
enable_gqa) + the output's transpose / reshape copy, and autograd's backward of that composition.
Both sides start from the fused projection ``qkv [B, S, (H + 2 KV) 64]`` and end at
``o [B, S, H 64]`` / ``dqkv``, so the RoPE split and its backward are inside both timings: ``ours``
is ``_RopeFlashFn`` (rope_fwd + flash_fwd; flash_bwd + rope_bwd with grp = 1).

``attn`` lines time the attention kernels alone on head-major q / k / v: ``flash_fwd`` /
``flash_bwd`` (dQ + dK / dV with the group sum inside) against SDPA's forward / backward on the
same tensors (its backward returns group-summed dk / dv too).

One JSON line per (S, impl, pass): ms per call (median over --rounds interleaved rounds of the
median of --iters HIP-event timings around --calls back-to-back calls), TFLOP/s of useful
attention work (forward 4 B H S^2 hd / 2, backward 2.5x) and, for the backward, the peak device
memory of one call above what was allocated before it (``peak_mb``).

  python bench/flash_attn64_gqa.py
  python bench/flash_attn64_gqa.py --seqs 2048 --batch 8
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def peak_mb(fn):
    """Peak allocated bytes of one call above the level before it, in MiB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    del r
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="back-to-back calls per timed window")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--seqs", default="512,2048,8192")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/flash_attn64_gqa.py needs a GPU")
    from consensusml_amd.ops.native import lib
    from consensusml_amd.ops.transformer import _RopeFlashFn, _sdpa_rows, qkv_split, rope_tables
    L = lib()
    B, H, KV, hd = a.batch, a.heads, a.kv_heads, 64
    scale = hd ** -0.5
    for S in (int(s) for s in a.seqs.split(",")):
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, (H + 2 * KV) * hd, device="cuda", generator=g).bfloat16()
        do = torch.randn(B, S, H * hd, device="cuda", generator=g).bfloat16()
        cos, sin = rope_tables(S, hd, 500000.0, "cuda")
        fns = {}
        # the whole call, from the fused projection
        x = qkv.clone().requires_grad_()
        f_ours = lambda: _RopeFlashFn.apply(x, cos, sin, H, KV, True, scale)   # noqa: E731
        f_sdpa = lambda: _sdpa_rows(*qkv_split(x, H, KV, hd, cos, sin), True, scale)   # noqa: E731
        for name, f in (("ours", f_ours), ("sdpa", f_sdpa)):
            y = f()
            fns[name] = (f, lambda y=y: torch.autograd.grad(y, (x,), do, retain_graph=True))
        # the attention kernels alone, on head-major q / k / v
        q, k, v = L.rope_fwd(qkv, cos, sin, H, KV, hd)
        o, lse = L.flash_fwd(q, k, v, True, scale)
        fns["attn_ours"] = (lambda: L.flash_fwd(q, k, v, True, scale),
                            lambda: L.flash_bwd(q, k, v, o, do, lse, True, scale))
        qs, ks, vs = (t.clone().requires_grad_() for t in (q, k, v))
        f_attn = lambda: F.scaled_dot_product_attention(   # noqa: E731
            qs, ks, vs, is_causal=True, scale=scale, enable_gqa=H != KV)
        ys = f_attn()
        dos = do.view(B, S, H, hd).transpose(1, 2)
        fns["attn_sdpa"] = (f_attn, lambda: torch.autograd.grad(ys, (qs, ks, vs), dos,
                                                                retain_graph=True))
        # interleaved rounds in one process (variants share the clock / thermal state)
        res = {(i, p): [] for i in fns for p in ("fwd", "bwd")}
        for _ in range(a.rounds):
            for impl, pair in fns.items():
                for p, fn in zip(("fwd", "bwd"), pair):
                    res[(impl, p)].append(timed(fn, a.iters, a.warmup, a.calls))
        fwd_flop = 2.0 * B * H * S * S * hd
        for (impl, p), ts in res.items():
            ts.sort()
            med = ts[len(ts) // 2]
            line = {"bench": "flash_attn64_gqa", "impl": impl, "pass": p, "B": B, "H": H, "KV": KV,
                    "S": S, "causal": True, "ms": round(med, 4), "ms_min": round(ts[0], 4),
                    "ms_max": round(ts[-1], 4), "rounds": a.rounds,
                    "tflops": round(fwd_flop * (1.0 if p == "fwd" else 2.5) / med / 1e9, 1)}
            if p == "bwd":
                line["peak_mb"] = round(peak_mb(fns[impl][1]), 1)
            print(json.dumps(line), flush=True)
        del fns, x, q, k, v, o, lse, qs, ks, vs, ys, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
