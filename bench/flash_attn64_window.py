#!/usr/bin/env python3
"""Sliding-window head-dim-64 grouped-query flash attention (csrc/kernels/flash_attn64_gqa_win.hip)
on the Llama-3.2-1B layer (B 4, 32 q / 8 kv heads, S 2048 / 8192, W 256 / 1024 / 4096) on
head-major q / k / v: ``flash_fwd`` / ``flash_bwd`` with ``window=W`` against

  causal   the plain causal kernels of flash_attn64_gqa.hip at the same S (no window: the
           baseline the skipped tiles are measured against; window >= S routes there too),
  sdpa     ROCm SDPA under the equivalent boolean ``attn_mask`` (what a windowed head-dim-64
           layer ran before), forward and autograd's backward.

One JSON line per (S, W, impl, pass): ms per call (median over --rounds interleaved rounds of the
median of --iters HIP-event timings around --calls back-to-back calls), and for the window lines
``vs_causal`` (ms / the causal ms of the same S and pass, the mean of its two positions in the
round: ``causal`` first, ``causal_again`` after the window kernels) next to ``tiles`` (visited key tiles
over the causal kernel's, about (W + 128) / (S / 2)): the ratio the time is expected to follow.

  python bench/flash_attn64_window.py
  python bench/flash_attn64_window.py --seqs 8192 --windows 1024 --no-sdpa
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup, calls):
    """Median ms per call over ``iters`` event pairs, each around ``calls`` back-to-back calls."""
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


def tile_ratio(S, W):
    """Key tiles a query block visits under the window over the causal kernel's, summed over the
    blocks (128-row tiles)."""
    nb = (S + 127) // 128
    win = sum(qb - max(qb * 128 - W + 1, 0) // 128 + 1 for qb in range(nb))
    return win / (nb * (nb + 1) / 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="back-to-back calls per timed window")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--seqs", default="2048,8192")
    ap.add_argument("--windows", default="256,1024,4096")
    ap.add_argument("--no-sdpa", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/flash_attn64_window.py needs a GPU")
    from consensusml_amd.ops.native import lib
    L = lib()
    B, H, KV, hd = a.batch, a.heads, a.kv_heads, 64
    scale = hd ** -0.5
    wins = [int(w) for w in a.windows.split(",")]
    for S in (int(s) for s in a.seqs.split(",")):
        g = torch.Generator(device="cuda").manual_seed(0)
        mk = lambda h: torch.randn(B, h, S, hd, device="cuda", generator=g).bfloat16()  # noqa: E731
        q, k, v = mk(H), mk(KV), mk(KV)
        do = torch.randn(B, S, H * hd, device="cuda", generator=g).bfloat16()

        def ours(W):
            o, lse = L.flash_fwd(q, k, v, True, scale, window=W)
            return (lambda: L.flash_fwd(q, k, v, True, scale, window=W),
                    lambda: L.flash_bwd(q, k, v, o, do, lse, True, scale, window=W))

        fns = {("causal", 0): ours(0)}
        for W in wins:
            fns[("window", W)] = ours(W)
        # the baseline once more, after the window kernels: the two differ by position in the
        # round only, which is the noise floor any window / causal ratio is read against
        fns[("causal_again", 0)] = ours(0)
        if not a.no_sdpa:
            qs, ks, vs = (t.clone().requires_grad_() for t in (q, k, v))
            dos = do.view(B, S, H, hd).transpose(1, 2)
            pos = torch.arange(S, device="cuda")
            for W in wins:
                mask = (pos <= pos[:, None]) & (pos > pos[:, None] - W)
                f = lambda mask=mask: F.scaled_dot_product_attention(   # noqa: E731
                    qs, ks, vs, attn_mask=mask, scale=scale, enable_gqa=H != KV)
                y = f()
                fns[("sdpa", W)] = (f, lambda y=y: torch.autograd.grad(y, (qs, ks, vs), dos,
                                                                       retain_graph=True))
        # interleaved rounds in one process (variants share the clock / thermal state)
        res = {(i, p): [] for i in fns for p in ("fwd", "bwd")}
        for _ in range(a.rounds):
            for impl, pair in fns.items():
                for p, fn in zip(("fwd", "bwd"), pair):
                    res[(impl, p)].append(timed(fn, a.iters, a.warmup, a.calls))
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in res.items()}
        for ((impl, W), p), ts in res.items():
            line = {"bench": "flash_attn64_window", "impl": impl, "pass": p, "B": B, "H": H,
                    "KV": KV, "S": S, "W": W, "ms": round(med[((impl, W), p)], 4),
                    "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "rounds": a.rounds}
            if impl == "window":
                base = 0.5 * (med[(("causal", 0), p)] + med[(("causal_again", 0), p)])
                line["vs_causal"] = round(med[((impl, W), p)] / base, 3)
                line["tiles"] = round(tile_ratio(S, W), 3)
            print(json.dumps(line), flush=True)
        del fns, q, k, v, do
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
