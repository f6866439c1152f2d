#!/usr/bin/env python3
"""Document-masked flash attention (the DOC kernels of csrc/kernels/flash_attn.hip) vs the plain
causal kernels and ROCm SDPA under the equivalent boolean mask, at the Llama-3-8B layer shape.

One JSON line per (layout, pass): ms per call (median over --rounds of the median of --iters
after warmup, HIP events; the layouts are interleaved inside every round of one process) and
`ideal`, the layout's share of the causal score area, sum L_i^2 / S^2: the time a kernel with no
tile-granularity or ordering loss would take relative to one document per row.

Layouts: plain (no bounds), doc1 (bounds, one document per row), doc<L> (equal documents of L
tokens), mixed (lengths drawn uniformly in [64, S / 2] with --seed, the last one cut to fit; the
same row in every batch entry), sdpa<L> / sdpa_mixed (SDPA with attn_mask).

  python bench/flash_attn_docs.py --B 4 --S 2048
  python bench/flash_attn_docs.py --B 1 --S 8192
"""
import argparse
import json
import os
import random
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--KV", type=int, default=8)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--docs", default="1024,512,256", help="equal document lengths")
    ap.add_argument("--sdpa", default="512,mixed", help="layouts also run through SDPA ('' = none)")
    a = ap.parse_args()
    from consensusml_amd.ops.native import lib
    from consensusml_amd.ops.transformer import doc_bounds
    B, H, KV, S, D = a.B, a.H, a.KV, a.S, 128
    scale = D ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, H, S, D, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, KV, S, D, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, KV, S, D, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, S, H * D, device="cuda", generator=g).bfloat16()
    rng, mixed = random.Random(a.seed), []
    while sum(mixed) < S:
        mixed.append(min(rng.randint(64, S // 2), S - sum(mixed)))
    layouts = {"doc1": [S], "mixed": mixed}
    layouts.update({f"doc{n}": [int(n)] * (S // int(n)) + [S % int(n)] * (S % int(n) > 0)
                    for n in a.docs.split(",") if n})
    L = lib()
    o, lse = L.flash_fwd(q, k, v, True, scale)
    fns = {"plain": (lambda: L.flash_fwd(q, k, v, True, scale),
                     lambda: L.flash_bwd(q, k, v, o, do, lse, True, scale))}
    ideal = {"plain": 1.0}
    for name, lens in layouts.items():
        ids = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).cuda()
        ids = ids.expand(B, S)
        lo, hi = doc_bounds(ids)
        od, lsed = L.flash_fwd(q, k, v, True, scale, lo=lo)
        fns[name] = (lambda lo=lo: L.flash_fwd(q, k, v, True, scale, lo=lo),
                     lambda lo=lo, hi=hi, od=od, lsed=lsed: L.flash_bwd(q, k, v, od, do, lsed, True,
                                                                        scale, lo=lo, hi=hi))
        ideal[name] = sum(n * n for n in lens) / float(S * S)
        if name.replace("doc", "") in a.sdpa.split(","):
            pos = torch.arange(S, device="cuda")
            mask = ((lo[:, :, None] <= pos) & (pos <= pos[:, None]))[:, None]
            qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))

            def run_f(qa=qa, ka=ka, va=va, mask=mask):
                return F.scaled_dot_product_attention(qa, ka, va, attn_mask=mask, scale=scale,
                                                      enable_gqa=H != KV)
            out = run_f()
            dos = do.view(B, S, H, D).transpose(1, 2)
            sname = "sdpa" + name.replace("doc", "").replace("mixed", "_mixed")
            fns[sname] = (run_f, lambda out=out, qa=qa, ka=ka, va=va: torch.autograd.grad(
                out, (qa, ka, va), dos, retain_graph=True))
            ideal[sname] = ideal[name]
    # interleaved rounds in one process (variants share the clock / thermal state)
    res = {(i, p): [] for i in fns for p in ("fwd", "bwd")}
    for _ in range(a.rounds):
        for impl, (fwd, bwd) in fns.items():
            for name, fn in (("fwd", fwd), ("bwd", bwd)):
                res[(impl, name)].append(timed(fn, a.iters, a.warmup)[0])
    for (impl, name), ts in res.items():
        ts.sort()
        print(json.dumps({"bench": "flash_attn_docs", "layout": impl, "pass": name, "B": B, "H": H,
                          "KV": KV, "S": S, "ms": round(ts[len(ts) // 2], 4),
                          "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                          "rounds": a.rounds, "ideal": round(ideal[impl], 4),
                          "mixed_lens": mixed if impl.endswith("mixed") else None}), flush=True)


if __name__ == "__main__":
    main()
