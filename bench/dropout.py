#!/usr/bin/env python3
"""What fused dropout costs, and what it saves over composing ``F.dropout`` / SDPA, on one MI355X.

Everything alternates within every repetition (HIP events around forward + backward after a
warm-up of three calls each; median, min and max over the repetitions), at BERT-base's shapes:
  add_norm    8192 tokens x D 768, LayerNorm: the fused op at p = 0 and p = 0.1, and the unfused
              alternative ``add_norm(x, F.dropout(r, 0.1), ...)`` (a mask and a dropped copy of r
              written and re-read on both passes)
  attention   B 64 x 12 heads x S 128 x 64 from the fused QKV layout: attention.hip at p = 0 and
              p = 0.1, and head split + ``scaled_dot_product_attention(dropout_p=0.1)`` + the
              transpose back
  step        the bert_base training step of ``bench/configs.py --config bert_geomed`` (batch 64,
              seq 128, geometric median, AdamW) at model.dropout 0 and 0.1, one trainer per
              setting in one process, stepped in turn
  flash64     B x 12 heads x S x 64 at 16 x 512 and 32 x 256: the flash kernels of
              flash_attn64.hip at p = 0, their dropout instantiations at p = 0.1, and the head-split
              softmax composition (``_dropout_attention``: fp32 scores and a [B, H, S, S] mask
              materialised) that served these shapes before; then the same bert_base step at
              batch 16, seq 512. One JSON line per shape and one for the step
Two instances of the p = 0 setting run in every group ("p0" / "p0_again"): their difference is the
same-setting spread a difference between settings has to exceed. One JSON line per group.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lars_step import alternate  # noqa: E402


def _report(group: str, t: dict, **extra) -> dict:
    res = {"group": group, **extra}
    for k, (med, lo, hi) in t.items():
        res[f"{k}_ms"], res[f"{k}_min_ms"], res[f"{k}_max_ms"] = med, lo, hi
    res["spread_p0"] = round(abs(t["p0"][0] - t["p0_again"][0]) / t["p0"][0], 4)
    res["fused_p01_over_p0"] = round(t["fused_p01"][0] / t["p0"][0], 3)
    if "unfused_p01" in t:
        res["unfused_over_fused_p01"] = round(t["unfused_p01"][0] / t["fused_p01"][0], 3)
    return res


def run_add_norm(reps: int, dev) -> dict:
    from consensusml_amd.ops import transformer as T
    M, D = 8192, 768
    g = torch.Generator(device=dev).manual_seed(0)
    x, r, dy = (torch.randn(M, D, generator=g, device=dev).bfloat16() for _ in range(3))
    x.requires_grad_(True)
    r.requires_grad_(True)
    w = torch.ones(D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    b = torch.zeros(D, device=dev, dtype=torch.bfloat16, requires_grad=True)

    def fused(p):
        _, y = T.add_norm(x, r, w, b, 1e-12, dropout=p)
        torch.autograd.grad(y, (x, r, w, b), dy)

    def unfused():
        _, y = T.add_norm(x, F.dropout(r, 0.1), w, b, 1e-12)
        torch.autograd.grad(y, (x, r, w, b), dy)
    t = alternate({"p0": lambda: fused(0.0), "fused_p01": lambda: fused(0.1),
                   "unfused_p01": unfused, "p0_again": lambda: fused(0.0)}, reps)
    return _report("add_norm", t, tokens=M, D=D)


def run_attention(reps: int, dev) -> dict:
    from consensusml_amd.ops import transformer as T
    B, H, S, hd = 64, 12, 128, 64
    g = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(B, S, 3 * H * hd, generator=g, device=dev).bfloat16().requires_grad_(True)
    do = torch.randn(B, S, H * hd, generator=g, device=dev).bfloat16()

    def fused(p):
        torch.autograd.grad(T.fused_qkv_attention(qkv, H, hd, dropout=p), qkv, do)

    def sdpa():
        q, k, v = T.qkv_split(qkv, H, H, hd)
        o = F.scaled_dot_product_attention(q, k, v, dropout_p=0.1)
        torch.autograd.grad(o.transpose(1, 2).reshape(B, S, H * hd), qkv, do)
    t = alternate({"p0": lambda: fused(0.0), "fused_p01": lambda: fused(0.1),
                   "unfused_p01": sdpa, "p0_again": lambda: fused(0.0)}, reps)
    return _report("attention", t, B=B, H=H, S=S, hd=hd)


def run_step(reps: int, dev, batch=None, seq_len=None) -> dict:
    from configs import CONFIGS
    from consensusml_amd import TrainConfig
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    c = dict(CONFIGS["bert_geomed"])
    c["batch"], c["seq_len"] = batch or c["batch"], seq_len or c["seq_len"]

    def trainer(p):
        cfg = TrainConfig()
        cfg.model.name, cfg.model.seq_len, cfg.model.dropout = c["model"], c["seq_len"], p
        cfg.batch_per_worker, cfg.dtype = c["batch"], c["dtype"]
        cfg.agg.rule, cfg.topology.kind, cfg.topology.bucket_mb = c["rule"], c["topology"], c["bucket_mb"]
        cfg.optim.name, cfg.optim.lr = c["optim"], c["lr"]
        return ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, dev, "none"))
    trs = {"p0": trainer(0.0), "fused_p01": trainer(0.1), "p0_again": trainer(0.0)}
    t = alternate({k: tr.train_step for k, tr in trs.items()}, reps)
    return _report("step", t, config="bert_geomed", batch=c["batch"], seq_len=c["seq_len"])


def run_flash64(reps: int, dev) -> list:
    from consensusml_amd.ops import transformer as T
    H, hd, out = 12, 64, []
    for B, S in ((16, 512), (32, 256)):
        g = torch.Generator(device=dev).manual_seed(2)
        qkv = torch.randn(B, S, 3 * H * hd, generator=g, device=dev).bfloat16().requires_grad_(True)
        do = torch.randn(B, S, H * hd, generator=g, device=dev).bfloat16()

        def fused(p):
            torch.autograd.grad(T.fused_qkv_attention(qkv, H, hd, dropout=p), qkv, do)

        def composed():
            o = T._dropout_attention(qkv, H, hd, False, None, T._drop(0.1, True, None))
            torch.autograd.grad(o, qkv, do)
        t = alternate({"p0": lambda: fused(0.0), "fused_p01": lambda: fused(0.1),
                       "unfused_p01": composed, "p0_again": lambda: fused(0.0)}, reps)
        out.append(_report("flash64", t, B=B, H=H, S=S, hd=hd))
        torch.cuda.empty_cache()
    out.append(run_step(reps, dev, batch=16, seq_len=512))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", nargs="*", default=["add_norm", "attention", "step", "flash64"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    runs = {"add_norm": run_add_norm, "attention": run_attention, "step": run_step,
            "flash64": run_flash64}
    for grp in a.groups:
        res = runs[grp](a.reps, dev)
        for r in res if isinstance(res, list) else [res]:
            line = json.dumps(r)
            print(line, flush=True)
            if a.json_out:
                with open(a.json_out, "a") as fh:
                    fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
