#!/usr/bin/env python3
"""LARS trust ratios under attack, on the GPU kernels: ``resnet_tiny`` with Krum over n = 8
virtual workers (f = 2), clean and with two workers sending scaled gradients (fault.kind=scaled),
for optim.name=lars and optim.name=sgd. Prints one JSON line per run -- final loss and, for
LARS, per-tensor q / wn / gn after the last step -- for the table of profiles/lars/README.md."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(name: str, attacked: bool, steps: int, dev) -> dict:
    from consensusml_amd import TrainConfig
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    cfg = TrainConfig()
    cfg.model.name = "resnet_tiny"
    cfg.model.num_classes = 10
    cfg.model.image_size = 32
    cfg.batch_per_worker = 8
    cfg.virtual_workers = 8
    cfg.agg.rule = "krum"
    cfg.agg.f = 2
    cfg.topology.kind = "sharded"
    cfg.optim.name = name
    cfg.optim.momentum = 0.9
    cfg.optim.weight_decay = 1e-4
    cfg.optim.lr = 1.0 if name == "lars" else 0.05
    cfg.optim.trust_coef = 0.02
    if attacked:
        cfg.fault.kind = "scaled"
        cfg.fault.ranks = [0, 1]
        cfg.fault.scale = 100.0
    tr = ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, dev, "none"))
    losses = [float(tr.train_step()) for _ in range(steps)]
    res = {"optim": name, "attacked": attacked, "steps": steps, "first_loss": round(losses[0], 4),
           "final_loss": round(sum(losses[-3:]) / 3, 4),
           "krum_selected": tr.engine.sel_counts.tolist()}
    if name == "lars":
        st = tr.engine.lars_stats.cpu()
        names = tr.engine.flat.param_names()
        res["tensors"] = [{"name": n, "wn": round(float(r[0]), 5), "gn": float(f"{float(r[1]):.4g}"),
                           "q": float(f"{float(r[2]):.4g}")} for n, r in zip(names, st)]
        res["non_finite_steps"] = float(st[:, 3].sum())
    tr.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in ("lars", "sgd"):
        for attacked in (False, True):
            line = json.dumps(run(name, attacked, a.steps, dev))
            print(line, flush=True)
            if a.json_out:
                with open(a.json_out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
