#!/usr/bin/env python3
"""What optim.clip_norm adds to a training step: the whole step (host clock around 30 steps ending
in a synchronise) and engine.step() alone (HIP events and host clock, medians), with clip_norm
0 / 1.0 / 0 / 1.0 in one process, for ResNet-50 and BERT-base with 8 virtual workers. One JSON
line per run.

  python tools/diag/clip_step_probe.py
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from consensusml_amd import TrainConfig
from consensusml_amd.parallel.dist import DistInfo
from consensusml_amd.trainer.trainer import ConsensusTrainer

def run(clip, model):
    cfg = TrainConfig()
    if model == "resnet50":
        cfg.override("model.name=resnet50 model.num_classes=1000 batch_per_worker=32 virtual_workers=8 agg.rule=krum agg.f=2 topology.kind=sharded".split())
    else:
        cfg.override("model.name=bert_base model.seq_len=128 batch_per_worker=8 virtual_workers=8 agg.rule=median agg.f=2 topology.kind=sharded optim.name=adamw optim.lr=0.0001".split())
    cfg.optim.clip_norm = clip
    dev = torch.device("cuda", 0)
    tr = ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, dev, "none"))
    e = tr.engine
    orig = e.step
    ev, host = [], []
    def timed():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter(); a.record(); orig(); b.record(); host.append(time.perf_counter() - t); ev.append((a, b))
    e.step = timed
    for _ in range(8):
        tr.train_step()
    torch.cuda.synchronize(); ev.clear(); host.clear()
    t0 = time.perf_counter()
    for _ in range(30):
        tr.train_step()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / 30 * 1e3
    dev_ms = sorted(a.elapsed_time(b) for a, b in ev)[15]
    host_ms = sorted(host)[15] * 1e3
    out = {"model": model, "clip": clip, "ms_per_step": round(wall, 3), "engine_step_device_ms": round(dev_ms, 4),
           "engine_step_host_ms": round(host_ms, 4), "buckets": len(e.flat.buckets)}
    print(json.dumps(out), flush=True)
    tr.close()
    del tr
    torch.cuda.empty_cache()

for model in ("resnet50", "bert"):
    for clip in (0.0, 1.0, 0.0, 1.0):
        run(clip, model)
