"""The plain sorted combine must not move (not collected: no ``test_`` prefix).

``golden_calls`` runs a small fixed set of median and trimmed-mean updates (fp32 and bf16 rows,
n = 5, 8, 33, D = 523: vector body plus scalar tail, SGD with momentum and weight decay) through
``K.agg_update`` without ``keep`` and returns ``gout``, the master and ``param_out`` of each.
``tests/golden/meamed_plain_paths.pt`` holds these tensors as the commit BEFORE the
nearest-to-centre combine produced them on an MI355X:

    python tests/meamed_golden.py tests/golden/meamed_plain_paths.pt

run in a checkout of that commit (bea6069, with this file copied in). ``test_meamed_gpu.py``
compares bit for bit.
"""
import sys

import torch

CASES = [(dt, comb, n) for dt in ("f32", "bf16") for comb in ("median", "trimmed")
         for n in (5, 8, 33)]
D = 523


def _window(comb, n):
    if comb == "median":
        return ((n - 1) // 2, 1) if n % 2 else (n // 2 - 1, 2)
    lo = max(1, n // 4)
    return lo, n - 2 * lo


def golden_calls(K, dev):
    out = {}
    for i, (dt, comb, n) in enumerate(CASES):
        gen = torch.Generator().manual_seed(7000 + i)
        dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        X = torch.randn(n, D + 5, generator=gen).to(dtype).to(dev)
        master = torch.randn(D, generator=gen).to(dev)
        s1 = torch.randn(D, generator=gen).to(dev)
        gout = torch.empty(D, device=dev)
        pout = torch.empty(D, dtype=torch.bfloat16, device=dev)
        lo, cnt = _window(comb, n)
        K.agg_update(X, combine="sorted", lo=lo, cnt=cnt, n=n, D=D,
                     opt=K.OptArgs(kind="sgd", lr=0.05, momentum=0.9, weight_decay=0.01),
                     master=master, s1=s1, param_out=pout, gout=gout)
        key = f"{dt}-{comb}-n{n}"
        out[key + "-gout"] = gout.cpu()
        out[key + "-master"] = master.cpu()
        out[key + "-param_out"] = pout.cpu()
    return out


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from consensusml_amd.ops import kernels as K
    torch.save(golden_calls(K, torch.device("cuda:0")), sys.argv[1])
