"""The whole dispatch space of ``agg_update.hip`` must not move (not collected: no ``test_``
prefix).

``golden_calls`` runs one small update per kernel form through ``K.agg_update`` and
``K.agg_update_multi`` (SGD with momentum 0.9 and weight decay 0.01, a bf16 ``param_out``, seeded
``randn`` inputs) and returns ``gout``, the master and ``param_out`` of each:

* single segment, D = 131 (vectors of 8, 4 or 2 elements plus a scalar tail of 3 or 1), fp32 and
  bf16 rows: the nearest-to-centre combine (n = 5, 8, 33; the median and the trimmed window as
  centre; f = max(1, n // 4), keep = n - f), the mixed and the nearest-mixed combine (n = 3, 5,
  12, 17, padding to 4, 8, 16 and 32 rows; a row-stochastic fp32 ``mix`` with exact zeros) and the
  weighted combine (n = 8 with one zero weight: seven rows, a group of four and a remainder of
  three; n = 5 with ``w=None``);
* several segments of (64, 16, 136) elements in one launch at n = 5, one case per form and row
  type, and one whose middle segment has 131 elements (one launch per segment).

``tests/golden/agg_dispatch_parent.pt`` holds these tensors as the commit BEFORE the dispatch
half of the file was folded into one table produced them on an MI355X:

    python tests/agg_dispatch_golden.py tests/golden/agg_dispatch_parent.pt

run in a checkout of that commit (8e39953, with this file copied in).
``test_agg_dispatch_gpu.py`` compares bit for bit. ``meamed_golden.py`` pins the plain sorted
combine in the same way.
"""
import sys

import torch

D = 131
SEGS = (64, 16, 136)
RAGGED = (64, 131, 136)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
FORMS = ("sorted", "near", "mixed", "near_mixed", "weighted")


def _window(centre, n, f):
    if centre == "median":
        return ((n - 1) // 2, 1) if n % 2 else (n // 2 - 1, 2)
    return f, n - 2 * f


def single_cases():
    """(key, dt, n, combine, centre, keep?, mix?, weights) of every single-segment case."""
    cases = []
    for dt in DTYPES:
        for n in (5, 8, 33):
            for centre in ("median", "trimmed"):
                cases.append((f"{dt}-near-{centre}-n{n}", dt, n, "sorted", centre, True, False, None))
        for n in (3, 5, 12, 17):
            cases.append((f"{dt}-mixed-n{n}", dt, n, "sorted", "median", False, True, None))
            cases.append((f"{dt}-near_mixed-n{n}", dt, n, "sorted", "trimmed", True, True, None))
        cases.append((f"{dt}-weighted-n8", dt, 8, "weighted", None, False, False, "one_zero"))
        cases.append((f"{dt}-weighted-n5", dt, 5, "weighted", None, False, False, None))
    return cases


def multi_cases():
    cases = [(f"{dt}-multi-{form}", dt, form, SEGS) for dt in DTYPES for form in FORMS]
    cases.append(("bf16-multi-near_mixed-ragged", "bf16", "near_mixed", RAGGED))
    return cases


def _mix(n, gen):
    M = torch.rand(n, n, generator=gen)
    M[torch.rand(n, n, generator=gen) < 0.3] = 0.0
    M += torch.eye(n)
    return (M / M.sum(1, keepdim=True)).float().contiguous()


def _rule(K, n, combine, centre, keep, mix, weights, gen, dev):
    """The keyword arguments of the rule shared by the single and the multi call."""
    f = max(1, n // 4)
    kw = {"combine": combine, "n": n,
          "opt": K.OptArgs(kind="sgd", lr=0.05, momentum=0.9, weight_decay=0.01)}
    if combine == "sorted":
        kw["lo"], kw["cnt"] = _window(centre, n, f)
        if keep:
            kw["keep"] = n - f
        if mix:
            kw["mix"] = _mix(n, gen).to(dev)
    elif weights == "one_zero":
        w = torch.rand(n, generator=gen) + 0.1
        w[3] = 0.0
        kw["w"] = w.to(dev)
    return kw


def _pack(out):
    """Every tensor of one dtype as a view of one storage: one record per dtype in the file."""
    for dtype in {t.dtype for t in out.values()}:
        keys = [k for k in out if out[k].dtype == dtype]
        flat = torch.cat([out[k].flatten() for k in keys])
        o = 0
        for k in keys:
            out[k] = flat[o:o + out[k].numel()]
            o += out[k].numel()
    return out


def golden_calls(K, dev):
    out = {}
    for i, (key, dt, n, combine, centre, keep, mix, weights) in enumerate(single_cases()):
        gen = torch.Generator().manual_seed(8000 + i)
        X = torch.randn(n, D + 5, generator=gen).to(DTYPES[dt]).to(dev)
        master = torch.randn(D, generator=gen).to(dev)
        s1 = torch.randn(D, generator=gen).to(dev)
        gout = torch.empty(D, device=dev)
        pout = torch.empty(D, dtype=torch.bfloat16, device=dev)
        K.agg_update(X, D=D, master=master, s1=s1, param_out=pout, gout=gout,
                     **_rule(K, n, combine, centre, keep, mix, weights, gen, dev))
        out[key + "-gout"] = gout.cpu()
        out[key + "-master"] = master.cpu()
        out[key + "-param_out"] = pout.cpu()
    for i, (key, dt, form, sizes) in enumerate(multi_cases()):
        gen = torch.Generator().manual_seed(8500 + i)
        n = 5
        offs, need = [], 0
        for d in sizes:
            offs.append(need)
            need += -(-d // 8) * 8     # every segment starts on the widest vector grid
        Xs = [torch.randn(n, -(-d // 8) * 8 + 8, generator=gen).to(DTYPES[dt]).to(dev)
              for d in sizes]
        master = torch.randn(need, generator=gen).to(dev)
        s1 = torch.randn(need, generator=gen).to(dev)
        gout = torch.zeros(need, device=dev)
        pouts = [torch.empty(d, dtype=torch.bfloat16, device=dev) for d in sizes]
        kw = _rule(K, n, "weighted" if form == "weighted" else "sorted", "median",
                   form.startswith("near"), form.endswith("mixed"), None, gen, dev)
        K.agg_update_multi(list(zip(Xs, sizes, offs, pouts)), master=master, s1=s1, gout=gout,
                           **kw)
        out[key + "-gout"] = gout.cpu()
        out[key + "-master"] = master.cpu()
        out[key + "-param_out"] = torch.cat(pouts).cpu()
    return _pack(out)


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from consensusml_amd.ops import kernels as K
    torch.save(golden_calls(K, torch.device("cuda:0")), sys.argv[1])
