"""The float64 oracle of ``agg_oracle.py`` against ``torch.optim`` (pins the oracle to something
outside the project), and the CPU branch of ``K.agg_update`` / ``K.agg_update_multi`` (which the
gloo configs run) against that oracle over the case table the GPU file uses."""
import pytest
import torch

import agg_oracle as AO
from consensusml_amd.ops import kernels as K

TORCH_OPTS = {
    "sgd_nesterov": (lambda p: torch.optim.SGD(p, lr=0.05, momentum=0.9, nesterov=True,
                                               weight_decay=0.01),
                     dict(kind="sgd", lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01)),
    "sgd_momentum": (lambda p: torch.optim.SGD(p, lr=0.05, momentum=0.9, weight_decay=0.01),
                     dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=0.01)),
    "sgd_m0": (lambda p: torch.optim.SGD(p, lr=0.05, momentum=0.0, weight_decay=0.01),
               dict(kind="sgd", lr=0.05, momentum=0.0, weight_decay=0.01)),
    "adam": (lambda p: torch.optim.Adam(p, lr=0.01, weight_decay=0.01),
             dict(kind="adam", lr=0.01, weight_decay=0.01)),
    "adamw": (lambda p: torch.optim.AdamW(p, lr=0.01, weight_decay=0.01),
              dict(kind="adamw", lr=0.01, weight_decay=0.01)),
}


@pytest.mark.parametrize("name", list(TORCH_OPTS))
def test_step64_matches_torch_optim(name):
    make, hyper = TORCH_OPTS[name]
    hyper = dict(hyper)
    kind = hyper.pop("kind")
    gen = torch.Generator().manual_seed(3)
    D = 257
    p_t = torch.randn(D, generator=gen, dtype=torch.float64).requires_grad_()
    opt = make([p_t])
    p = p_t.detach().clone()
    s1 = torch.zeros(D, dtype=torch.float64)
    s2 = torch.zeros(D, dtype=torch.float64)
    for step in (1, 2, 3):
        g = torch.randn(D, generator=gen, dtype=torch.float64)
        p_t.grad = g.clone()
        opt.step()
        p, s1, s2 = AO.step64(kind, p, g, s1, s2, first=step == 1, step=step, **hyper)
        torch.testing.assert_close(p, p_t.detach(), rtol=1e-12, atol=0)
    st = opt.state[p_t]
    if kind == "sgd" and hyper["momentum"]:
        torch.testing.assert_close(s1, st["momentum_buffer"], rtol=1e-12, atol=0)
    if kind != "sgd":
        torch.testing.assert_close(s1, st["exp_avg"], rtol=1e-12, atol=0)
        torch.testing.assert_close(s2, st["exp_avg_sq"], rtol=1e-12, atol=0)


def test_combine64_small():
    X = torch.tensor([[3.0, float("nan"), -1.0], [1.0, 2.0, -2.0], [2.0, -4.0, 5.0]])
    g, A, k = AO.combine64(X, None, 3, 3, "sorted", 1, 1, None, 1.0)
    assert g.tolist() == [2.0, 2.0, -1.0] and A.tolist() == [2.0, 2.0, 1.0] and k == 1
    rows = torch.tensor([2, 0], dtype=torch.int32)
    w = torch.tensor([0.5, -2.0])
    g, A, k = AO.combine64(X, rows, 2, 2, "weighted", 0, 1, w, 0.5)
    assert g[0].item() == -2.5 and torch.isnan(g[1]) and k == 2 and A[0].item() == 3.5
    w = torch.tensor([0.5, 0.0])          # the zero-weight row (NaN in column 1) is not read
    g, A, k = AO.combine64(X, rows, 2, 2, "weighted", 0, 1, w, 1.0)
    assert g.tolist() == [1.0, -2.0] and A.tolist() == [1.0, 2.0] and k == 1


def test_case_table_covers_the_dispatch_space():
    ids = [c.id for c in AO.CASES] + [c.id for c in AO.MULTI_CASES]
    assert len(set(ids)) == len(ids)
    core = [c for c in AO.CASES if c.id.startswith("core-")]
    for dt in ("bf16", "f32"):
        for b in (2, 4, 8, 16, 32, 64):
            kinds = {AO.OPTS[c.opt]["kind"] for c in core
                     if c.dtype == dt and AO.np_bucket(c.n) == b}
            assert "sgd" in kinds and kinds & {"adam", "adamw"}, (dt, b, kinds)
    # grid-stride segments: more than three trips of the capped one-launch grid
    for c in AO.MULTI_CASES:
        if c.id.startswith("stride-"):
            vec = 2 if c.n > 32 else (8 if c.dtype == "bf16" else 4)
            assert len(c.Ds) == 16 and all(D % vec == 0 for D in c.Ds)
            assert max(c.Ds) > 3 * (2048 // len(c.Ds)) * 256 * vec
            assert vec in c.Ds


@pytest.mark.parametrize("case", AO.CASES, ids=lambda c: c.id)
def test_agg_update_cpu(case):
    AO.run_case(case, torch.device("cpu"), K)


@pytest.mark.parametrize("case", AO.MULTI_CASES, ids=lambda c: c.id)
def test_agg_update_multi_cpu(case):
    AO.run_multi_case(case, torch.device("cpu"), K)
