"""Nearest-neighbour mixing on the GPU: the mixing stage of ``weights.hip`` against the CPU branch
of ``K.robust_weights``, the mixed sorted combine of ``agg_update.hip`` against a float64 oracle
that uses the fp32 M the kernel was given, its multi-segment launch and fallbacks, and an engine
step with ``agg.pre=nnm`` against the CPU engine.

Bound on the mixed combine, elementwise:

    |gout - g64| <= max_i (n + 2) 2^-23 sum_j |M_ij| |x_j|  +  (cnt + 2) 2^-23 A

The first term bounds the error of every mixed value y_i = sum_j M_ij x_j (n fp32 fmas, unit
roundoff 2^-24, doubled as in ``agg_oracle``); order statistics are 1-Lipschitz in the sup norm,
so every sorted rank moves by at most the largest of them. The second term is ``agg_oracle``'s
bound (a) on the window mean, A = the window mean of |y|.
"""
import math

import pytest
import torch

from agg_oracle import (GUARD, OPTS, TOL_ADAM_M, TOL_ADAM_V, TOL_MASTER, TOL_SGD_BUF, _guarded,
                        _guards_intact, _on, _state, _tdt, _worker_rows, step64, window)
from consensusml_amd import TrainConfig
from consensusml_amd.ops import kernels as K
from consensusml_amd.ops import reference as ref
from consensusml_amd.ops.kernels import WEIGHT_RULES as GRAM_RULES
from consensusml_amd.parallel.dist import DistInfo
from consensusml_amd.parallel.engine import ConsensusEngine

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


# =========================================================================== weights.hip
def _gram_case(n, rule, seed, nan_row=None, dup=None):
    """fp64 Gram of n random rows (+ the previous aggregate for centered clipping), two loose
    clusters so that neighbourhoods are not arbitrary."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 48, generator=g, dtype=torch.float64)
    X[n // 2:] += 1.5
    if dup is not None:
        X[dup[1]] = X[dup[0]]
    if nan_row is not None:
        X[nan_row, 7] = float("nan")
    if rule == "centered_clip":
        X = torch.cat([X, 0.1 * torch.randn(1, 48, generator=g, dtype=torch.float64)])
    return X @ X.t()


def _weights_both(G, rule, n, f, dev):
    """K.robust_weights with pre='nnm' on the CPU branch and on the GPU: (w, mix, sel, counts)."""
    out = []
    for d in (CPU, dev):
        dim = n + 1 if rule == "centered_clip" else n
        w = torch.full((dim,), 7.0, dtype=torch.float32, device=d)
        mix = torch.full((n, n), 7.0, dtype=torch.float32, device=d)
        sel = torch.zeros(n + 1, dtype=torch.int32, device=d)
        cnt = torch.zeros(n, dtype=torch.float64, device=d)
        sc = torch.zeros(n, dtype=torch.float64, device=d)
        iters = 3 if rule == "centered_clip" else 8
        K.robust_weights(G.to(d), rule, n, f, iters=iters, tau=1.0, w_out=w, scores=sc, sel=sel,
                         sel_counts=cnt, pre="nnm", mix_out=mix)
        out.append((w.cpu(), mix.cpu(), sel.cpu(), cnt.cpu(), sc.cpu()))
    return out


def _check_weights(G, rule, n, f, dev):
    (wc, mc, sc_, cc, _), (wg, mg, sg, cg, _) = _weights_both(G, rule, n, f, dev)
    assert torch.equal(mg, mc), "mixing matrix differs from the CPU branch"
    assert torch.equal(mg, ref.nnm_matrix(G, n, f).float())
    assert torch.equal(sg[:n], sc_[:n]), (sg.tolist(), sc_.tolist())
    assert torch.equal(cg, cc)
    torch.testing.assert_close(wg, wc, rtol=0, atol=1e-6)
    assert abs(float(wg.sum()) - 1.0) < 1e-5


# centered clipping carries the previous aggregate as row n + 1 <= 64: its largest n is 63
@pytest.mark.parametrize("n", [3, 4, 8, 9, 16, 17, 33, 64])
@pytest.mark.parametrize("rule", GRAM_RULES)
def test_mixing_stage_matches_cpu_branch(cuda, rule, n):
    if rule == "centered_clip" and n == 64:
        n = 63
    f = (n - 1) // 3
    _check_weights(_gram_case(n, rule, 100 + n), rule, n, f, cuda)


@pytest.mark.parametrize("rule", GRAM_RULES)
def test_mixing_stage_nan_row(cuda, rule):
    n, f = 9, 2
    G = _gram_case(n, rule, 7, nan_row=4)
    _check_weights(G, rule, n, f, cuda)
    (w, mix, sel, _, _) = _weights_both(G, rule, n, f, cuda)[1]
    assert float(w[4]) == 0.0 and bool(torch.isfinite(w).all())
    e = torch.zeros(n)
    e[4] = 1.0
    assert torch.equal(mix[4], e) and torch.equal(mix[:, 4], e)


@pytest.mark.parametrize("rule", GRAM_RULES)
def test_mixing_stage_identical_rows(cuda, rule):
    n, f = 8, 2
    _check_weights(_gram_case(n, rule, 9, dup=(2, 5)), rule, n, f, cuda)


@pytest.mark.parametrize("n", [3, 8, 17, 32])
def test_mixing_matrix_only(cuda, n):
    """Rule 'nnm_only' (the coordinate rules): M and nothing else."""
    f = (n - 1) // 3
    G = _gram_case(n, "median", 40 + n)
    w = torch.full((n,), 7.0, device=cuda)
    mix = torch.full((n, n), 7.0, device=cuda)
    center = torch.zeros(2, dtype=torch.int32, device=cuda)
    K.robust_weights(G.to(cuda), "nnm_only", n, f, w_out=w, pre="nnm", mix_out=mix,
                     center_out=center)
    assert torch.equal(mix.cpu(), ref.nnm_matrix(G, n, f).float())
    assert bool((w == 7.0).all())
    assert int(center[0]) == ref.gram_center(G)


def test_pre_none_launch_is_unchanged(cuda):
    """The trailing arguments default to off: same weights with and without them."""
    n, f = 9, 2
    G = _gram_case(n, "krum", 3).to(cuda)
    for rule in ("krum", "multi_krum", "geomed"):
        a = K.robust_weights(G, rule, n, f)
        b = K.robust_weights(G, rule, n, f, pre="none", mix_out=torch.zeros(n, n, device=cuda))
        assert torch.equal(a, b)
        assert torch.equal(a.cpu(), K.robust_weights(G.cpu(), rule, n, f))


# =========================================================================== agg_update.hip
def _mix_matrix(kind, gen, n, X, f):
    """fp32 [n, n]: 'nnm' from the rows' Gram; 'dense' random, non-symmetric, row-stochastic, about
    30 % zeros; 'dense_nan' the same with column n - 1 all zero (that row of X is NaN)."""
    if kind == "nnm":
        return ref.nnm_matrix(ref.gram(X), n, f).float()
    M = torch.rand(n, n, generator=gen) + 0.05
    M[torch.rand(n, n, generator=gen) < 0.3] = 0.0
    M[torch.arange(n), (torch.arange(n) + 1) % n] += 0.2      # no empty row, not symmetric
    if kind == "dense_nan":
        M[:, n - 1] = 0.0
        M[torch.arange(n), (torch.arange(n) + 1) % (n - 1)] += 0.2
    return (M / M.sum(1, keepdim=True)).contiguous()


def mixed64(X, M, n, D, lo, cnt):
    """(g, A, mixbound): float64 window mean of the sorted mixed rows, the window mean of |y| and
    max_i (n + 2) 2^-23 sum_j |M_ij| |x_j|, zero entries of M skipped."""
    R = X[:n, :D].double()
    Md = M.double()
    Rz = torch.where(torch.isnan(R), torch.zeros_like(R), R)
    used = ((Md != 0).double() @ torch.isnan(R).double()) > 0    # a NaN under a non-zero entry
    Y = Md @ Rz
    Y = torch.where(used, torch.full_like(Y, math.inf), Y)       # NaN -> +inf
    S = Y.sort(dim=0).values[lo:lo + cnt]
    mixb = ((n + 2) * 2.0 ** -23 * (Md.abs() @ Rz.abs())).max(0).values
    return S.sum(0) / cnt, S.abs().sum(0) / cnt, mixb


def _check_gout(what, gout, X, M, n, D, lo, cnt):
    g64, A, mixb = mixed64(X, M, n, D, lo, cnt)
    assert bool(torch.isfinite(g64).all()), f"{what}: oracle not finite"
    assert bool(torch.isfinite(gout).all()), f"{what}: gout not finite"
    bound = mixb + (cnt + 2) * 2.0 ** -23 * A
    bound = torch.where(bound == 0, torch.full_like(bound, 2.0 ** -149), bound)
    ratio = ((gout.double() - g64).abs() / bound).max().item()
    print(f"{what}: max |gout - g64| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: gout error {ratio:.3f} of the bound"


def _check_state(what, hyper, before, after):
    """agg_oracle's checks (b), (c), (e) on one segment, fed with the kernel's own gout."""
    m0, s10, s20 = before
    m1, s11, s21, gout, pout = after
    kind = hyper["kind"]
    d = lambda t: None if t is None else t.double()   # noqa: E731
    pe, s1e, s2e = step64(kind, d(m0), gout.double(), d(s10), d(s20),
                          **{k: v for k, v in hyper.items() if k != "kind"})
    assert bool(torch.isfinite(m1).all()), f"{what}: master not finite"
    torch.testing.assert_close(m1.double(), pe, rtol=TOL_MASTER[0], atol=TOL_MASTER[1])
    if kind == "sgd":
        if hyper.get("momentum"):
            torch.testing.assert_close(s11.double(), s1e, rtol=TOL_SGD_BUF[0], atol=TOL_SGD_BUF[1])
            assert bool(torch.isfinite(s11).all()), f"{what}: momentum buffer not finite"
    else:
        torch.testing.assert_close(s11.double(), s1e, rtol=TOL_ADAM_M[0], atol=TOL_ADAM_M[1])
        torch.testing.assert_close(s21.double(), s2e, rtol=TOL_ADAM_V[0], atol=TOL_ADAM_V[1])
    assert torch.equal(pout, m1.to(pout.dtype)), f"{what}: param_out != master as {pout.dtype}"


OPT_CYCLE = ("sgd_nesterov", "sgd_first", "adamw")


def _run_mixed(dev, dt, n, D, comb, kind, optname, seed, pout="bf16"):
    gen = torch.Generator().manual_seed(seed)
    dtype = _tdt(dt)
    lo, cnt = window(comb, n)
    nan_rows = (n - 1,) if kind == "dense_nan" else ()
    flat, Xc, o, ld = _worker_rows(gen, dtype, n, D, list(range(n)), n + 1, nan_rows=nan_rows)
    Mc = _mix_matrix(kind, gen, n, Xc[:n, :D].double(), (n - 1) // 3)
    X, M = _on(dev, flat, o, n + 1, ld), Mc.to(dev)
    hyper = dict(OPTS[optname])
    m0, s10, s20 = _state(gen, hyper["kind"], hyper.get("first", False), D)
    mb = _guarded(m0, D, GUARD, torch.float32, dev)
    s1b = _guarded(s10, D, GUARD, torch.float32, dev)
    s2b = _guarded(s20, D, GUARD, torch.float32, dev) if s20 is not None else None
    gb = _guarded(None, D, GUARD, torch.float32, dev)
    pb = _guarded(None, D, GUARD, _tdt(pout), dev)
    sl = lambda b: None if b is None else b[GUARD:GUARD + D]   # noqa: E731
    K.agg_update(X, combine="sorted", lo=lo, cnt=cnt, n=n, D=D, opt=K.OptArgs(**hyper),
                 master=sl(mb), s1=sl(s1b), s2=sl(s2b), param_out=sl(pb), gout=sl(gb), mix=M)
    what = f"{dt} n={n} D={D} {comb} {kind} {optname}"
    for name, b in (("master", mb), ("s1", s1b), ("s2", s2b), ("gout", gb), ("param_out", pb)):
        if b is not None:
            assert _guards_intact(b, GUARD, D), f"{what}: wrote outside {name}"
    _check_gout(what, sl(gb), X, M, n, D, lo, cnt)
    before = tuple(None if t is None else t.to(dev) for t in (m0, s10, s20))
    _check_state(what, hyper, before, (sl(mb), sl(s1b), sl(s2b), sl(gb), sl(pb)))


@pytest.mark.parametrize("kind", ["nnm", "dense", "dense_nan"])
@pytest.mark.parametrize("comb", ["median", "trimmed"])
@pytest.mark.parametrize("n", [3, 4, 5, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_mixed_sorted_against_oracle(cuda, dt, n, comb, kind):
    i = n + 3 * (comb == "trimmed") + 5 * ("nnm", "dense", "dense_nan").index(kind) + (dt == "f32")
    _run_mixed(cuda, dt, n, 2059, comb, kind, OPT_CYCLE[i % 3], seed=1000 + i,
               pout=("bf16", "f32")[i % 2])


@pytest.mark.parametrize("D", [1, 7, 8])
@pytest.mark.parametrize("kind", ["nnm", "dense_nan"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_mixed_sorted_tiny_sizes(cuda, dt, kind, D):
    _run_mixed(cuda, dt, 5, D, "median", kind, OPT_CYCLE[D % 3], seed=2000 + D)
    _run_mixed(cuda, dt, 17, D, "trimmed", kind, OPT_CYCLE[(D + 1) % 3], seed=2100 + D)


def test_mixed_sorted_matches_cpu_branch(cuda):
    """The CPU branch of K.agg_update applies the same mix (zero-entry rule included)."""
    gen = torch.Generator().manual_seed(5)
    n, D = 9, 515
    X = torch.randn(n, D, generator=gen)
    X[n - 1] = float("nan")
    M = _mix_matrix("dense_nan", gen, n, None, 0)
    outs = []
    for d in (CPU, cuda):
        out = torch.empty(D, device=d)
        K.agg_update(X.to(d), combine="sorted", lo=2, cnt=5, gout=out, mix=M.to(d))
        outs.append(out.cpu())
    torch.testing.assert_close(outs[1], outs[0], rtol=1e-5, atol=1e-6)


def test_mix_argument_checks(cuda):
    X = torch.randn(8, 64, device=cuda)
    out = torch.empty(64, device=cuda)
    M = torch.eye(8, device=cuda)
    lib = K.lib()
    args = (X, 8, 64, None, 0, 3, 2, None, 0, None, None, None, None, out, 0.1, 0.0, 0.0, 0.9,
            0.999, 1e-8, 0.1, 1.0, 1.0, False, False)
    lib.agg_update(*args)                                   # positional call without mix
    plain = out.clone()
    lib.agg_update(*args, M)                                # the identity mixes nothing
    assert torch.equal(out, plain)
    for bad in (M.double(), M[:7, :7].contiguous(), M.cpu(),
                torch.eye(16, device=cuda)[::2, ::2]):          # dtype, shape, device, strides
        with pytest.raises((RuntimeError, ValueError)):
            lib.agg_update(*args, bad)
    with pytest.raises((RuntimeError, ValueError)):          # weighted combine takes no mix
        lib.agg_update(X, 8, 64, None, 1, 0, 1, None, 0, None, None, None, None, out, 0.1, 0.0,
                       0.0, 0.9, 0.999, 1e-8, 0.1, 1.0, 1.0, False, False, M)
    with pytest.raises((RuntimeError, ValueError)):          # more than 32 rows
        K.agg_update(torch.randn(33, 64, device=cuda), combine="sorted", lo=16, cnt=1, gout=out,
                     mix=torch.eye(33, device=cuda))


# --------------------------------------------------------------------------- multi-segment
def _run_mixed_multi(dev, dt, n, Ds, comb, kind, optname, seed, misoff=-1):
    gen = torch.Generator().manual_seed(seed)
    dtype = _tdt(dt)
    lo, cnt = window(comb, n)
    hyper = dict(OPTS[optname])
    offs, end = [], 0
    for i, D in enumerate(Ds):        # agg_oracle.run_multi_case's layout
        off = (end + 7) // 8 * 8 + (8 if i else 0) + (1 if i == misoff else 0)
        offs.append(off)
        end = off + D
    total = end
    covered = torch.zeros(total, dtype=torch.bool)
    for D, off in zip(Ds, offs):
        covered[off:off + D] = True
    gap = ~covered
    m0, s10, s20 = _state(gen, hyper["kind"], hyper.get("first", False), total)

    def state_buf(vals):
        v = torch.full((total,), math.nan) if vals is None else vals.clone()
        v[gap] = 77.0
        return _guarded(v, total, GUARD, torch.float32, dev)

    mb, s1b, gb = state_buf(m0), state_buf(s10), state_buf(None)
    s2b = state_buf(s20) if s20 is not None else None
    nan_rows = (n - 1,) if kind == "dense_nan" else ()
    Xs, pbs = [], []
    for D in Ds:
        flat, _, o, ld = _worker_rows(gen, dtype, n, D, list(range(n)), n + 1, nan_rows=nan_rows)
        Xs.append(_on(dev, flat, o, n + 1, ld))
        pbs.append(_guarded(None, D, GUARD, torch.bfloat16, dev))
    M = _mix_matrix(kind, gen, n, None, 0).to(dev)
    sl = lambda b: None if b is None else b[GUARD:GUARD + total]   # noqa: E731
    K.agg_update_multi([(X, D, off, pb[GUARD:GUARD + D])
                        for X, D, off, pb in zip(Xs, Ds, offs, pbs)],
                       combine="sorted", lo=lo, cnt=cnt, n=n, opt=K.OptArgs(**hyper),
                       master=sl(mb), s1=sl(s1b), s2=sl(s2b), gout=sl(gb), mix=M)
    gapd = gap.to(dev)
    for name, b in (("master", mb), ("s1", s1b), ("s2", s2b), ("gout", gb)):
        if b is not None:
            assert _guards_intact(b, GUARD, total), f"wrote outside {name}"
            assert bool((sl(b)[gapd] == 77.0).all()), f"wrote between segments of {name}"
    for i, (X, D, off, pb) in enumerate(zip(Xs, Ds, offs, pbs)):
        assert _guards_intact(pb, GUARD, D), f"wrote outside param_out {i}"
        cut = lambda t: None if t is None else t[off:off + D]   # noqa: E731
        what = f"{dt} n={n} seg {i} (D={D}, off={off})"
        _check_gout(what, cut(sl(gb)), X, M, n, D, lo, cnt)
        before = tuple(None if t is None else cut(t).to(dev) for t in (m0, s10, s20))
        _check_state(what, hyper, before, (cut(sl(mb)), cut(sl(s1b)), cut(sl(s2b)), cut(sl(gb)),
                                           pb[GUARD:GUARD + D]))


@pytest.mark.parametrize("dt,n", [("bf16", 8), ("f32", 8), ("bf16", 4), ("f32", 17), ("bf16", 32)])
def test_mixed_multi_one_launch(cuda, dt, n):
    # elements per lane of the mixed kernel: 8 (bf16, n <= 4), 4 (n <= 16), 2 (n <= 32)
    vec = 8 if (dt == "bf16" and n <= 4) else (4 if n <= 16 else 2)
    _run_mixed_multi(cuda, dt, n, (4096, vec, 808, 520), "trimmed", "dense_nan", "sgd_nesterov",
                     seed=3000 + n)
    _run_mixed_multi(cuda, dt, n, (4096, vec, 808, 520), "median", "dense", "adamw",
                     seed=3100 + n)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_mixed_multi_fallbacks(cuda, dt):
    # a state offset off the vector grid, and a ragged segment size: one launch per segment
    _run_mixed_multi(cuda, dt, 8, (4096, 2048, 808, 520), "trimmed", "dense_nan", "sgd_first",
                     seed=3200, misoff=2)
    _run_mixed_multi(cuda, dt, 8, (4096, 2051, 808, 520), "median", "dense", "adamw", seed=3201)


# =========================================================================== engine
@pytest.mark.parametrize("rule", ["krum", "trimmed_mean"])
def test_engine_step_matches_cpu_engine(cuda, rule):
    """One sharded step over 8 virtual workers' bf16 gradient rows, agg.pre=nnm: the GPU engine
    (Gram, mixing stage, mixed / weighted update kernels) against the CPU engine on the same
    rows, at the tolerances of test_engine_gpu.py::test_gpu_topologies_match_cpu_reference."""
    n, f = 8, 2

    def eng(dev):
        torch.manual_seed(0)
        cfg = TrainConfig()
        cfg.virtual_workers = n
        cfg.agg.rule = rule
        cfg.agg.f = f
        cfg.agg.pre = "nnm"
        cfg.topology.kind = "sharded"
        cfg.topology.bucket_mb = 0.004
        cfg.optim.name = "sgd"
        cfg.optim.lr = 0.1
        cfg.optim.momentum = 0.9
        model = torch.nn.Linear(64, 64).to(torch.bfloat16).to(dev)
        return ConsensusEngine(model, cfg, DistInfo(0, 1, 0, dev, "none"))

    c, g = eng(CPU), eng(cuda)
    assert len(g.flat.buckets) >= 2 and g.flat.flat_grad.dtype == torch.bfloat16
    assert torch.equal(c.master, g.master.cpu())
    gen = torch.Generator().manual_seed(21)
    for step in range(2):
        base = torch.randn(c.flat.total, generator=gen)
        X = base + 0.3 * torch.randn(n, c.flat.total, generator=gen)
        X[:f] = -0.1 * X[f:].mean(0)
        X = X.to(torch.bfloat16)
        for e in (c, g):
            e.zero_grad()
            e.flat.flat_grad.copy_(X.to(e.device))
            e._flushed = {b.index for b in e.flat.buckets}
            e.step()
        assert torch.equal(g.M.cpu(), c.M), step
        if rule == "krum":
            assert torch.equal(g.sel.cpu(), c.sel), step
    torch.testing.assert_close(g.master.cpu(), c.master, rtol=2e-4, atol=2e-5)
    assert torch.equal(g.flat.flat_param, g.master.to(torch.bfloat16))
