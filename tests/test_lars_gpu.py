"""LARS on the MI355X (csrc/kernels/lars.hip): ``seg_sq_norm`` and ``lars_ratio`` against the fp64
definitions of ``ops.reference``, ``lars_update`` bit for bit against the weighted n = 1 kernel
of agg_update.hip (q = 1) and under LARS's defining invariance (a rescaled gradient), its
coverage against the CPU path, and the engine's three stages against the independent oracle of
tests/lars_oracle.py."""
import copy
import math

import pytest
import torch

import lars_oracle as LO

pytestmark = pytest.mark.gpu

RTOL_NORM = 1e-9     # tests/test_clip_norm_gpu.py: fp64 sums of non-negative terms, <= D * 2^-53
RTOL, ATOL = 2e-5, 2e-6      # ... and its pair for a fused fp32 update against a reference path


def _values(D, dtype, gen):
    """fp32: magnitudes spread log-uniformly over 1e-20 .. 1e15, random signs; bf16: N(0, 1)."""
    if dtype == torch.float32:
        e = torch.rand(D, generator=gen, dtype=torch.float64) * 35.0 - 20.0
        s = torch.randint(0, 2, (D,), generator=gen).double() * 2.0 - 1.0
        return (s * 10.0 ** e).float()
    return torch.randn(D, generator=gen).to(dtype)


def _sizes(T, C, gen):
    """T tensor sizes from the set of the kernel's edges (the largest one at most twice), with
    zero-length entries in between."""
    pool = [1, 7, 8, 9, 63, 64, 255, 6149, C - 1, C, C + 1, 2 * C + 3, 2 ** 20 + 5]
    if T == 1:
        return [2 ** 20 + 5]
    if T == 3:
        return [2 * C + 3, 0, 7]
    idx = torch.randint(0, len(pool) - 1, (T,), generator=gen).tolist()
    sizes = [pool[i] for i in idx]
    sizes[20:20 + len(pool)] = pool              # every size at least once
    sizes[60] = 2 ** 20 + 5
    for k in (0, 17, 18, T - 1):                 # zero-length entries, also first and last
        sizes[k] = 0
    return sizes


def _layout(sizes):
    starts, off = [], 0
    for n in sizes:
        starts.append(off)
        off += -(-n // 8) * 8
    return starts, -(-max(off, 8) // 64) * 64


@pytest.fixture(scope="module")
def norm_cases():
    """Per (T, chunk, dtype): CPU vectors with garbage in the padding, and the fp64 oracle values
    per scale, computed once."""
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.ops import reference as ref
    gen = torch.Generator().manual_seed(11)
    out = {}
    for T in (1, 3, 200):
        for chunk in (K.LARS_CHUNK, 1024):
            sizes = _sizes(T, chunk, gen)
            starts, total = _layout(sizes)
            for dtype in (torch.float32, torch.bfloat16):
                p = torch.randn(total, generator=gen)
                g = _values(total, dtype, gen)
                for s, n, e in zip(starts, sizes, starts[1:] + [total]):
                    p[s + n:e] = float("nan")        # padding: fault injection may write there
                    g[s + n:e] = float("inf")
                want = {sc: ref.seg_sq_norm(p, g, sc, starts, sizes) for sc in (1.0, 0.125)}
                out[T, chunk, dtype] = (starts, sizes, total, p, g, want)
    return out


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("chunk", [0, 1024], ids=["C-default", "C-1024"])
@pytest.mark.parametrize("T", [1, 3, 200])
def test_seg_sq_norm_float64_oracle(cuda, norm_cases, T, chunk, dtype, scale):
    from consensusml_amd.ops import kernels as K
    starts, sizes, total, p, g, want = norm_cases[T, chunk or K.LARS_CHUNK, dtype]
    assert sizes.count(0) >= (0 if T == 1 else 1)
    plan = K.lars_plan(starts, sizes, chunk=chunk, total=total)
    pd, gd = p.to(cuda), g.to(cuda)
    outs = []
    for cap in (0, 0, 3):         # the default grid twice, then three striding workgroups
        plan.on(cuda)[3].fill_(float("nan"))             # every slot that is read is written
        out = torch.full((plan.T, 2), -1.0, dtype=torch.float64, device=cuda)
        K.seg_sq_norm(pd, gd, scale, plan, out=out, grid_cap=cap)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])   # the same bits
    w = want[scale]
    worst = 0.0
    for t, n in enumerate(sizes):
        for c in (0, 1):
            if n == 0 or float(w[t, c]) == 0.0:
                assert float(outs[0][t, c]) == float(w[t, c])
            else:
                worst = max(worst, abs(float(outs[0][t, c]) - float(w[t, c])) / float(w[t, c]))
    print(f"seg_sq_norm T={T} chunk={plan.chunk} {dtype} scale={scale}: worst rel err {worst:.3e} "
          f"over {plan.items.shape[0]} items")
    assert worst <= RTOL_NORM


def test_seg_sq_norm_checks(cuda):
    from consensusml_amd.ops import kernels as K
    plan = K.lars_plan([0, 16], [9, 40], total=64)
    m = torch.ones(64, device=cuda)
    with pytest.raises(RuntimeError, match="g must be"):
        K.seg_sq_norm(m, torch.ones(32, device=cuda), 1.0, plan)
    with pytest.raises(RuntimeError, match="master must be"):
        K.seg_sq_norm(m.double(), m, 1.0, plan)
    with pytest.raises(RuntimeError, match="16-B aligned"):
        K.seg_sq_norm(torch.ones(72, device=cuda)[1:65], m, 1.0, plan)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        K.seg_sq_norm(m, m.half(), 1.0, plan)


# ------------------------------------------------------------------------------- lars_ratio
BRANCHES = [
    (4.0, 0.25, True), (4.0, 0.25, False), (0.0, 0.25, True), (4.0, 0.0, True),
    (4.0, float("inf"), True), (4.0, float("nan"), False), (float("inf"), 1.0, True),
    (float("nan"), 1.0, True), (1e-20, 1e20, True), (3.7e11, 2.9e-17, True),
]


@pytest.mark.parametrize("wd,eps", [(0.0, 0.0), (0.05, 1e-8)])
def test_lars_ratio_all_branches(cuda, wd, eps):
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.ops import reference as ref
    pairs = torch.tensor([[a, b] for a, b, _ in BRANCHES], dtype=torch.float64)
    adapt = torch.tensor([ad for _, _, ad in BRANCHES], dtype=torch.uint8)
    q, st, bad = ref.lars_ratio(pairs, adapt, 0.02, wd, eps)
    T = len(BRANCHES)
    for via_reduced in (False, True):
        qo = torch.full((T,), -1.0, device=cuda)
        stats = torch.zeros(T, K.LARS_STATS, dtype=torch.float64, device=cuda)
        stats[:, 3] = 5.0
        junk = torch.full((T, 2), 123.0, dtype=torch.float64, device=cuda)
        if via_reduced:
            K.lars_ratio(junk, adapt.to(cuda), 0.02, wd, eps, qo, stats, reduced=pairs.to(cuda))
        else:
            K.lars_ratio(pairs.to(cuda), adapt.to(cuda), 0.02, wd, eps, qo, stats)
        got, gs = qo.cpu(), stats.cpu()
        for t in range(T):
            assert float(got[t]) == pytest.approx(float(q[t]), rel=1e-15), t
            assert float(gs[t, 3]) == 5.0 + int(bad[t])
            assert float(gs[t, 2]) == float(got[t])
            for c in (0, 1):
                if math.isnan(float(st[t, c])):
                    assert math.isnan(float(gs[t, c]))
                else:
                    assert float(gs[t, c]) == pytest.approx(float(st[t, c]), rel=1e-15)
            if bad[t]:
                assert float(got[t]) == 0.0
    assert q.tolist()[1:4] == [1.0, 1.0, 1.0] and float(q[0]) not in (0.0, 1.0)


# ------------------------------------------------------------------------------- lars_update
def _state(gen, sizes, dtype, cuda):
    starts, total = _layout(sizes)
    p = torch.randn(total, generator=gen)
    g = torch.randn(total, generator=gen).to(dtype)
    buf = torch.randn(total, generator=gen)
    return starts, total, p, g, buf


EXACT_SIZES = [6149, 8, 1, 70001, 255, 64, 9]


@pytest.mark.parametrize("pdtype", [torch.bfloat16, torch.float32], ids=["p-bf16", "p-fp32"])
@pytest.mark.parametrize("momentum,nesterov,first,wd", [
    (0.0, False, False, 0.0), (0.9, False, True, 0.0), (0.9, False, False, 0.01),
    (0.9, True, False, 0.01), (0.9, True, True, 0.0)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lars_update_unit_ratio_is_the_sgd_kernel(cuda, dtype, momentum, nesterov, first, wd,
                                                  pdtype):
    """q = 1 everywhere: master, momentum and parameters have the bits of
    ``agg_update(combine="weighted", n=1, opt=sgd)`` on the same inputs."""
    from consensusml_amd.ops import kernels as K
    gen = torch.Generator().manual_seed(21)
    starts, total, p, g, buf = _state(gen, EXACT_SIZES, dtype, cuda)
    plan = K.lars_plan(starts, EXACT_SIZES, total=total)
    q = torch.ones(plan.T, device=cuda)
    for scale in (1.0, 0.125):
        res = []
        for lars in (False, True):
            m, b, x = p.to(cuda), buf.to(cuda), g.to(cuda)
            pout = torch.zeros(total, dtype=pdtype, device=cuda)
            kw = dict(lr=0.1, momentum=momentum, weight_decay=wd, nesterov=nesterov, first=first)
            if lars:
                K.lars_update(x, scale, plan, q, K.OptArgs(kind="lars", **kw), m,
                              b if momentum else None, segs=[(pout, 0, total)])
            else:
                K.agg_update(x, combine="weighted", n=1, opt=K.OptArgs(kind="sgd", gscale=scale,
                                                                        **kw),
                             master=m, s1=b if momentum else None, param_out=pout)
            res.append((m.cpu(), b.cpu(), pout.cpu()))
        for a, c in zip(*res):
            assert torch.equal(a, c)
        assert not torch.equal(res[0][0], p)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lars_step_is_invariant_to_the_gradient_scale(cuda, dtype, momentum):
    """wd = 0, eps = 0, every tensor adapted: a gradient row scaled by 4 gives q / 4 exactly and
    every output bit for bit."""
    from consensusml_amd.ops import kernels as K
    gen = torch.Generator().manual_seed(22)
    starts, total, p, g, buf = _state(gen, EXACT_SIZES, dtype, cuda)
    plan = K.lars_plan(starts, EXACT_SIZES, chunk=1024, total=total)
    adapt = torch.ones(plan.T, dtype=torch.uint8, device=cuda)
    res = []
    for mult in (1.0, 4.0):
        m, b, x = p.to(cuda), buf.to(cuda), (g.float() * mult).to(dtype).to(cuda)
        pout = torch.zeros(total, dtype=torch.bfloat16, device=cuda)
        q = torch.zeros(plan.T, device=cuda)
        stats = torch.zeros(plan.T, K.LARS_STATS, dtype=torch.float64, device=cuda)
        pairs = K.seg_sq_norm(m, x, 1.0, plan)
        K.lars_ratio(pairs, adapt, 0.02, 0.0, 0.0, q, stats)
        K.lars_update(x, 1.0, plan, q, K.OptArgs(kind="lars", lr=0.1, momentum=momentum), m,
                      b if momentum else None, segs=[(pout, 0, total)])
        res.append((q.cpu(), m.cpu(), b.cpu(), pout.cpu()))
    assert torch.equal(res[0][0], res[1][0] * 4.0) and bool((res[0][0] > 0).all())
    for a, c in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, c)


def _against_cpu_path(cuda, sizes, segs_of, dtype, gen, nan_tensor=None):
    """lars_update on the GPU against the same wrapper on CPU tensors (the reference path)."""
    from consensusml_amd.ops import kernels as K
    starts, total, p, g, buf = _state(gen, sizes, dtype, cuda)
    plan = K.lars_plan(starts, sizes, total=total)
    q = torch.rand(plan.T, generator=gen) * 1.5 + 0.5
    if nan_tensor is not None:
        q[nan_tensor] = 0.0
        g[starts[nan_tensor]] = float("nan")
    opt = K.OptArgs(kind="lars", lr=0.1, momentum=0.9, weight_decay=0.01, nesterov=True)
    res = []
    for dev in ("cpu", cuda):
        m, b, x = p.clone().to(dev), buf.clone().to(dev), g.to(dev)     # (.to("cpu") is no copy)
        segs = [(torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=dev), o, n)
                for o, n in segs_of(total)]
        K.lars_update(x, 0.5, plan, q.to(dev), opt, m, b, segs=segs)
        res.append((m.cpu(), b.cpu(), [s[0].cpu() for s in segs]))
    (m0, b0, o0), (m1, b1, o1) = res
    covered = torch.zeros(total, dtype=torch.bool)
    for o, n in segs_of(total):
        covered[o:o + n] = True
    assert bool(torch.isfinite(m1[covered]).all()) and bool(torch.isfinite(b1[covered]).all())
    torch.testing.assert_close(m1, m0, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(b1, b0, rtol=RTOL, atol=ATOL)
    assert torch.equal(m1[~covered], p[~covered]) and torch.equal(b1[~covered], buf[~covered])
    for (o, n), a, c in zip(segs_of(total), o0, o1):
        assert torch.equal(c[:n], m1[o:o + n].to(torch.bfloat16))
        assert bool((c[n:] == 7.0).all()) and bool((a[n:] == 7.0).all())   # nothing past a segment


@pytest.mark.parametrize("nseg", [1, 3, 16, 17])
def test_lars_update_output_segments(cuda, nseg):
    """Segments of unequal lengths that tile the vector (17: two launches), the last one ragged
    and short of the vector's end: what no segment covers is not touched."""
    def segs_of(total):
        cuts = [total * k // nseg // 8 * 8 for k in range(nseg)] + [total - 13]
        return [(a, e - a) for a, e in zip(cuts, cuts[1:])]
    gen = torch.Generator().manual_seed(30 + nseg)
    _against_cpu_path(cuda, [6149, 8, 1, 40001, 255, 64, 9, 20000], segs_of, torch.bfloat16, gen,
                      nan_tensor=3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lars_update_table_of_300_tensors(cuda, dtype):
    gen = torch.Generator().manual_seed(40)
    pool = [1, 7, 8, 9, 63, 64, 255, 0, 6149]
    sizes = [pool[i] for i in torch.randint(0, len(pool), (300,), generator=gen).tolist()]
    sizes[0], sizes[150] = 9, 70001
    _against_cpu_path(cuda, sizes, lambda total: [(0, total)], dtype, gen, nan_tensor=150)


def test_lars_update_checks(cuda):
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.ops.native import lib
    m, g = torch.ones(64, device=cuda), torch.ones(64, device=cuda)
    q = torch.ones(2, device=cuda)
    starts = torch.tensor([0, 12, 64], device=cuda)
    args = ([None], [0], [64], 0.1, 0.0, 0.0, False, False)
    with pytest.raises(RuntimeError, match="not a multiple of 8"):
        lib().lars_update(g, 1.0, m, None, q, starts, [0, 12, 64], *args)
    with pytest.raises(ValueError, match="not a multiple of 8"):
        K.lars_plan([0, 12], [9, 40])
    with pytest.raises(RuntimeError, match="ascend"):
        lib().lars_update(g, 1.0, m, None, q, starts, [0, 64, 16], *args)
    plan = K.lars_plan([0, 16], [9, 40], total=64)
    opt = K.OptArgs(kind="lars", lr=0.1, momentum=0.9)
    with pytest.raises(RuntimeError, match="momentum needs s1"):
        K.lars_update(g, 1.0, plan, q, opt, m, None)
    with pytest.raises(RuntimeError, match="multiple of 8 inside"):
        K.lars_update(g, 1.0, plan, q, opt, m, m.clone(), segs=[(None, 4, 16)])
    with pytest.raises(RuntimeError, match="multiple of 8 inside"):
        K.lars_update(g, 1.0, plan, q, opt, m, m.clone(), segs=[(None, 8, 64)])
    with pytest.raises(ValueError, match="kind='lars'"):
        K.lars_update(g, 1.0, plan, q, K.OptArgs(kind="sgd"), m, None)
    assert torch.equal(m.cpu(), torch.ones(64))


# ------------------------------------------------------------------------------- engine
def _cfg(rule, topo, V, f, pre="none", dtype="bf16"):
    from consensusml_amd import TrainConfig
    cfg = TrainConfig()
    cfg.dtype = dtype
    cfg.virtual_workers = V
    cfg.agg.rule = rule
    cfg.agg.f = f
    cfg.agg.pre = pre
    cfg.topology.kind = topo
    cfg.topology.bucket_mb = 0.0002       # ~100 bf16 elements: four buckets for the MLP
    cfg.optim.name = "lars"
    cfg.optim.lr = 0.5
    cfg.optim.momentum = 0.9
    cfg.optim.weight_decay = 0.01
    cfg.optim.trust_coef = 0.02
    cfg.batch_per_worker = 16
    cfg.model.extra = {"classes": 2}
    return cfg


def _trainer(cfg, dev):
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    return ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, dev, "none"))


ENGINE_CASES = [
    ("median", "sharded", 8, 2, "none", "bf16"),
    ("krum", "allgather", 8, 1, "none", "bf16"),
    ("meamed", "sharded", 8, 1, "nnm", "bf16"),
    ("centered_clip", "sharded", 8, 1, "none", "bf16"),
    ("mean", "allreduce", 8, 0, "none", "bf16"),
    ("mean", "gossip", 1, 0, "none", "bf16"),
    ("mean", "gossip", 1, 0, "none", "fp32"),
]


@pytest.mark.parametrize("rule,topo,V,f,pre,dtype", ENGINE_CASES,
                         ids=[f"{c[0]}-{c[1]}-V{c[2]}-{c[5]}" for c in ENGINE_CASES])
def test_engine_against_oracle(cuda, rule, topo, V, f, pre, dtype):
    """The three stages on the device against the per-tensor fp64 oracle, fed the aggregate the
    engine used (``gout``, or the single gradient row times its scale on the direct paths)."""
    tr = _trainer(_cfg(rule, topo, V, f, pre, dtype), cuda)
    e = tr.engine
    assert e.lars and not e.early_update and e.s2 is None
    assert (e.gout is None) == (topo == "allreduce" or V == 1)
    assert len(e.flat.buckets) >= 3
    LO.check_engine_against_oracle(tr, 3, RTOL, ATOL)
    tr.close()


@pytest.mark.parametrize("rule,topo,V,f,dtype", [
    ("median", "sharded", 8, 2, "fp32"),
    ("krum", "allgather", 8, 2, "bf16"),
    ("mean", "gossip", 1, 0, "bf16"),
], ids=["median-sharded", "krum-allgather", "mean-gossip-V1-bf16row"])
def test_engine_step_has_the_lars_length(cuda, rule, topo, V, f, dtype):
    """No momentum, no weight decay, eps = 0: an adapted tensor moves by lr * trust * wn whatever
    its gradient, an excluded one by lr * gn, with wn and gn read from ``engine.lars_stats``."""
    cfg = _cfg(rule, topo, V, f, dtype=dtype)
    cfg.optim.momentum = 0.0
    cfg.optim.weight_decay = 0.0
    cfg.optim.eps = 0.0
    cfg.optim.trust_coef = 0.1      # steps of 5 % of ||w||: far above the fp32 rounding of p
    lr, trust = cfg.optim.lr, cfg.optim.trust_coef
    tr = _trainer(cfg, cuda)
    e = tr.engine
    fl = e.flat
    assert e.s1 is None
    for step in range(3):
        before = e.master.double().clone()
        tr.train_step()
        st = e.lars_stats.cpu()
        delta = e.master.double() - before
        for i, p in enumerate(fl.params):
            s, n = fl.param_offset[i], p.numel()
            got = float(delta[s:s + n].norm())
            wn, gn, q = st[i, :3].tolist()
            want = lr * trust * wn if p.dim() >= 2 else lr * gn
            print(f"{rule}/{topo} step {step} tensor {i} dim {p.dim()}: wn {wn:.6g} gn {gn:.6g} "
                  f"q {q:.6g} |dm| {got:.9g} want {want:.9g} rel {abs(got - want) / want:.3e}")
            assert wn > 0 and gn > 0 and (q == 1.0) == (p.dim() < 2)
            assert got == pytest.approx(want, rel=1e-5)
    tr.close()


def test_engine_norms_match_reference_of_the_aggregate(cuda):
    """Sharded, multi-segment stage 1: ``lars_stats``' gn is the fp64 norm of the materialised
    aggregate per tensor, and centered clipping keeps the aggregate as v0."""
    from consensusml_amd.ops import reference as ref
    for rule in ("median", "centered_clip"):
        tr = _trainer(_cfg(rule, "sharded", 8, 1), cuda)
        e = tr.engine
        fl = e.flat
        master = e.master.cpu().clone()
        tr.train_step()
        st = e.lars_stats.cpu()
        starts = [fl.param_offset[i] for i in range(len(fl.params))]
        sizes = [p.numel() for p in fl.params]
        want = ref.seg_sq_norm(master, e.gout.cpu(), 1.0, starts, sizes).sqrt()
        for i in range(len(sizes)):
            assert float(st[i, 0]) == pytest.approx(float(want[i, 0]), rel=RTOL_NORM)
            assert float(st[i, 1]) == pytest.approx(float(want[i, 1]), rel=RTOL_NORM)
        if rule == "centered_clip":
            for b, X, length in e._bucket_cols():
                assert torch.equal(X[e.n, :length], e.gout[b.offset:b.offset + length].to(X.dtype))
        tr.close()


def test_engine_gpu_path_matches_cpu_path(cuda):
    """fp32, median over 8 virtual workers, sharded: the HIP stages against the engine's own CPU
    path on the same batches after 3 steps."""
    cfg = _cfg("median", "sharded", 8, 2, dtype="fp32")
    g = _trainer(cfg, cuda)
    c = _trainer(copy.deepcopy(cfg), torch.device("cpu"))
    c.model.load_state_dict({k: v.cpu() for k, v in g.model.state_dict().items()})
    c.engine.master.copy_(g.engine.master.cpu())
    for _ in range(3):
        batches = [c.task.make_batch(16, gen) for gen in c.gens]
        for tr, dev in ((c, "cpu"), (g, cuda)):
            tr.engine.zero_grad()
            for v, (x, y) in enumerate(batches):
                tr.engine.bind_worker(v)
                tr.task.loss_fn(tr.model, (x.to(dev), y.to(dev))).backward()
            tr.engine.step()
    for a, b in zip(c.model.parameters(), g.model.parameters()):
        torch.testing.assert_close(a, b.cpu(), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(c.engine.lars_stats[:, :3], g.engine.lars_stats[:, :3].cpu(),
                               rtol=1e-4, atol=0)
    g.close()
    c.close()


def test_fused_lars_matches_cpu_path(cuda):
    """bf16 parameters with an fp32 master: ``FusedLARS`` through the HIP kernels against the
    same optimizer on the CPU, fed the same gradients."""
    from consensusml_amd.optim import FusedLARS

    def build(dev):
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Linear(192, 64), torch.nn.LayerNorm(64),
                                torch.nn.Linear(64, 5))
        m = m.to(device=dev, dtype=torch.bfloat16)
        return m, FusedLARS(m.parameters(), lr=0.2, momentum=0.9, weight_decay=0.01,
                            trust_coef=0.02, eps=1e-9)
    a, oa = build(cuda)
    b, ob = build("cpu")
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        for p, q in zip(a.parameters(), b.parameters()):
            g = torch.randn(q.shape, generator=gen).to(torch.bfloat16)
            q.grad = g.clone()
            p.grad = g.to(cuda)
        oa.step(grad_scale=0.5)
        ob.step(grad_scale=0.5)
        sa, sb = oa.lars_stats[0].cpu(), ob.lars_stats[0]
        torch.testing.assert_close(sa[:, :2], sb[:, :2], rtol=1e-6, atol=0)
        torch.testing.assert_close(sa[:, 2], sb[:, 2], rtol=1e-6, atol=0)
        assert float(sa[:, 3].sum()) == 0.0
    for p, q in zip(a.parameters(), b.parameters()):
        ma, mb = oa.state[p]["master"], ob.state[q]["master"]
        torch.testing.assert_close(ma.cpu(), mb, rtol=RTOL, atol=ATOL)
        assert torch.equal(p.detach(), ma.to(torch.bfloat16))
