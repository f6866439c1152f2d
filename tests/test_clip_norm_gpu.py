"""Global-norm clipping on the MI355X: ``sq_norm`` and ``clip_coef`` (csrc/kernels/clip_norm.hip)
against the fp64 definitions of ``ops.reference``, the engine's three stages (materialise, norm,
weighted update) against the fused pass they replace, and ``FusedAdamW(max_grad_norm=...)``
against its own CPU path."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 255, 256, 257, 2048 * 3 + 5, 2 ** 20 + 5]
RTOL = 1e-9      # fp64 accumulation of non-negative terms: at most D * 2^-53 ~ 1.2e-10 at 2^20 + 5


def _values(D, dtype, gen):
    """fp32: magnitudes spread log-uniformly over 1e-20 .. 1e15, random signs; bf16: N(0, 1)."""
    if dtype == torch.float32:
        e = torch.rand(D, generator=gen, dtype=torch.float64) * 35.0 - 20.0
        s = torch.randint(0, 2, (D,), generator=gen).double() * 2.0 - 1.0
        return (s * 10.0 ** e).float()
    return torch.randn(D, generator=gen).to(dtype)


def _placed(x, offset, dev):
    """x on the device, starting ``offset`` elements past a 16-B aligned address."""
    buf = torch.zeros(x.numel() + 16, dtype=x.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + x.numel()]
    v.copy_(x)
    assert (v.data_ptr() % 16 == 0) == (offset * x.element_size() % 16 == 0)
    return v


@pytest.fixture(scope="module")
def rows():
    """CPU rows per (dtype, D) and their fp64 oracle values per scale, computed once."""
    from consensusml_amd.ops import reference as ref
    gen = torch.Generator().manual_seed(7)
    out = {}
    for dtype in (torch.float32, torch.bfloat16):
        for D in LENGTHS:
            x = _values(D, dtype, gen)
            out[dtype, D] = (x, {sc: ref.sq_norm([x], sc) for sc in (1.0, 0.125)})
    return out


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sq_norm_float64_oracle(cuda, rows, dtype, scale, offset):
    from consensusml_amd.ops import kernels as K
    for D in LENGTHS:
        x, want = rows[dtype, D]
        v = _placed(x, offset, cuda)
        out = torch.full((2,), -1.0, dtype=torch.float64, device=cuda)
        K.sq_norm([v], scale, None, out[:1])
        K.sq_norm([v], scale, None, out[1:])
        got = out.cpu()
        rel = abs(float(got[0]) - float(want[scale])) / float(want[scale])
        print(f"sq_norm {dtype} D={D} scale={scale} offset={offset}: rel err {rel:.3e}")
        assert rel <= RTOL, (D, rel)
        assert got[0] == got[1], D                       # two runs: the same bits
        # the oracle itself against plain fp64 torch (both scales are powers of two: exact)
        plain = ((x.double() * scale) ** 2).sum()
        assert abs(float(want[scale]) - float(plain)) <= 1e-14 * float(plain)


@pytest.mark.parametrize("grid_cap", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sq_norm_several_passes(cuda, rows, dtype, grid_cap):
    """The default grid gives every workgroup one pass up to 1024 workgroups' worth of elements;
    a capped grid makes the same workgroups stride (many passes, the last one partial)."""
    from consensusml_amd.ops import kernels as K
    for D in (2048 * 3 + 5, 2 ** 20 + 5):
        x, want = rows[dtype, D]
        v = _placed(x, 1, cuda)
        out = torch.zeros(1, dtype=torch.float64, device=cuda)
        K.sq_norm([v], 1.0, None, out, grid_cap=grid_cap)
        rel = abs(float(out) - float(want[1.0])) / float(want[1.0])
        assert rel <= RTOL, (D, rel)


@pytest.mark.parametrize("nseg", [1, 3, 16, 21])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sq_norm_multi_segment(cuda, dtype, nseg):
    """Ragged segments in one launch (21: two launches of 16 + 5), one of length 1, starts at
    every alignment; a reused workspace; two runs bit-equal."""
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.ops import reference as ref
    gen = torch.Generator().manual_seed(100 + nseg)
    lens = [1, 2048 * 3 + 5, 257, 7, 70001, 8, 4096, 255, 33, 5000, 12, 1, 100, 9999, 64, 3,
            640, 2, 77777, 31, 16][:nseg]
    host = [_values(L, dtype, gen) for L in lens]
    segs = [_placed(x, i % 5, cuda) for i, x in enumerate(host)]
    for scale in (1.0, 0.125):
        want = float(ref.sq_norm(host, scale))
        work = K.sq_norm_workspace(segs)
        work.fill_(float("nan"))                          # every slot that is read is written
        out = torch.zeros(2, dtype=torch.float64, device=cuda)
        K.sq_norm(segs, scale, work, out[:1])
        K.sq_norm(segs, scale, work, out[1:])
        got = out.cpu()
        rel = abs(float(got[0]) - want) / want
        assert rel <= RTOL, (nseg, scale, rel)
        assert got[0] == got[1]
    with pytest.raises(RuntimeError, match="work"):
        K.sq_norm(segs + [segs[0]] * 16, 1.0, torch.zeros(1, dtype=torch.float64, device=cuda),
                  out[:1])


def test_sq_norm_non_finite_and_checks(cuda):
    from consensusml_amd.ops import kernels as K
    out = torch.zeros(1, dtype=torch.float64, device=cuda)
    for bad in (float("inf"), float("nan")):
        x = torch.ones(1000, device=cuda)
        x[777] = bad
        K.sq_norm([x], 1.0, None, out)
        assert not math.isfinite(float(out))
    with pytest.raises(RuntimeError, match="one dtype"):
        K.sq_norm([torch.ones(4, device=cuda), torch.ones(4, device=cuda).bfloat16()], 1.0, None, out)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        K.sq_norm([torch.ones(4, device=cuda).half()], 1.0, None, out)
    with pytest.raises(RuntimeError, match="out"):
        K.sq_norm([torch.ones(4, device=cuda)], 1.0, None, torch.zeros(1, device=cuda))


@pytest.mark.parametrize("norm2,c,base", [
    (4.0, 1.0, 1.0), (4.0, 1.0, 0.125), (0.25, 1.0, 1.0), (0.25, 1.0, 1.0 / 3.0), (0.0, 1.0, 1.0),
    (0.0, 1e-9, 1.0), (1e30, 1.0, 1.0), (float("inf"), 1.0, 0.5), (float("nan"), 1.0, 0.5),
    (-1.0, 1.0, 0.5),
])
def test_clip_coef_all_branches(cuda, norm2, c, base):
    from consensusml_amd.ops import kernels as K
    from consensusml_amd.ops import reference as ref
    w, norm, coef, bad = ref.clip_coef(torch.tensor([norm2], dtype=torch.float64), c, base)
    for via_reduced in (False, True):
        n2 = torch.tensor([norm2], dtype=torch.float64, device=cuda)
        junk = torch.tensor([123.0], dtype=torch.float64, device=cuda)
        w_out = torch.full((1,), -1.0, device=cuda)
        stats = torch.zeros(K.CLIP_STATS, dtype=torch.float64, device=cuda)
        stats[2] = 5.0
        if via_reduced:
            K.clip_coef(junk, c, base, w_out, stats, reduced=n2)
        else:
            K.clip_coef(n2, c, base, w_out, stats)
        st = stats.cpu()
        assert float(w_out) == float(w)                   # the same fp32 bits as the definition
        assert float(st[1]) == pytest.approx(float(coef), rel=1e-15)
        assert float(st[2]) == 5.0 + bad
        if bad:
            assert float(w_out) == 0.0 and float(st[1]) == 0.0
        else:
            assert float(st[0]) == pytest.approx(math.sqrt(norm2), rel=1e-15)
            assert float(st[3]) == norm2
        if not bad and math.sqrt(norm2) + 1e-6 <= c:
            assert float(st[1]) == 1.0
            assert float(w_out) == float(torch.tensor(base, dtype=torch.float32))


# ------------------------------------------------------------------------------- engine
def _cfg(rule, topo, V, f, pre="none", dtype="bf16", clip=0.0, opt="sgd"):
    from consensusml_amd import TrainConfig
    cfg = TrainConfig()
    cfg.dtype = dtype
    cfg.virtual_workers = V
    cfg.agg.rule = rule
    cfg.agg.f = f
    cfg.agg.pre = pre
    cfg.topology.kind = topo
    cfg.topology.bucket_mb = 0.0002       # ~100 bf16 elements: four buckets for the MLP
    cfg.optim.name = opt
    cfg.optim.lr = 0.1 if opt == "sgd" else 0.01
    cfg.optim.clip_norm = clip
    cfg.batch_per_worker = 16
    cfg.model.extra = {"classes": 2}
    return cfg


OFF_CASES = [
    ("mean", "allreduce", 0, "none"),
    ("median", "sharded", 2, "none"),
    ("krum", "allgather", 1, "none"),
    ("centered_clip", "sharded", 1, "none"),
    ("meamed", "sharded", 1, "nnm"),
    ("mean", "gossip", 0, "none"),
]


@pytest.mark.parametrize("rule,topo,f,pre", OFF_CASES, ids=[f"{r}-{t}" for r, t, _, _ in OFF_CASES])
def test_engine_huge_clip_norm_bit_identical_to_off(cuda, rule, topo, f, pre):
    """bf16 rows, n = 8 virtual workers, 3 steps: stage 1 (the rule kernels without an optimizer,
    writing the fp32 aggregate) + stage 3 (the weighted kernel over that one row) give the bits
    of the fused kernels when the coefficient is exactly 1."""
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    res = []
    for clip in (0.0, 1e30):
        tr = ConsensusTrainer(_cfg(rule, topo, 8, f, pre, clip=clip),
                              info=DistInfo(0, 1, 0, cuda, "none"))
        assert len(tr.engine.flat.buckets) >= 3
        tr.fit(3, log_every=0)
        torch.cuda.synchronize()
        e = tr.engine
        res.append((e.master.cpu().clone(), e.flat.flat_param.cpu().clone(), e.s1.cpu().clone()))
        if clip:
            st = e.grad_stats.cpu().tolist()
            assert st[1] == 1.0 and st[2] == 0.0 and st[0] > 0
            assert (e.gout is None) == (topo == "allreduce")     # (gossip, V = 8: not direct)
        tr.close()
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rule,topo,V,f,dtype", [
    ("median", "sharded", 8, 2, "fp32"),
    ("krum", "allgather", 8, 2, "fp32"),
    ("mean", "gossip", 1, 0, "fp32"),
    ("mean", "gossip", 1, 0, "bf16"),          # the direct path over a bf16 row (fp32 master)
], ids=["median-sharded", "krum-allgather", "mean-gossip-V1", "mean-gossip-V1-bf16row"])
def test_engine_clipped_step_has_the_clipped_norm(cuda, rule, topo, V, f, dtype):
    """SGD, lr 0.1, no momentum, no weight decay: ||delta master|| / lr is the norm of what the
    optimizer saw, c * norm / (norm + 1e-6), with ``norm`` read from ``engine.grad_stats``."""
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    c, lr = 0.05, 0.1
    cfg = _cfg(rule, topo, V, f, dtype=dtype, clip=c)
    cfg.optim.momentum = 0.0
    tr = ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, cuda, "none"))
    e = tr.engine
    assert (e.gout is None) == (V == 1) and not e.early_update
    for step in range(3):
        before = e.master.double().clone()
        tr.train_step()
        st = e.grad_stats.cpu().tolist()
        got = float((e.master.double() - before).norm()) / lr
        want = c * st[0] / (st[0] + 1e-6)
        print(f"{rule}/{topo} step {step}: norm {st[0]:.6g} coef {st[1]:.6g} "
              f"|dm|/lr {got:.9g} want {want:.9g} rel {abs(got - want) / want:.3e}")
        assert st[0] > c and st[1] == pytest.approx(c / (st[0] + 1e-6), rel=1e-12)   # active
        assert got == pytest.approx(want, rel=1e-5)
    tr.close()


def test_engine_norm_matches_reference_of_the_aggregate(cuda):
    """Sharded, multi-segment stage 1: grad_stats' norm is the fp64 norm of the materialised
    aggregate, and centered clipping keeps the UNCLIPPED aggregate as v0."""
    from consensusml_amd.ops import reference as ref
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    for rule in ("median", "centered_clip"):
        tr = ConsensusTrainer(_cfg(rule, "sharded", 8, 1, clip=0.01),
                              info=DistInfo(0, 1, 0, cuda, "none"))
        e = tr.engine
        tr.train_step()
        st = e.grad_stats.cpu().tolist()
        want = float(ref.sq_norm([e.gout.cpu()], 1.0))
        assert st[3] == pytest.approx(want, rel=RTOL) and st[1] < 1.0
        if rule == "centered_clip":
            for b, X, length in e._bucket_cols():
                assert torch.equal(X[e.n, :length], e.gout[b.offset:b.offset + length].to(X.dtype))
        tr.close()


# ------------------------------------------------------------------------------- fused optimizer
def test_fused_adamw_max_grad_norm_matches_cpu_path(cuda):
    """bf16 parameters with an fp32 master, two param groups: the HIP path (sq_norm over both
    flat gradients, the device weight into the fused AdamW kernel) against the same optimizer on
    the CPU (the fp64 / fp32 reference path), fed the same gradients. Tolerances: the norm is an
    fp64 sum of exact squares on both sides (RTOL); masters as
    tests/test_optim.py::test_gpu_fused_optim_matches_torch; parameters are their master rounded."""
    from consensusml_amd.optim import FusedAdamW

    def build(dev):
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Linear(192, 64), torch.nn.GELU(), torch.nn.Linear(64, 5))
        m = m.to(device=dev, dtype=torch.bfloat16)
        groups = [{"params": list(m[0].parameters())},
                  {"params": list(m[2].parameters()), "lr": 5e-3}]
        return m, FusedAdamW(groups, lr=1e-2, weight_decay=0.05, max_grad_norm=1.0)
    a, oa = build(cuda)
    b, ob = build("cpu")
    gen = torch.Generator().manual_seed(3)
    for step in range(3):
        # the first step's gradient is far above the threshold, the last one below it
        mag = (1.0, 0.05, 1e-4)[step]
        for p, q in zip(a.parameters(), b.parameters()):
            g = (torch.randn(q.shape, generator=gen) * mag).to(torch.bfloat16)
            q.grad = g.clone()
            p.grad = g.to(cuda)
        oa.step()
        ob.step()
        sa, sb = oa.grad_stats.cpu().tolist(), ob.grad_stats.tolist()
        assert sa[0] == pytest.approx(sb[0], rel=RTOL) and sa[1] == pytest.approx(sb[1], rel=RTOL)
        assert (sa[1] < 1.0) == (step < 2) and sa[2] == 0.0
    for p, q in zip(a.parameters(), b.parameters()):
        ma, mb = oa.state[p]["master"], ob.state[q]["master"]
        torch.testing.assert_close(ma.cpu(), mb, rtol=2e-5, atol=2e-6)
        assert torch.equal(p.detach(), ma.to(torch.bfloat16))
