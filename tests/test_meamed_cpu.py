"""MeaMed and Phocas (mean of the n - f values nearest to a robust centre, per coordinate) on the
CPU path: ``reference.mean_around`` against a brute-force float64 selection, the tie rule, the
non-finite contract, the ops wrappers, the config errors and the engine in both topologies."""
import math

import pytest
import torch

from consensusml_amd import TrainConfig
from consensusml_amd.ops import kernels as K
from consensusml_amd.ops import reference as ref

CPU = torch.device("cpu")
INF, NAN = math.inf, math.nan


def brute_force(X, lo, cnt, keep):
    """float64: the ``keep`` values nearest to the centre by |s - c|, ties to the lower rank."""
    S = X.double().sort(dim=0).values
    c = S[lo:lo + cnt].mean(0)
    n, D = S.shape
    out = torch.empty(D, dtype=torch.float64)
    for d in range(D):
        order = sorted(range(n), key=lambda i: (abs(float(S[i, d] - c[d])), i))[:keep]
        out[d] = S[sorted(order), d].sum() / keep
    return out


# --------------------------------------------------------------------------- mean_around
@pytest.mark.parametrize("n", [3, 4, 5, 8, 9])
def test_mean_around_against_brute_force(n):
    g = torch.Generator().manual_seed(n)
    X = torch.randn(n, 257, generator=g)
    for f in range(0, (n - 1) // 2 + 1):
        for lo, cnt in (ref.median_window(n), (f, n - 2 * f)):
            want = brute_force(X, lo, cnt, n - f)
            got = ref.mean_around(X, lo, cnt, n - f)
            assert got.dtype == torch.float32
            # fp32 sums of at most 9 terms of N(0, 1) values: far inside 1e-6; a window off by
            # one rank would differ by ~1e-1
            torch.testing.assert_close(got.double(), want, rtol=0, atol=2e-6)
        torch.testing.assert_close(ref.meamed(X, f).double(),
                                   brute_force(X, *ref.median_window(n), n - f), rtol=0, atol=2e-6)
        torch.testing.assert_close(ref.phocas(X, f).double(),
                                   brute_force(X, f, n - 2 * f, n - f), rtol=0, atol=2e-6)
        assert torch.equal(ref.aggregate(X, "meamed", f=f), ref.meamed(X, f))
        assert torch.equal(ref.aggregate(X, "phocas", f=f), ref.phocas(X, f))
        assert torch.equal(ref.aggregate(X, "phocas", f=f, trim=0), ref.phocas(X, f, trim=0))


def test_ties_go_to_the_lower_rank():
    # centre 2 (median); 0 and 4 are equally far: strict "<" keeps the lower rank
    X = torch.tensor([[0.0], [2.0], [4.0]])
    assert float(ref.mean_around(X, 1, 1, 2)) == 1.0                 # {0, 2}, not {2, 4}
    # n = 5, keep = 3, centre 5: pairs (1, 8): 3 < 4 -> move; (4, 9): 4 < 1 false
    X = torch.tensor([[1.0], [4.0], [5.0], [8.0], [9.0]])
    assert float(ref.mean_around(X, 2, 1, 3)) == pytest.approx((4 + 5 + 8) / 3)
    # exact tie on the second pair: (4, 6) around 5 -> stays on the lower rank
    X = torch.tensor([[0.0], [4.0], [5.0], [6.0], [7.0]])
    # pair 0: (6 - 5) < (5 - 0) true; pair 1: (7 - 5) < (5 - 4) false -> window [1, 4)
    assert float(ref.mean_around(X, 2, 1, 3)) == 5.0
    X = torch.tensor([[3.0], [4.0], [5.0], [6.0], [7.0]])
    # pair 0: (6 - 5) < (5 - 3) true; pair 1: (7 - 5) < (5 - 4) false
    assert float(ref.mean_around(X, 2, 1, 3)) == 5.0
    X = torch.tensor([[4.0], [4.0], [5.0], [6.0], [6.0]])
    # pair 0: 1 < 1 false -> window [0, 3)
    assert float(ref.mean_around(X, 2, 1, 3)) == pytest.approx(13 / 3)
    # all equal
    assert float(ref.mean_around(torch.full((6, 1), 2.5), 2, 2, 4)) == 2.5


@pytest.mark.parametrize("n", [3, 4, 8, 9])
def test_keep_n_and_f0_are_the_mean(n):
    X = torch.randn(n, 65, generator=torch.Generator().manual_seed(n))
    want = X.double().mean(0)
    torch.testing.assert_close(ref.mean_around(X, 0, 1, n).double(), want, rtol=0, atol=1e-6)
    torch.testing.assert_close(ref.meamed(X, 0).double(), want, rtol=0, atol=1e-6)
    torch.testing.assert_close(ref.phocas(X, 0).double(), want, rtol=0, atol=1e-6)
    out = torch.empty(65)
    K.agg_update(X, combine="sorted", lo=0, cnt=1, gout=out, keep=n)
    torch.testing.assert_close(out.double(), want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("bad", [(NAN,), (INF,), (-INF,), (-INF, INF), (NAN, -INF), (INF, INF),
                                 (-INF, -INF)])
@pytest.mark.parametrize("rule", ["meamed", "phocas"])
def test_nonfinite_contract(rule, bad):
    """A finite centre and at most f non-finite values per coordinate, on either side in any
    mix: no non-finite value reaches the output, and the result is the rule on the finite
    values' window."""
    n, f, D = 9, 2, 64
    g = torch.Generator().manual_seed(len(bad))
    X = torch.randn(n, D, generator=g)
    for d in range(D):
        for j, v in enumerate(bad):
            X[(d + 3 * j) % n, d] = v
    got = ref.aggregate(X, rule, f=f)
    assert bool(torch.isfinite(got).all())
    # the non-finite values are the farthest from any finite centre: with exactly f of them the
    # result is the mean of the finite values
    if len(bad) == f:
        fin = torch.where(torch.isfinite(X), X, torch.zeros_like(X)).double().sum(0) / (n - f)
        torch.testing.assert_close(got.double(), fin, rtol=0, atol=1e-6)
    assert torch.equal(K.aggregate(X, rule, f=f), got)


# --------------------------------------------------------------------------- ops
def test_near_range_and_coord_rules():
    assert K.COORD_RULES == ("median", "trimmed_mean", "meamed", "phocas")
    assert K.near_range("meamed", 8, 2) == (3, 2, 6)
    assert K.near_range("meamed", 9, 4) == (4, 1, 5)
    assert K.near_range("phocas", 8, 2) == (2, 4, 6)
    assert K.near_range("phocas", 8, 2, trim=1) == (1, 6, 6)
    assert K.near_range("median", 8, 2) == (3, 2, 0)
    assert K.near_range("trimmed_mean", 8, 2) == (2, 4, 0)
    for rule, n, f, trim in (("meamed", 8, 4, None), ("phocas", 8, 4, None), ("phocas", 8, 1, 4)):
        with pytest.raises(ValueError):
            K.near_range(rule, n, f, trim)


@pytest.mark.parametrize("rule", ["meamed", "phocas"])
def test_agg_update_keep_cpu(rule):
    n, f, D = 8, 2, 131
    g = torch.Generator().manual_seed(3)
    X = torch.randn(n + 1, D + 5, generator=g)
    lo, cnt, keep = K.near_range(rule, n, f)
    want = ref.aggregate(X[:n, :D], rule, f=f)
    out = torch.empty(D)
    K.agg_update(X, combine="sorted", lo=lo, cnt=cnt, n=n, D=D, gout=out, keep=keep)
    assert torch.equal(out, want)
    assert torch.equal(K.aggregate(X[:n, :D], rule, f=f), want)
    # keep=None / 0 is the plain window
    K.agg_update(X, combine="sorted", lo=lo, cnt=cnt, n=n, D=D, gout=out)
    plain = out.clone()
    K.agg_update(X, combine="sorted", lo=lo, cnt=cnt, n=n, D=D, gout=out, keep=0)
    assert torch.equal(out, plain) and not torch.equal(plain, want)
    # with an optimizer, through the multi-segment wrapper
    m = torch.randn(D, generator=g)
    m2 = m.clone()
    po, po2 = torch.empty(D), torch.empty(D)
    opt = K.OptArgs(kind="sgd", lr=0.1)
    K.agg_update(X, combine="sorted", lo=lo, cnt=cnt, n=n, D=D, opt=opt, master=m, param_out=po,
                 keep=keep)
    K.agg_update_multi([(X, 64, 0, po2[:64]), (X[:, 64:], D - 64, 64, po2[64:])], combine="sorted",
                       lo=lo, cnt=cnt, n=n, opt=opt, master=m2, keep=keep)
    assert torch.equal(m, m2) and torch.equal(po, po2)
    # the mixed form runs the rule on the mixed rows
    M = ref.nnm_matrix(ref.gram(X[:n, :D]), n, f).float()
    K.agg_update(X, combine="sorted", lo=lo, cnt=cnt, n=n, D=D, gout=out, mix=M, keep=keep)
    torch.testing.assert_close(out, ref.aggregate(X[:n, :D], rule, f=f, pre="nnm"), rtol=1e-5,
                               atol=1e-6)
    torch.testing.assert_close(K.aggregate(X[:n, :D], rule, f=f, pre="nnm"), out, rtol=1e-5,
                               atol=1e-6)
    for kw in (dict(combine="weighted", keep=keep), dict(combine="sorted", keep=n + 1),
               dict(combine="sorted", keep=-1), dict(combine="sorted", keep=3)):
        with pytest.raises(ValueError):
            K.agg_update(X, lo=lo, cnt=cnt, n=n, D=D, gout=out, **kw)


# --------------------------------------------------------------------------- config
def test_config_validation():
    TrainConfig().override(["agg.rule=meamed", "agg.f=2"]).validate(8)
    TrainConfig().override(["agg.rule=phocas", "agg.f=2"]).validate(8)
    TrainConfig().override(["agg.rule=phocas", "agg.f=2", "agg.trim=3"]).validate(8)
    TrainConfig().override(["agg.rule=meamed", "agg.f=31"]).validate(64)
    for rule in ("meamed", "phocas"):
        c = TrainConfig().override([f"agg.rule={rule}", "agg.f=4"])
        with pytest.raises(ValueError, match="n > 2f"):
            c.validate(8)
        with pytest.raises(ValueError, match="at most 64"):
            TrainConfig().override([f"agg.rule={rule}", "agg.f=2"]).validate(65)
        nnm = TrainConfig().override([f"agg.rule={rule}", "agg.f=2", "agg.pre=nnm",
                                      "topology.kind=sharded"])
        nnm.validate(32)
        with pytest.raises(ValueError, match="at most 32"):
            nnm.validate(33)
    with pytest.raises(ValueError, match="2\\*trim"):
        TrainConfig().override(["agg.rule=phocas", "agg.f=2", "agg.trim=4"]).validate(8)
    # meamed does not read trim
    TrainConfig().override(["agg.rule=meamed", "agg.f=2", "agg.trim=4"]).validate(8)


# --------------------------------------------------------------------------- engine
def _cfg(rule, topo, V=5, f=1, pre="none", wm=False, steps=6):
    cfg = TrainConfig()
    cfg.dtype = "fp32"
    cfg.virtual_workers = V
    cfg.agg.rule = rule
    cfg.agg.f = f
    cfg.agg.pre = pre
    cfg.topology.kind = topo
    cfg.topology.bucket_mb = 0.002      # several buckets even for the tiny MLP
    cfg.optim.lr = 0.1
    cfg.optim.momentum = 0.9
    cfg.optim.worker_momentum = wm
    cfg.batch_per_worker = 16
    cfg.model.extra = {"classes": 2}
    cfg.steps = steps
    return cfg


def _trainer(cfg):
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.trainer.trainer import ConsensusTrainer
    return ConsensusTrainer(cfg, info=DistInfo(0, 1, 0, CPU, "none"))


def _params(tr):
    return torch.cat([p.detach().reshape(-1).float() for p in tr.model.parameters()])


_RUNS = {}


def _fit(rule, topo, pre="none", wm=False):
    key = (rule, topo, pre, wm)
    if key not in _RUNS:
        tr = _trainer(_cfg(rule, topo, pre=pre, wm=wm))
        res = tr.fit(6, log_every=0)
        _RUNS[key] = (_params(tr).clone(), res["history"])
        tr.close()
    return _RUNS[key]


@pytest.mark.parametrize("pre,wm", [("none", False), ("nnm", False), ("none", True)])
@pytest.mark.parametrize("rule", ["meamed", "phocas"])
def test_engine_trains_and_topologies_agree(rule, pre, wm):
    a, ha = _fit(rule, "sharded", pre, wm)
    b, hb = _fit(rule, "allgather", pre, wm)
    assert bool(torch.isfinite(a).all()) and all(math.isfinite(h) for h in ha)
    assert torch.equal(a, b) and ha == hb
    # not the median's run, nor the trimmed mean's
    for other in ("median", "trimmed_mean"):
        assert not torch.equal(a, _fit(other, "sharded", pre, wm)[0])


@pytest.mark.parametrize("rule", ["meamed", "phocas"])
def test_engine_step_matches_hand_computation(rule):
    from consensusml_amd.parallel.dist import DistInfo
    from consensusml_amd.parallel.engine import ConsensusEngine
    n, f, lr = 8, 2, 0.1
    torch.manual_seed(0)
    cfg = _cfg(rule, "sharded", V=n, f=f)
    cfg.topology.bucket_mb = 0.004
    cfg.optim.lr = lr
    e = ConsensusEngine(torch.nn.Linear(64, 64), cfg, DistInfo())
    assert len(e.flat.buckets) >= 2
    total = e.flat.total
    g = torch.Generator().manual_seed(11)
    X = torch.randn(total, generator=g) + 0.3 * torch.randn(n, total, generator=g)
    X[:f] *= -10.0
    p0 = e.master.clone()
    e.zero_grad()
    e.flat.flat_grad.copy_(X.to(e.flat.flat_grad.dtype))
    e._flushed = {b.index for b in e.flat.buckets}
    e.step()
    lo, cnt, keep = K.near_range(rule, n, f)
    agg = brute_force(e.flat.flat_grad, lo, cnt, keep)
    want = p0.double() - lr * agg                # first SGD step: the buffer is the gradient
    torch.testing.assert_close(e.master.double(), want, rtol=1e-5, atol=1e-6)
    out = e._aggregate_only(e.flat.buckets[0], e._rows(e.flat.buckets[0]),
                            e._bucket_cols()[0][2])
    b0 = e.flat.buckets[0]
    lo_c, hi_c = e._local_range(b0, e._bucket_cols()[0][2])
    torch.testing.assert_close(out.double(), agg[lo_c:hi_c], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("rule,pre,wm", [("meamed", "none", True), ("phocas", "nnm", False)])
def test_checkpoint_resume_bit_identical(tmp_path, rule, pre, wm):
    cfg = _cfg(rule, "sharded", pre=pre, wm=wm)
    full = _trainer(cfg)
    full.fit(6, log_every=0)
    a = _trainer(cfg)
    a.fit(3, log_every=0)
    a.save(str(tmp_path / "ck"))
    b = _trainer(cfg)
    b.load(str(tmp_path / "ck"))
    b.fit(6, log_every=0)
    assert torch.equal(_params(b), _params(full))
    for t in (full, a, b):
        t.close()


@pytest.mark.parametrize("topo", ["sharded", "allgather"])
def test_consensus_table(topo):
    """The table's distance-to-aggregate column goes through ``_aggregate_only``."""
    pytest.importorskip("pandas")
    tr = _trainer(_cfg("phocas", topo))
    tr.fit(1, log_every=0)
    tr.engine.record_stats = True
    tr.train_step()
    df = tr.consensus_table()
    body = df.iloc[:-3]
    assert len(body) > 0 and bool((body["agg_norm"] > 0).all())
    assert bool((body[[f"dist_to_agg_w{i}" for i in range(5)]] > 0).all().all())
    tr.close()
