"""Nearest-neighbour mixing (``agg.pre=nnm``) on the CPU path: the mixing matrix, every rule on
the mixed rows against the rule applied directly to ``M @ X``, the config errors and one engine
step against the same step computed by hand from the worker rows."""
import pytest
import torch

from consensusml_amd import TrainConfig
from consensusml_amd.ops import kernels as K
from consensusml_amd.ops import reference as ref
from consensusml_amd.parallel.dist import DistInfo
from consensusml_amd.parallel.engine import ConsensusEngine

NNM_RULES = ("krum", "multi_krum", "geomed", "centered_clip", "median", "trimmed_mean")


def _rows(n, D, seed, outliers=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, D, generator=g)
    if outliers:
        X[-outliers:] += 3.0
    return X


# --------------------------------------------------------------------------- nnm_matrix
@pytest.mark.parametrize("n,f", [(8, 2), (9, 3), (5, 1), (16, 5)])
def test_nnm_matrix_rows(n, f):
    X = _rows(n, 40, n)
    M = ref.nnm_matrix(ref.gram(X), n, f)
    assert M.dtype == torch.float64 and tuple(M.shape) == (n, n)
    assert torch.equal(M.sum(1), torch.ones(n, dtype=torch.float64)) or \
        torch.allclose(M.sum(1), torch.ones(n, dtype=torch.float64), rtol=0, atol=1e-15)
    assert bool((torch.diagonal(M) > 0).all())             # the diagonal is always taken
    assert bool(((M > 0).sum(1) == n - f).all())            # exactly n - f entries ...
    assert bool(((M == 0) | (M == 1.0 / (n - f))).all())    # ... of 1 / (n - f)
    # the entries are the n - f nearest rows
    D = ref.sq_dists_from_gram(ref.gram(X))
    for i in range(n):
        near = set(torch.argsort(D[i], stable=True)[: n - f].tolist())
        assert set(torch.nonzero(M[i]).flatten().tolist()) == near


def test_nnm_matrix_ties_go_to_the_lower_index():
    # rows 1, 3, 4 and 6 are one vector: equal distances everywhere
    X = _rows(8, 16, 3)
    X[3] = X[1]
    X[4] = X[1]
    X[6] = X[1]
    M = ref.nnm_matrix(ref.gram(X), 8, 5)        # k = 3 of the 4 copies
    assert torch.nonzero(M[1]).flatten().tolist() == [1, 3, 4]
    assert torch.nonzero(M[3]).flatten().tolist() == [1, 3, 4]
    assert torch.nonzero(M[4]).flatten().tolist() == [1, 3, 4]
    # row 6 keeps itself ahead of the equally near copies, then the lowest indices
    assert torch.nonzero(M[6]).flatten().tolist() == [1, 3, 6]
    # a far row: the tie between the copies on its k-th place also goes to the lower index
    far = torch.nonzero(M[0]).flatten().tolist()
    copies = [j for j in far if j in (1, 3, 4, 6)]
    assert copies == [1, 3, 4, 6][: len(copies)]


@pytest.mark.parametrize("badval", [float("nan"), float("inf")])
def test_nnm_matrix_bad_row(badval):
    n, f = 8, 2
    X = _rows(n, 24, 1)
    X[2, 5] = badval
    M = ref.nnm_matrix(ref.gram(X), n, f)
    e = torch.zeros(n, dtype=torch.float64)
    e[2] = 1.0
    assert torch.equal(M[2], e)                              # stays as it is
    assert bool((M[:, 2] == e).all())                        # nobody's neighbour
    good = [i for i in range(n) if i != 2]
    assert bool(((M[good] > 0).sum(1) == n - f).all())


def test_nnm_matrix_fewer_good_rows_than_k():
    n, f = 8, 2                      # k = 6, only 4 good rows
    X = _rows(n, 24, 2)
    X[[0, 3, 5, 6]] = float("nan")
    M = ref.nnm_matrix(ref.gram(X), n, f)
    good = [1, 2, 4, 7]
    want = torch.zeros(n, dtype=torch.float64)
    want[good] = 0.25
    for i in good:
        assert torch.equal(M[i], want)
    for i in (0, 3, 5, 6):
        assert float(M[i, i]) == 1.0 and float(M[i].sum()) == 1.0


def test_nnm_matrix_f0_is_the_mean():
    M = ref.nnm_matrix(ref.gram(_rows(7, 12, 4)), 7, 0)
    assert torch.equal(M, torch.full((7, 7), 1.0 / 7, dtype=torch.float64))


def test_nnm_matrix_reads_the_worker_block_only():
    """Centered clipping's Gram has the previous aggregate as row n."""
    X = _rows(9, 20, 6)
    assert torch.equal(ref.nnm_matrix(ref.gram(X), 8, 2), ref.nnm_matrix(ref.gram(X[:8]), 8, 2))
    E = ref.nnm_extend(ref.nnm_matrix(ref.gram(X), 8, 2), 9)
    assert float(E[8, 8]) == 1.0 and float(E[8, :8].abs().sum()) == 0.0 \
        and float(E[:8, 8].abs().sum()) == 0.0


# --------------------------------------------------------------------------- rules on mixed rows
@pytest.mark.parametrize("n,f", [(8, 2), (9, 3)])
@pytest.mark.parametrize("rule", NNM_RULES)
def test_aggregate_nnm_equals_rule_on_mixed_rows(rule, n, f):
    X = _rows(n, 203, 10 * n + f, outliers=f)
    M = ref.nnm_matrix(ref.gram(X), n, f)
    Y = M @ X.double()                                   # the mixed rows in float64
    want = ref.aggregate(Y, rule, f=f)
    got = K.aggregate(X, rule, f=f, pre="nnm")
    assert got.dtype == torch.float32
    torch.testing.assert_close(got.double(), want.double(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ref.aggregate(X, rule, f=f, pre="nnm").double(), want.double(),
                               rtol=1e-5, atol=1e-5)
    # the mixing does something on these rows (Multi-Krum's n - f honest rows each mix to the
    # mean of the same n - f rows, which is what the plain rule returns)
    if rule != "multi_krum":
        assert float((K.aggregate(X, rule, f=f) - got).abs().max()) > 1e-3


def test_pre_none_is_the_default():
    X = _rows(8, 50, 0, outliers=2)
    for rule in NNM_RULES:
        assert torch.equal(K.aggregate(X, rule, f=2), K.aggregate(X, rule, f=2, pre="none"))


def test_robust_weights_nnm_outputs_refer_to_mixed_rows():
    n, f = 8, 2
    X = _rows(n, 64, 5, outliers=f)
    G = ref.gram(X)
    M = ref.nnm_matrix(G, n, f)
    mix = torch.zeros(n, n)
    sel = torch.zeros(n + 1, dtype=torch.int32)
    scores = torch.zeros(n, dtype=torch.float64)
    counts = torch.zeros(n, dtype=torch.float64)
    w = K.robust_weights(G, "krum", n, f, sel=sel, scores=scores, sel_counts=counts, pre="nnm",
                         mix_out=mix)
    assert torch.equal(mix, M.float())
    Gm = ref.gram(M @ X.double())
    pick = int(torch.argmin(ref.krum_scores(Gm, f)))
    assert sel[:n].tolist() == [int(i == pick) for i in range(n)]
    assert counts.tolist() == [float(i == pick) for i in range(n)]
    torch.testing.assert_close(scores, ref.krum_scores(Gm, f), rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(w.double(), M[pick], rtol=0, atol=1e-7)   # M^T e_pick
    with pytest.raises(ValueError):
        K.robust_weights(G, "mean", n, f, pre="nnm")
    with pytest.raises(ValueError):
        K.robust_weights(G, "krum", n, f, pre="mixing")
    with pytest.raises(ValueError):
        K.robust_weights(G, "nnm_only", n, f, mix_out=mix)


def test_agg_update_mix_cpu_zero_entry_rule():
    """A general linear pre-mix: a zero entry contributes nothing even where x_j is NaN."""
    n, D = 5, 33
    g = torch.Generator().manual_seed(8)
    X = torch.randn(n, D, generator=g)
    M = torch.rand(n, n, generator=g)
    M[:, 3] = 0.0
    M = M / M.sum(1, keepdim=True)
    want = ref.coord_median(M @ X)
    X[3] = float("nan")
    out = torch.empty(D)
    K.agg_update(X, combine="sorted", lo=2, cnt=1, gout=out, mix=M)
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        K.agg_update(X, combine="weighted", gout=out, mix=M)
    with pytest.raises(ValueError):
        K.agg_update(X, combine="sorted", lo=2, cnt=1, gout=out, mix=M.double())
    with pytest.raises(ValueError):
        K.agg_update(X, combine="sorted", lo=2, cnt=1, gout=out, mix=M[:4, :4].contiguous())


# --------------------------------------------------------------------------- config
def _cfg(rule="krum", n_f=2, topo="sharded", pre="nnm"):
    cfg = TrainConfig()
    cfg.agg.rule = rule
    cfg.agg.f = n_f
    cfg.agg.pre = pre
    cfg.topology.kind = topo
    return cfg


def test_validate_errors():
    assert TrainConfig().agg.pre == "none"
    _cfg().validate(8)
    _cfg("trimmed_mean").validate(32)
    _cfg("krum").validate(64)                    # Gram rules keep their limit
    with pytest.raises(ValueError, match="pre-aggregation"):
        _cfg(pre="mixing").validate(8)
    for rule in ("mean", "bulyan"):
        with pytest.raises(ValueError, match="nnm"):
            _cfg(rule, n_f=1).validate(8)
    for rule in ("median", "geomed"):
        with pytest.raises(ValueError, match="n > 2f"):
            _cfg(rule, n_f=4).validate(8)
    for rule in ("median", "trimmed_mean"):
        with pytest.raises(ValueError, match="at most 32"):
            _cfg(rule).validate(33)
    with pytest.raises(ValueError, match="at most 64"):
        _cfg("krum").validate(65)
    for topo in ("gossip", "allreduce"):
        with pytest.raises(ValueError, match="topology"):
            _cfg("median", topo=topo).validate(8)
    cfg = TrainConfig().override(["agg.pre=nnm", "agg.rule=median", "agg.f=2"])
    assert cfg.agg.pre == "nnm" and cfg.to_dict()["agg"]["pre"] == "nnm"


# --------------------------------------------------------------------------- engine
@pytest.mark.parametrize("rule", ["krum", "trimmed_mean"])
def test_engine_step_matches_hand_computation(rule):
    n, f, lr = 8, 2, 0.1
    torch.manual_seed(0)
    cfg = TrainConfig()
    cfg.virtual_workers = n
    cfg.agg.rule = rule
    cfg.agg.f = f
    cfg.agg.pre = "nnm"
    cfg.topology.kind = "sharded"
    cfg.topology.bucket_mb = 0.004
    cfg.optim.name = "sgd"
    cfg.optim.lr = lr
    cfg.optim.momentum = 0.9
    e = ConsensusEngine(torch.nn.Linear(64, 64), cfg, DistInfo())
    assert len(e.flat.buckets) >= 2
    total = e.flat.total
    g = torch.Generator().manual_seed(11)
    base = torch.randn(total, generator=g)
    X = base + 0.3 * torch.randn(n, total, generator=g)
    X[:f] = -0.1 * X[f:].mean(0)                 # two colluders send one vector (IPM)
    p0 = e.master.clone()
    e.zero_grad()
    e.flat.flat_grad.copy_(X.to(e.flat.flat_grad.dtype))
    e._flushed = {b.index for b in e.flat.buckets}
    e.step()
    # by hand, from the worker rows
    Xd = e.flat.flat_grad.double()
    M = ref.nnm_matrix(Xd @ Xd.t(), n, f)
    Y = M @ Xd
    if rule == "krum":
        pick = int(torch.argmin(ref.krum_scores(Y @ Y.t(), f)))
        agg = Y[pick]
        assert e.sel[:n].tolist() == [int(i == pick) for i in range(n)]
    else:
        agg = Y.sort(dim=0).values[f:n - f].mean(0)
    torch.testing.assert_close(e.M.double(), M, rtol=0, atol=1e-7)
    want = p0.double() - lr * agg                # first SGD step: the buffer is the gradient
    torch.testing.assert_close(e.master.double(), want, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(e.flat.flat_param.double(), want, rtol=1e-5, atol=1e-6)
    # and it differs from the unmixed rule
    plain = (Xd[int(torch.argmin(ref.krum_scores(Xd @ Xd.t(), f)))] if rule == "krum"
             else Xd.sort(dim=0).values[f:n - f].mean(0))
    assert float((agg - plain).abs().max()) > 1e-3


def test_engine_rejects_nnm_on_gossip():
    cfg = TrainConfig()
    cfg.virtual_workers = 4
    cfg.agg.rule = "median"
    cfg.agg.f = 1
    cfg.agg.pre = "nnm"
    cfg.topology.kind = "gossip"
    with pytest.raises(ValueError, match="topology"):
        ConsensusEngine(torch.nn.Linear(8, 8), cfg, DistInfo())
