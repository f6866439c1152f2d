"""The nearest-to-centre sorted combine of ``agg_update.hip`` (``keep > 0``: MeaMed / Phocas)
against a float64 oracle written here, over its dispatch space: row types, NP buckets, vector body
and scalar tail, single / multi segment, unmixed / mixed, the optimizer cycle of ``agg_oracle``.

The oracle sorts the (sanitised, for the mixed form float64-mixed) rows, takes the centre c = mean
of ranks [lo, lo+cnt) and the window position j* = #{j < n-k : (s_{j+k} - c) < (c - s_j)}, and
returns per coordinate the window mean and the set of ADMISSIBLE windows:

* a coordinate is ambiguous when for some j |(s_{j+k} - c) - (c - s_j)| <= eps with
  eps = (cnt + 4) 2^-23 max|finite s| -- the forward error of the fp32 centre (cnt adds and the
  1/cnt multiply) and of the two subtractions, doubled; the mixed form adds 2 n 2^-23 max|finite s|
  for the fp32 mix. There any window between #{j : delta_j < -eps} and #{j : delta_j <= eps} is
  admissible; everywhere else only j* is;
* ``gout`` must match an admissible window within ``agg_oracle``'s bound (a), (k + 2) 2^-23 A (for
  the mixed form plus ``test_nnm_gpu``'s bound on the mixed values themselves);
* a case with more than 2 % ambiguous coordinates fails as vacuous.

State and ``param_out`` are checked as (b)-(e) of ``agg_oracle`` (fed with the kernel's own
``gout``); every element of X the call must not read is NaN.
"""
import math
import os

import pytest
import torch

from agg_oracle import (CORE_CYCLE, GUARD, OPTS, SENT, TOL_ADAM_M, TOL_ADAM_V, TOL_MASTER,
                        TOL_SGD_BUF, _guarded, _guards_intact, _on, _state, _tdt, _worker_rows,
                        step64)
from consensusml_amd import TrainConfig
from consensusml_amd.ops import kernels as K
from consensusml_amd.ops import reference as ref
from consensusml_amd.parallel.dist import DistInfo
from consensusml_amd.parallel.engine import ConsensusEngine
from meamed_golden import golden_calls

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
U23 = 2.0 ** -23
VACUITY_CAP = 0.02
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "meamed_plain_paths.pt")


# =========================================================================== oracle
def centre_window(centre, n, f):
    """(lo, cnt) of the centre: the median window (MeaMed) or the f-trimmed window (Phocas)."""
    if centre == "median":
        return ((n - 1) // 2, 1) if n % 2 else (n // 2 - 1, 2)
    if centre == "rank0":      # n = 2: the median ties every coordinate, the trimmed window is empty
        return 0, 1
    return f, n - 2 * f


def near64(Y, lo, cnt, keep, extra_terms=0):
    """Y: float64 [n, D] rows (NaN allowed). Returns (g [f+1, D], A [f+1, D], adm [f+1, D] bool,
    jstar [D], ambiguous [D] bool): mean and mean of |.| of every candidate window [t, t+keep),
    and which of them are admissible."""
    n, D = Y.shape
    f = n - keep
    S = torch.where(torch.isnan(Y), torch.full_like(Y, math.inf), Y).sort(dim=0).values
    c = S[lo:lo + cnt].sum(0) / cnt
    fin = torch.isfinite(S)
    maxabs = torch.where(fin, S.abs(), torch.zeros_like(S)).max(0).values
    eps = (cnt + 4 + extra_terms) * U23 * maxabs
    delta = (S[keep:] - c) - (c - S[:f])                   # [f, D]; inf - inf -> NaN
    up, dn = S[keep:] - c, c - S[:f]
    pred = up < dn
    jstar = pred.sum(0)
    close = torch.isfinite(delta) & (delta.abs() <= eps)
    amb = close.any(0)
    jmin = (pred & ~close).sum(0)
    jmax = (pred | close).sum(0)
    g, A, adm = [], [], []
    for t in range(f + 1):
        W = S[t:t + keep]
        g.append(W.sum(0) / keep)
        A.append(W.abs().sum(0) / keep)
        adm.append((jmin <= t) & (t <= jmax))
    return torch.stack(g), torch.stack(A), torch.stack(adm), jstar, amb


def check_gout(what, gout, Y, lo, cnt, keep, extra_terms=0, extra_bound=None):
    g, A, adm, jstar, amb = near64(Y, lo, cnt, keep, extra_terms)
    share = amb.double().mean().item()
    assert bool(torch.isfinite(gout).all()), f"{what}: gout not finite"
    pick = g.gather(0, jstar[None])[0]
    assert bool(torch.isfinite(pick).all()), f"{what}: oracle not finite"
    bound = (keep + 2) * U23 * A
    if extra_bound is not None:
        bound = bound + extra_bound[None]
    bound = torch.where(bound == 0, torch.full_like(bound, 2.0 ** -149), bound)
    err = (gout.double()[None] - g).abs() / bound                  # [f+1, D]
    err = torch.where(adm & torch.isfinite(err), err, torch.full_like(err, math.inf))
    best = err.min(0).values
    moved = (err.argmin(0) != jstar) & amb
    print(f"{what}: keep={keep} ambiguous {100 * share:.3f} % (other window taken on "
          f"{int(moved.sum())}), max |gout - g64| / bound = {best.max().item():.3f}")
    assert share <= VACUITY_CAP, f"{what}: {100 * share:.2f} % of the coordinates are ambiguous"
    assert best.max().item() <= 1.0, \
        f"{what}: gout error {best.max().item():.3f} of the bound on {int((best > 1).sum())} " \
        f"coordinates (first {int((best > 1).nonzero()[0])})"


def check_state(what, hyper, before, after):
    """agg_oracle's checks (b), (c), (e) on one segment, fed with the kernel's own gout."""
    m0, s10, s20 = before
    m1, s11, s21, gout, pout = after
    kind = hyper["kind"]
    if kind == "none":
        return
    d = lambda t: None if t is None else t.double()   # noqa: E731
    pe, s1e, s2e = step64(kind, d(m0), gout.double(), d(s10), d(s20),
                          **{k: v for k, v in hyper.items() if k != "kind"})
    assert bool(torch.isfinite(m1).all()), f"{what}: master not finite"
    torch.testing.assert_close(m1.double(), pe, rtol=TOL_MASTER[0], atol=TOL_MASTER[1])
    if kind == "sgd":
        if hyper.get("momentum"):
            torch.testing.assert_close(s11.double(), s1e, rtol=TOL_SGD_BUF[0], atol=TOL_SGD_BUF[1])
            assert bool(torch.isfinite(s11).all()), f"{what}: momentum buffer not finite"   # (e)
    else:
        torch.testing.assert_close(s11.double(), s1e, rtol=TOL_ADAM_M[0], atol=TOL_ADAM_M[1])
        torch.testing.assert_close(s21.double(), s2e, rtol=TOL_ADAM_V[0], atol=TOL_ADAM_V[1])
    assert torch.equal(pout, m1.to(pout.dtype)), f"{what}: param_out != master as {pout.dtype}"


def _mix_matrix(kind, gen, n, X, f):
    """fp32 [n, n]: 'nnm' through K.robust_weights(..., 'nnm_only') from the rows' Gram, or
    'dense' random, non-symmetric, row-stochastic, about 30 % zeros."""
    if kind == "nnm":
        M = torch.empty(n, n)
        K.robust_weights(ref.gram(X), "nnm_only", n, f, pre="nnm", mix_out=M)
        return M
    M = torch.rand(n, n, generator=gen) + 0.05
    M[torch.rand(n, n, generator=gen) < 0.3] = 0.0
    M[torch.arange(n), (torch.arange(n) + 1) % n] += 0.2
    return (M / M.sum(1, keepdim=True)).contiguous()


def _rows64(X, rows, n, D, M):
    """float64 rows the rule sees, and for the mixed form the bound on the mixed values' fp32
    error, max_i (n + 2) 2^-23 sum_j |M_ij| |x_j| (test_nnm_gpu)."""
    R = (X[rows.long()] if rows is not None else X[:n])[:, :D].double()
    if M is None:
        return R, None
    Md = M.double()
    return Md @ R, ((n + 2) * U23 * (Md.abs() @ R.abs())).max(0).values


def _poison(X, used, D, f, gen, kinds):
    """At most f non-finite values per coordinate, of every kind in ``kinds``, on rows that move
    with the coordinate."""
    n = len(used)
    for d in range(D):
        m = 1 + (d % f)
        for j in range(m):
            X[used[(d + 7 * j) % n], d] = kinds[(d // 3 + j) % len(kinds)]


# =========================================================================== single segment
def run_near(dev, dt, n, f, centre, D, optname, seed, mis="", rows=None, xrows=0, mix=None,
             pout="bf16", poison=None):
    gen = torch.Generator().manual_seed(seed)
    dtype = _tdt(dt)
    lo, cnt = centre_window(centre, n, f)
    keep = n - f
    used = list(rows) if rows else list(range(n))
    R = xrows if rows else n + 1
    flat, Xc, o, ld = _worker_rows(gen, dtype, n, D, used, R, mis)
    if poison:
        _poison(Xc, used, D, f, gen, poison)
    if mix == "nnm":
        # what the mixing is for: f rows away from the rest. (Honest-only N(0, 1) rows at n = 4
        # mix to two pairs of equal rows, whose median centre ties every coordinate exactly.)
        Xc[n - f:n, :D] += 3.0
    Mc = None if mix is None else _mix_matrix(mix, gen, n, Xc[:n, :D].double(), f)
    X = _on(dev, flat, o, R, ld)
    M = None if Mc is None else Mc.to(dev)
    rws = torch.tensor(rows, dtype=torch.int32, device=dev) if rows else None
    hyper = dict(OPTS[optname])
    kind = hyper["kind"]
    so = GUARD + (1 if mis == "state" else 0)
    po = GUARD + (1 if mis == "pout" else 0)
    m0 = s10 = s20 = mb = s1b = s2b = None
    if kind != "none":
        m0, s10, s20 = _state(gen, kind, hyper.get("first", False), D)
        mb = _guarded(m0, D, so, torch.float32, dev)
        if kind != "sgd" or hyper["momentum"]:
            s1b = _guarded(s10, D, so, torch.float32, dev)
        else:
            s10 = None
        if s20 is not None:
            s2b = _guarded(s20, D, so, torch.float32, dev)
    gb = _guarded(None, D, so, torch.float32, dev)
    pb = _guarded(None, D, po, _tdt(pout), dev)
    sl = lambda b, off: None if b is None else b[off:off + D]   # noqa: E731
    K.agg_update(X, combine="sorted", lo=lo, cnt=cnt, rows=rws, n=n, D=D, opt=K.OptArgs(**hyper),
                 master=sl(mb, so), s1=sl(s1b, so), s2=sl(s2b, so), param_out=sl(pb, po),
                 gout=sl(gb, so), mix=M, keep=keep)
    what = f"{dt} n={n} f={f} {centre} D={D} {optname} {mis} {mix or ''}"
    for name, b, off in (("master", mb, so), ("s1", s1b, so), ("s2", s2b, so), ("gout", gb, so),
                         ("param_out", pb, po)):
        if b is not None:
            assert _guards_intact(b, off, D), f"{what}: wrote outside {name}"      # (d)
    if kind == "none":
        assert bool(torch.isnan(pb[po:po + D]).all()), f"{what}: OPT_NONE wrote param_out"
    Y, mixb = _rows64(X, rws, n, D, M)
    check_gout(what, sl(gb, so), Y, lo, cnt, keep, extra_terms=2 * n if M is not None else 0,
               extra_bound=mixb)
    before = tuple(None if t is None else t.to(dev) for t in (m0, s10, s20))
    check_state(what, hyper, before, (sl(mb, so), sl(s1b, so), sl(s2b, so), sl(gb, so),
                                      sl(pb, po)))


NS = (3, 5, 8, 9, 16, 17, 32, 33, 64)


@pytest.mark.parametrize("centre", ["median", "trimmed"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_near_against_oracle(cuda, dt, n, centre):
    for f in sorted({1, (n - 1) // 2}):
        i = NS.index(n) + 2 * (centre == "trimmed") + 3 * (dt == "f32") + f
        run_near(cuda, dt, n, f, centre, 2051, CORE_CYCLE[i % len(CORE_CYCLE)], seed=5000 + i,
                 pout=("bf16", "f32")[i % 2])


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_near_opt_none_and_tiny_sizes(cuda, dt):
    run_near(cuda, dt, 8, 2, "median", 2051, "none", seed=5100)
    run_near(cuda, dt, 33, 16, "trimmed", 2051, "none", seed=5101)
    for D in (1, 7, 8):
        run_near(cuda, dt, 5, 1, "median", D, "sgd_plain", seed=5110 + D)
        run_near(cuda, dt, 2, 1, "rank0", D, "adam", seed=5120 + D)       # the NP = 2 bucket


@pytest.mark.parametrize("mis", ["xbase", "xstride", "state", "pout"])
@pytest.mark.parametrize("n,f", [(5, 2), (33, 8)])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_near_misaligned(cuda, dt, n, f, mis):
    run_near(cuda, dt, n, f, "median", 2051, "sgd_plain", seed=5200 + n, mis=mis)
    run_near(cuda, dt, n, f, "trimmed", 2051, "adamw", seed=5300 + n, mis=mis, pout="f32")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_near_rows_indirection(cuda, dt):
    run_near(cuda, dt, 7, 2, "trimmed", 2051, "adamw", seed=5400, rows=(9, 2, 11, 0, 5, 7, 4),
             xrows=12)


@pytest.mark.parametrize("mix", ["nnm", "dense"])
@pytest.mark.parametrize("n", [4, 8, 16, 32])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_near_mixed_against_oracle(cuda, dt, n, mix):
    f = (n - 1) // 3
    i = n + (mix == "dense") + 2 * (dt == "f32")
    run_near(cuda, dt, n, f, "median", 2051, CORE_CYCLE[i % len(CORE_CYCLE)], seed=5500 + i,
             mix=mix)
    run_near(cuda, dt, n, f, "trimmed", 2051, CORE_CYCLE[(i + 3) % len(CORE_CYCLE)],
             seed=5600 + i, mix=mix, pout="f32")


@pytest.mark.parametrize("centre", ["median", "trimmed"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_near_nonfinite_contract(cuda, dt, centre):
    """A finite centre and at most f non-finite values per coordinate (NaN, +-inf, either side,
    any mix): outputs stay finite and match the oracle's window. Columns [D, ld) and the unused
    row are NaN throughout (``_worker_rows``)."""
    inf, nan = math.inf, math.nan
    for n, f in ((5, 2), (9, 3), (33, 16), (64, 31)):
        for kinds in ((nan,), (inf,), (-inf,), (-inf, nan, inf)):
            run_near(cuda, dt, n, f, centre, 515, "sgd_nesterov", seed=5700 + n, poison=kinds)


# =========================================================================== multi segment
def run_near_multi(dev, dt, n, f, centre, Ds, optname, seed, mix=None):
    gen = torch.Generator().manual_seed(seed)
    dtype = _tdt(dt)
    lo, cnt = centre_window(centre, n, f)
    keep = n - f
    hyper = dict(OPTS[optname])
    offs, end = [], 0
    for i, D in enumerate(Ds):        # agg_oracle.run_multi_case's layout
        off = (end + 7) // 8 * 8 + (8 if i else 0)
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
        v[gap] = SENT
        return _guarded(v, total, GUARD, torch.float32, dev)

    mb, s1b, gb = state_buf(m0), state_buf(s10), state_buf(None)
    s2b = state_buf(s20) if s20 is not None else None
    Xs, pbs = [], []
    for D in Ds:
        flat, _, o, ld = _worker_rows(gen, dtype, n, D, list(range(n)), n + 1)
        Xs.append(_on(dev, flat, o, n + 1, ld))
        pbs.append(_guarded(None, D, GUARD, torch.bfloat16, dev))
    M = None if mix is None else _mix_matrix("dense", gen, n, None, f).to(dev)
    sl = lambda b: None if b is None else b[GUARD:GUARD + total]   # noqa: E731
    K.agg_update_multi([(X, D, off, pb[GUARD:GUARD + D])
                        for X, D, off, pb in zip(Xs, Ds, offs, pbs)],
                       combine="sorted", lo=lo, cnt=cnt, n=n, opt=K.OptArgs(**hyper),
                       master=sl(mb), s1=sl(s1b), s2=sl(s2b), gout=sl(gb), mix=M, keep=keep)
    gapd = gap.to(dev)
    for name, b in (("master", mb), ("s1", s1b), ("s2", s2b), ("gout", gb)):
        if b is not None:
            assert _guards_intact(b, GUARD, total), f"wrote outside {name}"
            assert bool((sl(b)[gapd] == SENT).all()), f"wrote between segments of {name}"
    for i, (X, D, off, pb) in enumerate(zip(Xs, Ds, offs, pbs)):
        assert _guards_intact(pb, GUARD, D), f"wrote outside param_out {i}"
        cut = lambda t: None if t is None else t[off:off + D]   # noqa: E731
        what = f"{dt} n={n} f={f} {centre} seg {i} (D={D}, off={off}) {mix or ''}"
        Y, mixb = _rows64(X, None, n, D, M)
        check_gout(what, cut(sl(gb)), Y, lo, cnt, keep,
                   extra_terms=2 * n if M is not None else 0, extra_bound=mixb)
        before = tuple(None if t is None else cut(t).to(dev) for t in (m0, s10, s20))
        check_state(what, hyper, before, (cut(sl(mb)), cut(sl(s1b)), cut(sl(s2b)), cut(sl(gb)),
                                          pb[GUARD:GUARD + D]))


def _near_vec(dt, n):
    """Elements per lane of the nearest-to-centre kernels (Form::vec, agg_update.hip)."""
    if n > 8:
        return 2
    return 8 if (dt == "bf16" and n <= 4) else 4


@pytest.mark.parametrize("n,f", [(8, 2), (33, 16)])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_near_multi(cuda, dt, n, f):
    vec = _near_vec(dt, n)
    run_near_multi(cuda, dt, n, f, "median", (4096, vec, 808, 520), "sgd_nesterov", 5800 + n)
    run_near_multi(cuda, dt, n, f, "trimmed", (4096, vec, 808, 520), "adamw", 5810 + n)
    # a ragged segment: per-segment launches
    run_near_multi(cuda, dt, n, f, "trimmed", (4096, 2051, 808, 520), "sgd_first", 5820 + n)


@pytest.mark.parametrize("n", [4, 8, 16, 32])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_near_mixed_multi(cuda, dt, n):
    f = (n - 1) // 3
    vec = 8 if (dt == "bf16" and n <= 4) else (4 if n <= 16 else 2)    # Form::vec, MIX
    run_near_multi(cuda, dt, n, f, "median", (4096, vec, 808, 520), "adamw", 5900 + n, mix="dense")
    run_near_multi(cuda, dt, n, f, "trimmed", (4096, 2051, 808, 520), "sgd_nesterov", 5910 + n,
                   mix="dense")


# =========================================================================== existing paths
def test_plain_paths_bit_identical_to_parent(cuda):
    """``keep=None``: median and trimmed mean (fp32 and bf16 rows, n = 5, 8, 33) give, bit for
    bit, what the commit before the nearest-to-centre combine gave on an MI355X. The file was
    recorded there with ``python tests/meamed_golden.py tests/golden/meamed_plain_paths.pt`` in a
    checkout of that commit (see ``meamed_golden.py``)."""
    want = torch.load(GOLDEN, weights_only=True)
    got = golden_calls(K, cuda)
    assert sorted(got) == sorted(want) and len(got) == 36
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key


# =========================================================================== bindings
def test_keep_argument_checks(cuda):
    X = torch.randn(8, 64, device=cuda)
    out = torch.empty(64, device=cuda)
    lib = K.lib()
    args = (X, 8, 64, None, 0, 3, 2, None, 0, None, None, None, None, out, 0.1, 0.0, 0.0, 0.9,
            0.999, 1e-8, 0.1, 1.0, 1.0, False, False)
    lib.agg_update(*args)                                   # the old positional call, up to first
    plain = out.clone()
    lib.agg_update(*args, None)                             # ... and up to mix
    assert torch.equal(out, plain)
    lib.agg_update(*args, None, 0)                          # keep = 0: the plain window
    assert torch.equal(out, plain)
    lib.agg_update(*args, None, 6)
    torch.testing.assert_close(out.cpu(), ref.mean_around(X.cpu(), 3, 2, 6), rtol=1e-6, atol=1e-6)
    assert not torch.equal(out, plain)
    lib.agg_update(*args, None, 8)                          # keep == n: the mean
    torch.testing.assert_close(out, X.mean(0), rtol=1e-6, atol=1e-6)
    for keep in (9, -1, 3):                                 # > n, negative, below n / 2
        with pytest.raises((RuntimeError, ValueError)):
            lib.agg_update(*args, None, keep)
    wargs = (X, 8, 64, None, 1, 0, 1, None, 0, None, None, None, None, out, 0.1, 0.0, 0.0, 0.9,
             0.999, 1e-8, 0.1, 1.0, 1.0, False, False)
    lib.agg_update(*wargs)
    with pytest.raises((RuntimeError, ValueError)):          # the weighted combine takes no keep
        lib.agg_update(*wargs, None, 6)
    margs = ([X], [64], [0], [torch.empty(64, dtype=torch.bfloat16, device=cuda)], 8, None, 0, 3,
             2, None, 0, None, None, None, out, 0.1, 0.0, 0.0, 0.9, 0.999, 1e-8, 0.1, 1.0, 1.0,
             False, False)
    lib.agg_update_multi(*margs)                            # the old positional call
    assert torch.equal(out, plain)
    lib.agg_update_multi(*margs, None, 6)
    torch.testing.assert_close(out.cpu(), ref.mean_around(X.cpu(), 3, 2, 6), rtol=1e-6, atol=1e-6)
    with pytest.raises((RuntimeError, ValueError)):
        lib.agg_update_multi(*margs, None, 9)
    for kw in (dict(combine="weighted", keep=6), dict(combine="sorted", keep=9)):
        with pytest.raises((RuntimeError, ValueError)):
            K.agg_update(X, lo=3, cnt=2, gout=out, **kw)


@pytest.mark.parametrize("pre", ["none", "nnm"])
@pytest.mark.parametrize("rule", ["meamed", "phocas"])
def test_aggregate_matches_cpu(cuda, rule, pre):
    gen = torch.Generator().manual_seed(9)
    X = torch.randn(9, 1031, generator=gen)
    X[-2:] += 3.0
    want = K.aggregate(X, rule, f=2, pre=pre)
    got = K.aggregate(X.to(cuda), rule, f=2, pre=pre).cpu()
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)


# =========================================================================== engine
@pytest.mark.parametrize("topo", ["sharded", "allgather"])
@pytest.mark.parametrize("rule", ["meamed", "phocas"])
def test_engine_step_matches_cpu_engine(cuda, rule, topo):
    """One step over 8 virtual workers' bf16 gradient rows, f = 2: the GPU engine against the CPU
    engine on the same rows, at the tolerances of
    test_engine_gpu.py::test_gpu_topologies_match_cpu_reference."""
    n, f = 8, 2

    def eng(dev):
        torch.manual_seed(0)
        cfg = TrainConfig()
        cfg.virtual_workers = n
        cfg.agg.rule = rule
        cfg.agg.f = f
        cfg.topology.kind = topo
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
    base = torch.randn(c.flat.total, generator=gen)
    X = base + 0.3 * torch.randn(n, c.flat.total, generator=gen)
    X[:f] *= -10.0
    X = X.to(torch.bfloat16)
    for e in (c, g):
        e.zero_grad()
        e.flat.flat_grad.copy_(X.to(e.device))
        e._flushed = {b.index for b in e.flat.buckets}
        e.step()
    assert not torch.equal(c.master, eng(CPU).master)
    torch.testing.assert_close(g.master.cpu(), c.master, rtol=2e-4, atol=2e-5)
    assert torch.equal(g.flat.flat_param, g.master.to(torch.bfloat16))
