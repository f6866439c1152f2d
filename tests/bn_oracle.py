"""Exact and fp64 oracles of the fused BatchNorm kernels (csrc/kernels/bn_act.hip) and the case
table of ``test_bn_oracle_cpu.py``, ``test_bn_exact_gpu.py`` and ``test_bn_exact_env_gpu.py`` (not
collected: no ``test_`` prefix). The reference half of this module (down to "the launches") is
plain torch on CPU or GPU tensors and never calls the extension.

Exact tier. Activations (x, x2, res, dy, dy2) are bf16 integers in [-4, 4] from seeded CPU
generators (so a CPU run sees the very inputs of the GPU run). Where a launch takes statistics,
mean is an integer in [-2, 2] and invstd in {1/4, 1/2, 1, 2}; gamma is in {+-1/2, +-1, +-3/2, +-2}
and beta a multiple of 1/4 in [-2, 2]. Then sc = gamma invstd is a multiple of 1/8 with |sc| <= 4,
bi = beta - mean sc a multiple of 1/8 with |bi| <= 10, z = x sc + bi (+ res) a multiple of 1/8 with
|z| <= 30 (two BNs: <= 52), xhat = (x - mean) invstd a multiple of 1/4 with |xhat| <= 12, dz = dy
(+ dy2) an integer with |dz| <= 8 and dz xhat a multiple of 1/4 with |dz xhat| <= 96: every fp32
operation of the kernels is exact, and a workgroup's fp32 partial sums stay below 2^24 units
(rpb <= 19 R rows at the largest case, 19 * 256 * 96 * 4 < 2^24); the fold over workgroups is
fp64. The results are therefore independent of summation order, FMA contraction and grid, and the
comparison is ``torch.equal``. The shifted statistics sums s = sum (x - x0), q = sum (x - x0)^2
are exact integers as well, so mean / invstd / running statistics are one fixed fp64 expression of
(s, q, M); the device may contract ``q / M - ms ms`` or the running update into an fma, which can
move the fp32 rounding of the result by one ulp at most: expected is bit equality, allowed is one
fp32 ulp per channel, and the number of channels that are not bit-equal is returned and printed.

The ``> 0`` convention of the ReLU mask. A quarter of the channels (c % 4 == 1) have beta = 0, and
at an eighth of their rows plus row 0 the inputs are planted so that z is exactly 0 (x = mean,
x2 = mean2, res = 0); ``eval_fwd`` / ``eval_fwd2`` / ``recomp_keep`` assert from the inputs alone
that at least 1 % of the z are exactly 0.

fp64 tier (dx, dx1, dx2, and the training forward's y and mask, which use non-dyadic mean /
invstd). The reference is the same formula in fp64 on the same inputs; the training forward starts
from the oracle's fp32 mean / invstd. The bound is

    |got - ref| <= 2^-8 |ref| + 4 * 2^-24 * S

where S is the sum of the absolute values of the terms of the expression. First term: the result
is stored as bf16 (8 significant bits: an ulp is 2^-7 of the binade), so rounding to nearest costs
at most 2^-8 |ref|, reached just above a power of two. Second term: the kernel forms the value in
a few fp32 operations, each correctly rounded (relative error <= 2^-24) with a result no larger
than S:
  forward   z = fma(x, sc, bi) (+ res) with sc = invstd gamma, bi = fma(-mean, sc, beta): four
            roundings (sc, bi, the fma, the residual add); S = |x sc| + |mean sc| + |beta| + |res|
            (two BNs: the sum of both BNs' terms).
  backward  dx = sc (dz - a - xhat b), a = sdz / M, b = sdzx / M; xhat is exact for dyadic
            statistics; roundings: 1 / M, the two products with it, dz - a, the fma with xhat b,
            the product with sc; S = |sc| (|dz| + |a| + |xhat b|). Each term passes through at most
            four of them on average; the strict first-order worst case, every rounding at its
            maximum and of the same sign, is 2^-24 |sc| (3 |dz| + 5 |a| + 4 |xhat b|), i.e. one
            more unit on |a| alone (none when M is a power of two: 1 / M is exact). The factor
            stays 4: the inputs are fixed by seed, so the comparison is deterministic.
Mask bits of the training forward are compared wherever |z_ref| > 4 * 2^-24 * S; the share of
elements left out by that rule must be at most 0.1 % per case (asserted). For that the training
cases draw beta from the odd multiples of 1/4 (second BN: multiples of 1/2), so that a channel
without variance (M = 1, or a constant column), where z = beta (+ res) up to rounding, is never
within the rule's reach of 0.

Cases. Rows are given in R = 2048 / C, the rows one workgroup covers per iteration; ``check_geometry``
asserts through ``bn_geometry`` / ``bn_settings`` that a case reaches the branch it is named for:
  S1  M = 1                 var = 0, the unbiased-variance branch
  S2  M = R - 1             fewer rows than row slots (none at R = 1)
  S3  M = 5 R + 1           nb = 1: the 4-row unrolled stats loop, the 1-row tail, ragged last trip
  S4  M = 37 R + 3          nb = 3 with a short last workgroup
  G1  M = 2048 R + R/2 + 1  apply_grid = the cap, the second row in flight taken by part of the grid
  G2  M = 4797 R + 1        nb = 300: the 8-slice unrolled fold and its remainder, a third apply trip
  G3  M = 19437 R + 1       nb = 1024, the workgroup cap, rpb = 19 R (19389 R + 1 gives nb = 1021)

Child mode: ``python bn_oracle.py '{"expect": {...}, "cases": [...]}'`` runs the named cases in the
environment it was started in and prints one JSON line per case; ``run_child`` starts it as a fresh
process and checks the settings it read and that every case passed.
"""
import functools
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENV_OF = {"bn_nt": "CML_BN_NT", "bn_grid_cap": "CML_BN_GRID_CAP"}
DEFAULTS = {"bn_nt": 0, "bn_grid_cap": 2048}
ALL_C = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)
U = 2.0 ** -24
EPS, MOMENTUM = 1e-5, 0.1
MIN_ZERO_SHARE = 0.01
MAX_LEFT_OUT = 0.001
GAMMAS = (-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0)
INVSTDS = (0.25, 0.5, 1.0, 2.0)


def rows(kind, C):
    R = 2048 // C
    return {"S1": 1, "S2": R - 1, "S3": 5 * R + 1, "S4": 37 * R + 3, "G1": 2048 * R + R // 2 + 1,
            "G2": 4797 * R + 1, "G3": 19437 * R + 1}[kind]


def _seed(*key):
    h = 1469598103
    for k in key:
        h = (h * 1000003 + int(k)) % (2 ** 31 - 1)
    return h


# ------------------------------------------------------------------------------------ the inputs
def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int8)


def _pick(values, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


def zero_channels(C):
    return torch.arange(C) % 4 == 1


@functools.lru_cache(maxsize=4)
def make_params(C, seed, train):
    """Per-channel parameters on the CPU: gamma / beta (bf16), dyadic mean / invstd (fp32) of two
    BNs, and non-trivial running statistics to start from."""
    p = {}
    for i, sfx in enumerate(("", "2")):
        p["gamma" + sfx] = _pick(GAMMAS, C, _seed(seed, 10 + i)).bfloat16()
        p["mean" + sfx] = _ints((C,), -2, 2, _seed(seed, 20 + i)).float()
        p["invstd" + sfx] = _pick(INVSTDS, C, _seed(seed, 30 + i))
        p["rmean" + sfx] = _ints((C,), -8, 8, _seed(seed, 40 + i)).float() * 0.25
        p["rvar" + sfx] = _ints((C,), 1, 12, _seed(seed, 50 + i)).float() * 0.25
    if train:   # never beta (+ beta2) (+ res) == 0: see the module docstring
        p["beta"] = ((2 * _ints((C,), -4, 3, _seed(seed, 60)).float() + 1) * 0.25).bfloat16()
        p["beta2"] = (_ints((C,), -4, 4, _seed(seed, 61)).float() * 0.5).bfloat16()
    else:
        zc = zero_channels(C)
        for i, sfx in enumerate(("", "2")):
            b = _ints((C,), -8, 8, _seed(seed, 60 + i)).float() * 0.25
            p["beta" + sfx] = torch.where(zc, torch.zeros(()), b).bfloat16()
    return p


def make_inputs(M, C, seed, train, names=("x", "x2", "res", "dy", "dy2")):
    """bf16 integer activations [M, C] on the CPU. Eval / backward inputs (not train) have the
    exact zeros of z planted in the zero channels."""
    t = {n: _ints((M, C), -4, 4, _seed(seed, 100 + i)) for i, n in
         enumerate(("x", "x2", "res", "dy", "dy2")) if n in names}
    if not train:
        p = make_params(C, seed, False)
        g = torch.Generator().manual_seed(_seed(seed, 99))
        plant = torch.rand(M, C, generator=g) < 0.125
        plant[0] = True
        plant &= zero_channels(C)
        for n, v in (("x", p["mean"]), ("x2", p["mean2"]), ("res", torch.zeros(C))):
            if n in t:
                t[n] = torch.where(plant, v.to(torch.int8), t[n])
    return {n: v.bfloat16() for n, v in t.items()}


# ------------------------------------------------------------------------------------ the oracle
def f32_exact(*ts):
    """Every fp64 tensor must equal its fp32 rounding (the kernel's fp32 operation is exact)."""
    for i, t in enumerate(ts):
        assert torch.equal(t.float().double(), t), f"intermediate {i} is not exact in fp32"


def pack_mask(pos):
    """bool [M, C] -> bytes [M, C / 8], bit k = channel 8 g + k."""
    M, C = pos.shape
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=pos.device)
    return (pos.view(M, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def unpack_mask(mask):
    M, G = mask.shape
    k = torch.arange(8, dtype=torch.int32, device=mask.device)
    return ((mask.to(torch.int32).unsqueeze(-1) >> k) & 1).bool().view(M, G * 8)


def ulp_diff(a, b):
    """Distance in fp32 ulps of two finite fp32 tensors."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape
    return (key(a) - key(b)).abs()


def f32(v):
    """A Python float rounded to fp32 and widened again, as the binding passes eps / momentum."""
    return float(torch.tensor(v, dtype=torch.float32))


def shifted_sums(x):
    """Exact integer s = sum (x - x0), q = sum (x - x0)^2 per channel (int64) and x0."""
    xi = x.to(torch.int64)
    assert torch.equal(xi.to(x.dtype), x), "x is not integer-valued"
    d = xi - xi[0]
    return d.sum(0), (d * d).sum(0), xi[0]


def train_stats(x, rmean0, rvar0, eps=EPS, momentum=MOMENTUM):
    """mean, invstd, running_mean, running_var (fp32) of a training BN over x [M, C], from the
    exact shifted sums; also the fp64 var."""
    M = x.shape[0]
    s, q, x0 = shifted_sums(x)
    ms = s.double() / M
    var = (q.double() / M - ms * ms).clamp_min(0.0)
    direct = x.double().var(0, unbiased=False)
    assert bool(((var - direct).abs() <= 1e-12 * direct).all()), "shifted variance != direct variance"
    mu = x0.double() + ms
    e, mom = f32(eps), f32(momentum)
    unb = var * float(M) / float(M - 1) if M > 1 else var
    return {"mean": mu.float(), "invstd": (1.0 / torch.sqrt(var + e)).float(),
            "rmean": ((1.0 - mom) * rmean0.double() + mom * mu).float(),
            "rvar": ((1.0 - mom) * rvar0.double() + mom * unb).float(), "var": var}


def affine(p, sfx=""):
    sc = p["invstd" + sfx].double() * p["gamma" + sfx].double()
    ms = p["mean" + sfx].double() * sc
    bi = p["beta" + sfx].double() - ms
    return sc, ms, bi


def zero_share(z):
    share = float((z == 0).double().mean())
    assert share >= MIN_ZERO_SHARE, f"only {share:.4%} of the z are exactly 0"
    return share


def eval_fwd(x, res, p, relu):
    """Exact eval-mode forward: (y bf16, mask bytes, z fp64, share of z == 0)."""
    sc, ms, bi = affine(p)
    xs = x.double() * sc
    z0 = xs + bi
    z = z0 if res is None else z0 + res.double()
    f32_exact(sc, ms, bi, xs, z0, z)
    share = zero_share(z)
    y = (z.clamp_min(0.0) if relu else z).bfloat16()
    return y, pack_mask(z > 0), z, share


def eval_fwd2(x1, x2, p):
    """Exact y = relu(bn1(x1) + bn2(x2)): (y bf16, mask bytes, z fp64, share of z == 0)."""
    sc1, ms1, bi1 = affine(p)
    sc2, ms2, bi2 = affine(p, "2")
    bi = bi1 + bi2
    t = x2.double() * sc2
    t2 = t + bi
    u = x1.double() * sc1
    z = u + t2
    f32_exact(sc1, ms1, bi1, sc2, ms2, bi2, bi, t, t2, u, z)
    share = zero_share(z)
    return z.clamp_min(0.0).bfloat16(), pack_mask(z > 0), z, share


def recomp_keep(x, p):
    """bool [M, C]: fma(x, sc, bi) > 0, the backward's recomputed ReLU mask (no residual)."""
    sc, ms, bi = affine(p)
    z = x.double() * sc + bi
    f32_exact(sc, ms, bi, z)
    zero_share(z)
    return z > 0


def masked_dz(dy, dy2, keep):
    dz = dy.double() if dy2 is None else dy.double() + dy2.double()
    return dz if keep is None else torch.where(keep, dz, torch.zeros_like(dz))


def xhat(x, p, sfx=""):
    xh = (x.double() - p["mean" + sfx].double()) * p["invstd" + sfx].double()
    f32_exact(xh)
    return xh


def bwd_sums(dz, xh):
    """Exact sdz = sum dz, sdzx = sum dz xhat (fp64) and what the kernel stores of them."""
    sdz, sdzx = dz.sum(0), (dz * xh).sum(0)
    return {"sdz": sdz, "sdzx": sdzx, "sdz32": sdz.float(), "sdzx32": sdzx.float(),
            "dbeta": sdz.float().bfloat16(), "dgamma": sdzx.float().bfloat16()}


def dx_ref(dz, xh, sc, sdz, sdzx):
    """fp64 dx = sc (dz - sdz / M - xhat sdzx / M) and S, the sum of its terms' magnitudes."""
    M = dz.shape[0]
    a, b = sdz / M, sdzx / M
    ref = sc * (dz - a - xh * b)
    S = sc.abs() * (dz.abs() + a.abs() + (xh * b).abs())
    return ref, S


def train_fwd_ref(x, res, p, mean, invstd, relu):
    """fp64 z of the training forward from fp32 mean / invstd, and S."""
    sc = invstd.double() * p["gamma"].double()
    z = (x.double() - mean.double()) * sc + p["beta"].double()
    S = (x.double() * sc).abs() + (mean.double() * sc).abs() + p["beta"].double().abs()
    if res is not None:
        z = z + res.double()
        S = S + res.double().abs()
    return z, S


def train_fwd2_ref(x1, x2, p, st1, st2):
    pa = {"gamma": p["gamma"], "beta": p["beta"]}
    pb = {"gamma": p["gamma2"], "beta": p["beta2"]}
    z1, S1 = train_fwd_ref(x1, None, pa, st1["mean"], st1["invstd"], False)
    z2, S2 = train_fwd_ref(x2, None, pb, st2["mean"], st2["invstd"], False)
    return z1 + z2, S1 + S2


def close_report(got, ref, S, what):
    """max of |got - ref| / (2^-8 |ref| + 4 * 2^-24 S); raises above 1."""
    err = (got.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 4 * U * S
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, first "
                             f"at {i}: got {float(got[tuple(i)])} ref {float(ref[tuple(i)])} "
                             f"bound {float(bound[tuple(i)])}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def left_out(z, S):
    """bool: the mask bits the rule leaves out, and their share (asserted <= 0.1 %)."""
    out = ~(z.abs() > 4 * U * S)
    share = float(out.double().mean())
    assert share <= MAX_LEFT_OUT, f"{share:.4%} of the mask bits are left out"
    return out, share


def assert_equal(got, want, what):
    if got.shape != want.shape or not torch.equal(got, want):
        bad = ~(got == want)
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: "
                             f"got {float(got[tuple(i)])} want {float(want[tuple(i)])}")


def assert_ulp(got, want, what):
    """Allowed: 1 fp32 ulp per channel. Returns the number of channels not bit-equal."""
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    d = ulp_diff(got, want)
    assert int(d.max()) <= 1, f"{what}: {int((d > 1).sum())} channels off by more than 1 ulp " \
                              f"(max {int(d.max())}, first at {int((d > 1).nonzero()[0])})"
    return int((d != 0).sum())


# ------------------------------------------------------------------------------------ the launches
def _lib():
    from consensusml_amd.ops.native import lib
    return lib()


def settings():
    return dict(_lib().bn_settings())


def check_geometry(kind, C):
    """The case reaches the branch it is named for, in this process's settings."""
    M, R = rows(kind, C), 2048 // C
    nb, rpb, grid = (int(v) for v in _lib().bn_geometry(M, C))
    cap = settings()["bn_grid_cap"]
    blocks = -(-M // R)
    assert grid == (min(blocks, cap) if cap > 0 else blocks), (kind, C, grid, cap)
    assert nb == -(-M // rpb) and rpb % R == 0, (kind, C, nb, rpb)
    rstride = grid * R
    if kind == "S1":
        assert M == 1 and nb == 1 and grid == 1
    elif kind == "S2":
        assert 1 <= M < R and nb == 1 and grid == 1
    elif kind == "S3":
        assert nb == 1 and 4 * R < M <= 6 * R and (M - 1) % R == 0
    elif kind == "S4":
        assert nb == 3 and 0 < M - 2 * rpb < rpb
        if cap == 3:
            assert grid == 3 and M > 8 * rstride     # more than four two-row trips
    elif kind == "G1":
        if cap == 2048:     # the second row in flight exists for a part of the grid only
            assert grid == cap and rstride < M < rstride + rstride // 2 + 2
        elif cap == 0:
            assert grid == blocks > 2048 and M <= rstride
    elif kind == "G2":
        assert 256 < nb < 1024 and nb % 256 != 0
        if cap == 2048:
            assert grid == cap and M > 2 * rstride
    elif kind == "G3":
        assert nb == 1024 and rpb > 16 * R and M % rpb != 0
    return {"nb": nb, "rpb": rpb, "grid": grid}


@functools.lru_cache(maxsize=2)
def _data(kind, C, train, dev):
    """Inputs and parameters of a case on `dev` (shared, read only)."""
    M, seed = rows(kind, C), _seed(ord(kind[0]), int(kind[1]), C, int(train))
    names = ("x", "dy") if kind == "G3" else ("x", "x2", "res", "dy", "dy2")
    d = {k: v.to(dev) for k, v in make_inputs(M, C, seed, train, names).items()}
    d.update({k: v.to(dev) for k, v in make_params(C, seed, train).items()})
    return d


def poison(dev, *nbytes):
    """Fill throw-away tensors of the outputs' sizes with 0xFF and free them: a row the kernel
    does not write then reads as NaN instead of a cached earlier result."""
    ts = [torch.empty(max(int(n), 1), dtype=torch.uint8, device=dev).fill_(0xFF) for n in nbytes]
    del ts


def as4d(t):
    """[M, C] -> the same memory as [1, C, M, 1] channels_last."""
    M, C = t.shape
    return t.view(1, M, 1, C).permute(0, 3, 1, 2)


def as2d(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _stats_check(got, st, what, fig):
    for k in ("mean", "invstd", "rmean", "rvar"):
        fig["not_bit_equal"] += assert_ulp(got[k], st[k], f"{what} {k}")


def case_stats(dev, kind, C):
    """bn_stats: statistics and running statistics."""
    L, d, M = _lib(), _data(kind, C, True, dev), rows(kind, C)
    fig = {"not_bit_equal": 0}
    st = train_stats(d["x"], d["rmean"], d["rvar"])
    rm, rv = d["rmean"].clone(), d["rvar"].clone()
    poison(dev, 4 * C, 4 * C)
    mean, invstd = L.bn_stats(d["x"], rm, rv, EPS, MOMENTUM)
    _stats_check({"mean": mean, "invstd": invstd, "rmean": rm, "rvar": rv}, st, "bn_stats", fig)
    if M == 1:
        assert float(st["var"].abs().max()) == 0.0
    return fig


def case_train(dev, kind, C):
    """Training bn_fwd: statistics (1 ulp), y and mask in the fp64 tier."""
    L, d, M = _lib(), _data(kind, C, True, dev), rows(kind, C)
    fig = {"not_bit_equal": 0, "left_out": 0.0, "ratio": 0.0}
    st = train_stats(d["x"], d["rmean"], d["rvar"])
    for relu, use_res, want_mask in ((False, False, False), (True, False, False), (True, True, True)):
        what = f"train relu={relu} res={use_res}"
        res = d["res"] if use_res else None
        z, S = train_fwd_ref(d["x"], res, d, st["mean"], st["invstd"], relu)
        out, share = left_out(z, S)
        rm, rv = d["rmean"].clone(), d["rvar"].clone()
        poison(dev, 2 * M * C, M * C // 8)
        y, mean, invstd, mask = L.bn_fwd(d["x"], res, d["gamma"], d["beta"], rm, rv, None, None,
                                         EPS, MOMENTUM, relu, True, want_mask)
        _stats_check({"mean": mean, "invstd": invstd, "rmean": rm, "rvar": rv}, st, what, fig)
        fig["ratio"] = max(fig["ratio"], close_report(y, z.clamp_min(0.0) if relu else z, S, what + " y"))
        if want_mask:
            bad = (unpack_mask(mask) != (z > 0)) & ~out
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} mask bits differ"
            fig["left_out"] = max(fig["left_out"], share)
    return fig


EVAL_MODES = (("plain", False, False, False), ("relu", True, False, False), ("res", False, True, False),
              ("res_relu", True, True, False), ("res_relu_mask", True, True, True))


def case_eval(dev, kind, C):
    """Eval bn_fwd in its five instantiations: y and mask bit for bit."""
    L, d, M = _lib(), _data(kind, C, False, dev), rows(kind, C)
    fig = {"zero_share": 1.0}
    for name, relu, use_res, want_mask in EVAL_MODES:
        res = d["res"] if use_res else None
        y_want, m_want, _, share = eval_fwd(d["x"], res, d, relu)
        fig["zero_share"] = min(fig["zero_share"], share)
        poison(dev, 2 * M * C, M * C // 8)
        y, _, _, mask = L.bn_fwd(d["x"], res, d["gamma"], d["beta"], None, None, d["mean"],
                                 d["invstd"], EPS, MOMENTUM, relu, False, want_mask)
        assert_equal(y, y_want, f"eval {name} y")
        if want_mask:
            assert_equal(mask, m_want, f"eval {name} mask")
    return fig


# name, relu, mask, dres, dy2
BWD_VARIANTS = (("none", False, False, False, False), ("none_dres", False, False, True, False),
                ("recomp", True, False, False, False), ("recomp_dy2", True, False, False, True),
                ("mask", True, True, False, False), ("mask_dres", True, True, True, False),
                ("mask_dres_dy2", True, True, True, True))


def _bwd_oracle(d, relu, use_mask, use_dy2):
    """(mask bytes or None, dz, xhat, sums) of one backward variant."""
    mask = None
    if not relu:
        keep = None
    elif use_mask:
        _, mask, z, _ = eval_fwd(d["x"], d["res"], d, True)
        keep = z > 0
    else:
        keep = recomp_keep(d["x"], d)
    dz = masked_dz(d["dy"], d["dy2"] if use_dy2 else None, keep)
    xh = xhat(d["x"], d)
    return mask, dz, xh, bwd_sums(dz, xh)


def case_bwd(dev, kind, C, variants=BWD_VARIANTS):
    """bn_bwd: dgamma / dbeta / dres bit for bit, dx in the fp64 tier."""
    L, d, M = _lib(), _data(kind, C, False, dev), rows(kind, C)
    fig = {"ratio": 0.0}
    sc = affine(d)[0]
    for name, relu, use_mask, dres, use_dy2 in variants:
        mask, dz, xh, sums = _bwd_oracle(d, relu, use_mask, use_dy2)
        ref, S = dx_ref(dz, xh, sc, sums["sdz"], sums["sdzx"])
        poison(dev, 2 * M * C, 2 * M * C)
        dx, dg, db, dr = L.bn_bwd(d["dy"], d["dy2"] if use_dy2 else None, d["x"], mask, d["gamma"],
                                  d["beta"], d["mean"], d["invstd"], relu, dres)
        assert_equal(dg, sums["dgamma"], f"bwd {name} dgamma")
        assert_equal(db, sums["dbeta"], f"bwd {name} dbeta")
        if dres:
            assert_equal(dr, dz.bfloat16(), f"bwd {name} dres")
        fig["ratio"] = max(fig["ratio"], close_report(dx, ref, S, f"bwd {name} dx"))
    return fig


SUMS_VARIANTS = (("none", False, False, False), ("recomp", True, False, False),
                 ("recomp_dy2", True, False, True), ("mask", True, True, False),
                 ("mask_dy2", True, True, True))


def case_sums(dev, kind, C):
    """bn_bwd_sums bit for bit; bn_bwd_apply from the oracle's sums in the fp64 tier and equal to
    bn_bwd(relu, no mask).dx bit for bit. G3: the recomputed-mask sums only."""
    L, d, M = _lib(), _data(kind, C, False, dev), rows(kind, C)
    fig = {"ratio": 0.0}
    for name, relu, use_mask, use_dy2 in (SUMS_VARIANTS[1:2] if kind == "G3" else SUMS_VARIANTS):
        mask, _, _, sums = _bwd_oracle(d, relu, use_mask, use_dy2)
        poison(dev, 4 * C, 4 * C)
        sdz, sdzx = L.bn_bwd_sums(d["dy"], d["dy2"] if use_dy2 else None, d["x"], mask, d["gamma"],
                                  d["beta"], d["mean"], d["invstd"], relu)
        assert_equal(sdz, sums["sdz32"], f"sums {name} sdz")
        assert_equal(sdzx, sums["sdzx32"], f"sums {name} sdzx")
    if kind == "G3":
        return fig
    _, dz, xh, sums = _bwd_oracle(d, True, False, False)
    ref, S = dx_ref(dz, xh, affine(d)[0], sums["sdz"], sums["sdzx"])
    poison(dev, 2 * M * C)
    dx = L.bn_bwd_apply(d["dy"], d["x"], d["gamma"], d["beta"], d["mean"], d["invstd"],
                        sums["sdz32"], sums["sdzx32"])
    fig["ratio"] = close_report(dx, ref, S, "bn_bwd_apply dx")
    poison(dev, 2 * M * C)
    dx2 = L.bn_bwd(d["dy"], None, d["x"], None, d["gamma"], d["beta"], d["mean"], d["invstd"], True,
                   False)[0]
    assert_equal(dx, dx2, "bn_bwd_apply dx vs bn_bwd dx")
    return fig


def case_fwd2(dev, kind, C):
    """bn_fwd2 with mask: eval bit for bit; training statistics (1 ulp), y / mask in the fp64 tier."""
    L, M = _lib(), rows(kind, C)
    d = _data(kind, C, False, dev)
    fig = {"not_bit_equal": 0, "left_out": 0.0, "ratio": 0.0}
    y_want, m_want, _, fig["zero_share"] = eval_fwd2(d["x"], d["x2"], d)
    poison(dev, 2 * M * C, M * C // 8)
    out = L.bn_fwd2(as4d(d["x"]), as4d(d["x2"]), d["gamma"], d["beta"], d["gamma2"], d["beta2"], None,
                    None, None, None, d["mean"], d["invstd"], d["mean2"], d["invstd2"], EPS,
                    MOMENTUM, False, True)
    assert_equal(as2d(out[0]), y_want, "eval fwd2 y")
    assert_equal(out[5], m_want, "eval fwd2 mask")
    d = _data(kind, C, True, dev)
    st1 = train_stats(d["x"], d["rmean"], d["rvar"])
    st2 = train_stats(d["x2"], d["rmean2"], d["rvar2"])
    z, S = train_fwd2_ref(d["x"], d["x2"], d, st1, st2)
    lo, fig["left_out"] = left_out(z, S)
    rm1, rv1, rm2, rv2 = (d[k].clone() for k in ("rmean", "rvar", "rmean2", "rvar2"))
    poison(dev, 2 * M * C, M * C // 8)
    y, m1, i1, m2, i2, mask = L.bn_fwd2(as4d(d["x"]), as4d(d["x2"]), d["gamma"], d["beta"],
                                        d["gamma2"], d["beta2"], rm1, rv1, rm2, rv2, None, None, None,
                                        None, EPS, MOMENTUM, True, True)
    _stats_check({"mean": m1, "invstd": i1, "rmean": rm1, "rvar": rv1}, st1, "train fwd2 bn1", fig)
    _stats_check({"mean": m2, "invstd": i2, "rmean": rm2, "rvar": rv2}, st2, "train fwd2 bn2", fig)
    fig["ratio"] = close_report(as2d(y), z.clamp_min(0.0), S, "train fwd2 y")
    bad = (unpack_mask(mask) != (z > 0)) & ~lo
    assert not bool(bad.any()), f"train fwd2: {int(bad.sum())} mask bits differ"
    return fig


def case_bwd2(dev, kind, C):
    """bn_bwd2 with and without dy2: both BNs' dgamma / dbeta bit for bit, dx1 / dx2 fp64 tier."""
    L, d, M = _lib(), _data(kind, C, False, dev), rows(kind, C)
    fig = {"ratio": 0.0}
    _, mask, z, _ = eval_fwd2(d["x"], d["x2"], d)
    xh1, xh2 = xhat(d["x"], d), xhat(d["x2"], d, "2")
    c1 = d["gamma"].double() * d["invstd"].double()
    c2 = d["gamma2"].double() * d["invstd2"].double()
    for use_dy2 in (False, True):
        dz = masked_dz(d["dy"], d["dy2"] if use_dy2 else None, z > 0)
        s1, s2 = bwd_sums(dz, xh1), bwd_sums(dz, xh2)
        poison(dev, 2 * M * C, 2 * M * C)
        dx1, dg1, db1, dx2, dg2, db2 = L.bn_bwd2(
            as4d(d["dy"]), as4d(d["dy2"]) if use_dy2 else None, as4d(d["x"]), as4d(d["x2"]), mask,
            d["gamma"], d["gamma2"], d["mean"], d["invstd"], d["mean2"], d["invstd2"])
        what = f"bwd2 dy2={use_dy2}"
        for got, want, n in ((dg1, s1["dgamma"], "dgamma1"), (db1, s1["dbeta"], "dbeta1"),
                             (dg2, s2["dgamma"], "dgamma2"), (db2, s2["dbeta"], "dbeta2")):
            assert_equal(got, want, f"{what} {n}")
        for got, xh, c, s, n in ((dx1, xh1, c1, s1, "dx1"), (dx2, xh2, c2, s2, "dx2")):
            ref, S = dx_ref(dz, xh, c, s["sdz"], s["sdzx"])
            fig["ratio"] = max(fig["ratio"], close_report(as2d(got), ref, S, f"{what} {n}"))
    return fig


def case_chain(dev, kind, C):
    """The forward kernel's own mask fed to the backward (mask + dres + dy2)."""
    L, d, M = _lib(), _data(kind, C, False, dev), rows(kind, C)
    poison(dev, 2 * M * C, M * C // 8)
    mask = L.bn_fwd(d["x"], d["res"], d["gamma"], d["beta"], None, None, d["mean"], d["invstd"],
                    EPS, MOMENTUM, True, False, True)[3]
    _, dz, xh, sums = _bwd_oracle(d, True, True, True)
    ref, S = dx_ref(dz, xh, affine(d)[0], sums["sdz"], sums["sdzx"])
    poison(dev, 2 * M * C, 2 * M * C)
    dx, dg, db, dr = L.bn_bwd(d["dy"], d["dy2"], d["x"], mask, d["gamma"], d["beta"], d["mean"],
                              d["invstd"], True, True)
    assert_equal(dg, sums["dgamma"], "chain dgamma")
    assert_equal(db, sums["dbeta"], "chain dbeta")
    assert_equal(dr, dz.bfloat16(), "chain dres")
    return {"ratio": close_report(dx, ref, S, "chain dx")}


FAMILIES = {"stats": case_stats, "train": case_train, "eval": case_eval, "bwd": case_bwd,
            "sums": case_sums, "fwd2": case_fwd2, "bwd2": case_bwd2}
SHAPES = ([(k, C) for k in ("S1", "S2", "S3", "S4") for C in ALL_C if rows(k, C) >= 1] +
          [("G1", C) for C in (8, 64, 512, 2048)] + [("G2", C) for C in (64, 2048)])

CASES = {}
for _k, _C in SHAPES:
    for _f, _fn in FAMILIES.items():
        CASES[f"{_k}-C{_C}-{_f}"] = functools.partial(_fn, kind=_k, C=_C)
CASES["S4-C64-chain"] = functools.partial(case_chain, kind="S4", C=64)
for _C in (2048, 64):
    for _f in ("stats", "sums"):
        CASES[f"G3-C{_C}-{_f}"] = functools.partial(FAMILIES[_f], kind="G3", C=_C)
# the exact tier under the read-once switches
ENV_NAMES = [f"{k}-C{C}-{f}" for k in ("S3", "S4", "G1") for C in (8, 256, 2048)
             for f in ("stats", "eval", "bwd", "sums", "fwd2", "bwd2")]
for _n in ENV_NAMES:
    if _n not in CASES:
        _k, _c, _f = _n.split("-")
        CASES[_n] = functools.partial(FAMILIES[_f], kind=_k, C=int(_c[1:]))
ENV_ONLY = [n for n in ENV_NAMES if (n.split("-")[0], int(n.split("-")[1][1:])) not in SHAPES]


# ------------------------------------------------------------------------------------ running
def check_settings(expect):
    """bn_settings() must be the defaults overridden by `expect` and nothing else."""
    got, want = settings(), dict(DEFAULTS, **expect)
    assert got == want, f"bn_settings() {got}, expected {want}"
    return got


def run_case(name, dev):
    """Assert the case's geometry, run it; returns (figures, seconds). Raises on a mismatch."""
    t0 = time.perf_counter()
    kw = CASES[name].keywords
    geo = check_geometry(kw["kind"], kw["C"])
    fig = CASES[name](str(dev))
    if str(dev) != "cpu":
        torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    print(f"{name}: {dt:.2f} s, M {rows(kw['kind'], kw['C'])} {geo} " +
          ", ".join(f"{k} {v:.4g}" for k, v in fig.items()))
    return fig, dt


def run_child(expect, names, geometry_only=False):
    """Run `names` in a fresh process whose environment sets exactly `expect`'s variables, one JSON
    line per case; assert the settings it read and that every case passed. geometry_only: the
    child checks the settings and the cases' geometry and touches no GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ENV_OF.values()}
    env["PYTHONPATH"] = ROOT
    for k, v in expect.items():
        env[ENV_OF[k]] = str(v)
    r = subprocess.run([sys.executable, os.path.abspath(__file__),
                        json.dumps({"expect": expect, "cases": list(names),
                                    "geometry_only": geometry_only})],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-8000:])
    assert r.returncode == 0, f"child exit {r.returncode}: {r.stderr[-3000:]}"
    res = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    want = dict(DEFAULTS, **expect)
    assert [x["name"] for x in res] == list(names), "the child did not run every case"
    for x in res:
        assert x["settings"] == want, (x["name"], x["settings"], want)
    failed = [f"{x['name']}: {x['report']}" for x in res if not x["ok"]]
    assert not failed, "\n".join(failed)
    return res


def _main():
    job = json.loads(sys.argv[1])
    got = check_settings(job["expect"])
    for name in job["cases"]:
        out = {"name": name, "ok": True, "report": None, "settings": got}
        t0 = time.perf_counter()
        try:
            if job.get("geometry_only"):
                kw = CASES[name].keywords
                out["figures"] = check_geometry(kw["kind"], kw["C"])
            else:
                out["figures"], _ = run_case(name, torch.device("cuda", 0))
        except AssertionError as e:
            out["ok"], out["report"] = False, str(e)[:4000]
        out["seconds"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    _main()
