"""Float64 oracle of the gossip mix, numpy model of the fault injector's Gaussian, and the case
tables of ``test_gossip_fault_gpu.py`` / ``test_gossip_oracle_cpu.py`` (not collected: no
``test_`` prefix). The kernels are in ``csrc/kernels/gossip_fault.hip``.

``mix_oracle``   x <- (w0 + sum w_k) x + sum_k w_k c_k (nb_k - x), c_k = min(1, clip / ||nb_k - x||)
                 in float64 on the CPU; with clip > 0 a neighbour whose squared distance is not
                 finite has c_k = 0 and contributes exactly zero at every coordinate. (A finite
                 neighbour whose *fp32* sum overflows is dropped by the kernel and not by this
                 oracle: float64 does not overflow there.)
``gauss_model``  the kernel's ``gauss(seed, i)``: splitmix64 hash, two 24-bit uniforms, Box-Muller.
                 The integer part and the fp32 products are bit-exact; sqrt / log / cos are taken
                 in float64, so the kernel differs by the error of the device's fp32 functions.

The sizes below are written in terms of the kernel's launch constants; ``test_case_tables`` in
``test_gossip_oracle_cpu.py`` reads the constants from the kernel source and asserts the relations
each size stands for, so a changed constant shows up as a stale table.
"""
import functools
import math

import numpy as np
import torch

# ----------------------------------------------------------------------------- kernel constants
VEC = 8              # elements per vector access
BLK = 256            # kBlk: threads per workgroup
FOLD = 64            # lanes that fold the distance slab in the mix kernel
MAX_BLK = 1024       # kMaxBlk: most workgroups of the distance launch (slab columns)
FAULT_CAP = 2048     # most workgroups of the fault launch
MAX_NBRS = 8         # kMaxNbrs
WG = VEC * BLK       # elements one workgroup covers per trip (2048)

GUARD = 64
SENT = 77.0          # exact in bf16 and fp32
TOL = 1e-5           # rtol = atol of test_kernels_gpu.py::test_gossip_mix_k

# ----------------------------------------------------------------------------- case tables
DTYPES = ("bf16", "f32")
D_SLAB2 = (FOLD + 1) * WG + 7                 # 133127: 65 workgroups, the fold's second trip
D_STRIDE2 = MAX_BLK * WG + 50 * WG + 56 * VEC + 3   # 2200003: distance workgroups 0..50 take a
                                                    # second trip, the last one ragged; 3-tail
SMALL_DS = (1, VEC - 1, VEC, 2 * VEC - 1, WG - 1, WG, WG + 1)
SIZE_DS = SMALL_DS + (D_SLAB2, D_STRIDE2)
SIZE_KS = (1, 2, 8)
REST_KS = (3, 4, 5, 6, 7)                     # once each, at D = WG + 1 in bf16
SIZE_CASES = [(dt, k, D, clip) for dt in DTYPES for k in SIZE_KS for D in SIZE_DS
              for clip in ("off", "active")] + \
             [("bf16", k, WG + 1, clip) for k in REST_KS for clip in ("off", "active")]

# localised distance: the window distance workgroup b reads on trip j, as (b, j); "clipped":
# (50, 1) cut at D; "tail": the scalar tail alone
LOCAL_WINDOWS = ((0, 0), (FOLD - 1, 0), (FOLD, 0), (MAX_BLK - 1, 0), (0, 1), (44, 1), "clipped",
                 "tail")
LAST_TRIP2 = 50                               # last distance workgroup with a second trip


def local_window(win, D=D_STRIDE2):
    """[start, end) of a LOCAL_WINDOWS entry."""
    nv = D // VEC
    if win == "tail":
        return nv * VEC, D
    b, j = (LAST_TRIP2, 1) if win == "clipped" else win
    s = (b * BLK + j * MAX_BLK * BLK) * VEC
    return s, min(s + WG, D)


GRID_CAP_CASES = [(dt, k, D, cap) for dt in DTYPES for k in (1, 5) for D in (WG + 1, D_SLAB2)
                  for cap in (1, 3)]
ENGINE_DS = (WG + 1, 100003)
NONFINITE_DS = (VEC - 1, WG + 1)
NONFINITE_KINDS = ("nan_body", "nan_tail", "inf", "neg_inf", "overflow")

FAULT_DS = (1, BLK - 1, BLK, BLK + 1, 4096, FAULT_CAP * BLK + 5)
FAULT_BIG = FAULT_DS[-1]                      # 524293: a second trip and a ragged rest
GAUSS_SEEDS = (0, 1, 2 ** 40 + 7)
GAUSS_SIGMAS = (1.0, 3.0)


def tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def weights(k):
    """Distinct mixing weights (i + 1) / 2^m that sum to one with w0 > 0, every partial sum exact
    in fp32: k = 1: [1/2], 1/2; k = 2: [1/4, 1/2], 1/4; ... k = 8: [1/64 .. 8/64], 28/64."""
    den = 2
    while den <= k * (k + 1) // 2:
        den *= 2
    w = [(i + 1) / den for i in range(k)]
    return w, 1.0 - sum(w)


# ----------------------------------------------------------------------------- mix oracle
def mix_oracle(x, nbrs, w, w0, clip):
    """The mixed x in float64 (CPU)."""
    x = x.detach().cpu().double()
    out = (w0 + sum(w)) * x
    for nb, wk in zip(nbrs, w):
        d = nb.detach().cpu().double() - x
        if clip > 0:
            s = float((d * d).sum())
            if not math.isfinite(s):
                continue
            d = d * min(1.0, clip / max(math.sqrt(s), 1e-30))
        out = out + wk * d
    return out


def distances(x, nbrs):
    """||nb_k - x|| in float64."""
    x = x.detach().cpu().double()
    return [float((nb.detach().cpu().double() - x).norm()) for nb in nbrs]


def active_clip(x, nbrs):
    """Half the smallest non-zero finite distance: every c_k of such a neighbour is in (0, 0.5]."""
    ds = [d for d in distances(x, nbrs) if math.isfinite(d) and d > 0]
    return 0.5 * min(ds)


@functools.lru_cache(maxsize=4)
def mix_inputs(D, k, dtype_name, seed=0, x_bf16=False):
    """(x fp32, [nb_i]) on the CPU: N(0, 1), neighbour i scaled by 1 + i and rounded to the
    neighbour dtype. Shared between cases: treat as read-only."""
    gen = torch.Generator().manual_seed(1000 * seed + 10 * k + D % 7)
    x = torch.randn(D, generator=gen)
    if x_bf16:
        x = x.bfloat16().float()
    nbrs = [(torch.randn(D, generator=gen) * (1 + i)).to(tdt(dtype_name)) for i in range(k)]
    return x, nbrs


def make_bad(nb, kind):
    """A copy of neighbour ``nb`` made non-finite (or overflowing) as NONFINITE_KINDS says; returns
    (neighbour, coordinates that hold the bad values)."""
    nb = nb.clone()
    D = nb.numel()
    if kind == "nan_body":
        idx = [0]                    # first vector (the tail itself where D < VEC)
        nb[0] = math.nan
    elif kind == "nan_tail":
        idx = [D - 1]
        nb[D - 1] = math.nan
    elif kind in ("inf", "neg_inf"):
        idx = [D // 2]
        nb[D // 2] = math.inf if kind == "inf" else -math.inf
    else:
        assert kind == "overflow", kind
        idx = list(range(D))
        nb.fill_(3e38)               # finite in bf16 and fp32; its square is not
    return nb, idx


# ----------------------------------------------------------------------------- mix checker
def guarded(vals, D, dtype, dev, tail=GUARD):
    """Sentinel buffer with ``vals`` (or sentinels) at [GUARD, GUARD + D); returns (buffer, slice)."""
    buf = torch.full((GUARD + D + tail,), SENT, dtype=dtype)
    if vals is not None:
        buf[GUARD:GUARD + D] = vals
    buf = buf.to(dev)
    return buf, buf[GUARD:GUARD + D]


def run_mix(K, dev, x, nbrs, w, w0, clip, grid_cap=0, expect=None, bound=True, what=""):
    """Call ``K.gossip_mix_k`` on ``dev`` with a NaN-filled workspace and both parameter outputs,
    and assert: master against the oracle (``expect`` overrides it; ``False`` skips), parameter
    outputs equal to the rounded master bit for bit, a finite result, and with clipping and
    weights that sum to one ||x_new - x|| <= clip sum_k w_k (1 + 1e-5). Returns the new master
    (CPU)."""
    dtype = nbrs[0].dtype
    D = x.numel()
    master = x.to(dev).clone()
    p = torch.full((D,), SENT, dtype=dtype, device=dev)
    p2 = torch.full((D,), SENT, dtype=dtype, device=dev)
    kw = {}
    if dev.type == "cuda":
        from consensusml_amd.ops.native import lib
        kw["work"] = torch.full((lib().gossip_workspace_bytes(D) // 4,), math.nan,
                                dtype=torch.float32, device=dev)
    if grid_cap:
        kw["grid_cap"] = grid_cap
    K.gossip_mix_k(master, [nb.to(dev) for nb in nbrs], w, w0, clip, param_out=p, param_out2=p2,
                   **kw)
    got = master.cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: master not finite"
    if expect is not False:
        want = mix_oracle(x, nbrs, w, w0, clip) if expect is None else expect
        torch.testing.assert_close(got.double(), want, rtol=TOL, atol=TOL,
                                   msg=lambda m: f"{what}: master against the oracle: {m}")
    rounded = got.to(dtype)
    for name, out in (("param_out", p), ("param_out2", p2)):
        assert torch.equal(out.cpu().view(torch.uint8), rounded.view(torch.uint8)), \
            f"{what}: {name} is not the rounded master bit for bit"
    if bound and clip > 0:
        assert abs(w0 + sum(w) - 1.0) < 1e-12, "the norm bound needs weights that sum to one"
        moved = float((got.double() - x.double()).norm())
        limit = clip * sum(w) * (1 + 1e-5)
        print(f"{what}: ||x_new - x|| / (clip sum w) = {moved / (clip * sum(w)):.8f}")
        assert moved <= limit, f"{what}: moved {moved} > clip sum w = {limit}"
    return got


# ----------------------------------------------------------------------------- gaussian model
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix64(z):
    """splitmix64's finaliser on uint64 arrays (wraps around)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


@functools.lru_cache(maxsize=8)
def gauss_model(seed, n):
    """float64 array of gauss(seed, i), i < n. Shared between cases: treat as read-only."""
    i = np.arange(n, dtype=np.uint64)
    h = mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ mix64(i))
    two24 = np.float32(2.0 ** -24)
    u1 = ((h >> np.uint64(40)).astype(np.float32) + np.float32(1.0)) * two24
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * two24
    ang = np.float32(6.28318530718) * u2                       # fp32 product, as in the kernel
    assert u1.dtype == np.float32 and ang.dtype == np.float32
    v = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(ang.astype(np.float64))
    v.setflags(write=False)
    return v


def bf16_ulp(t):
    """Spacing of bf16 at the (bf16-representable, fp32) values of ``t``."""
    a = t.float().abs()
    _, e = torch.frexp(a)                                      # |t| = m 2^e, m in [0.5, 1)
    tiny = torch.full_like(a, 2.0 ** -133)                     # the subnormals' spacing
    ulp = torch.ldexp(torch.ones_like(a), e - 8)
    return torch.where(a == 0, tiny, torch.maximum(ulp, tiny))
