"""``csrc/kernels/gossip_fault.hip`` against the float64 oracle and the Gaussian model of
``gossip_oracle.py``: the k-neighbour mix with neighbour clipping across sizes that reach the
second trip of the distance launch and of the slab fold, both neighbour dtypes, both parameter
outputs, capped grids, the engine's sliced call shape, non-finite neighbours, argument checks;
and every kind of the fault injector, bit for bit where the operation is exact.

Every mix case goes through ``gossip_oracle.run_mix``: master against the oracle at the tolerance
of ``test_kernels_gpu.py::test_gossip_mix_k``, ``param_out`` / ``param_out2`` equal to the rounded
master bit for bit, ||x_new - x|| <= clip sum_k w_k (1 + 1e-5), and a finite result from a
workspace pre-filled with NaN (only slab entries the distance launch wrote are read; none without
clipping). Unless a case says otherwise ``clip`` is half the smallest ||nb_k - x||, so every c_k is
in (0, 0.5] and an error in any of them moves the result far beyond the tolerance.

Gaussian tolerance. A wrong bit in the hash or in a bit-slice changes values by O(1), so the
tolerance against the model only covers the device's logf / cosf / sqrtf and the final fp32
product: the largest |kernel - sigma * model| measured on an MI355X over all fp32 cases of
``test_fault_gaussian`` was GAUSS_MEASURED * sigma; the test asserts
max(4 * GAUSS_MEASURED, 1e-6) * sigma, which has to stay below 1e-4 * sigma.
"""
import math

import pytest
import torch

import gossip_oracle as GO
from consensusml_amd.ops import kernels as K
from consensusml_amd.ops.native import lib

pytestmark = pytest.mark.gpu

GAUSS_MEASURED = 6.456e-7        # (D = 524293, seed 1; 5.1e-7 .. 6.5e-7 over the large cases)
GAUSS_ATOL = max(4 * GAUSS_MEASURED, 1e-6)     # 2.6e-6
assert GAUSS_ATOL <= 1e-4


def _clip(mode, x, nbrs):
    return 0.0 if mode == "off" else GO.active_clip(x, nbrs)


# ----------------------------------------------------------------------------- mix: sizes
@pytest.mark.parametrize("dt,k,D,mode", GO.SIZE_CASES,
                         ids=[f"{dt}-k{k}-D{D}-{m}" for dt, k, D, m in GO.SIZE_CASES])
def test_mix_sizes(cuda, dt, k, D, mode):
    x, nbrs = GO.mix_inputs(D, k, dt)
    w, w0 = GO.weights(k)
    GO.run_mix(K, cuda, x, nbrs, w, w0, _clip(mode, x, nbrs), what=f"{dt}-k{k}-D{D}-{mode}")


@pytest.mark.parametrize("dt", GO.DTYPES)
@pytest.mark.parametrize("D", [GO.WG + 1, GO.D_SLAB2])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_mix_clip_not_binding(cuda, dt, D, k):
    """clip = twice the largest distance: every c_k is exactly 1, the clip = 0 result bit for bit."""
    x, nbrs = GO.mix_inputs(D, k, dt)
    w, w0 = GO.weights(k)
    clip = 2.0 * max(GO.distances(x, nbrs))
    a = GO.run_mix(K, cuda, x, nbrs, w, w0, clip, bound=False, what="loose")
    b = GO.run_mix(K, cuda, x, nbrs, w, w0, 0.0, what="off")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dt", GO.DTYPES)
@pytest.mark.parametrize("D", [GO.VEC - 1, GO.WG + 1])
def test_mix_zero_distance_neighbour(cuda, dt, D):
    """A neighbour equal to x (distance 0, c = min(1, clip / 1e-30) = 1): finite, and its weight
    stays with x."""
    x, nbrs = GO.mix_inputs(D, 3, dt, x_bf16=True)
    nbrs = [nbrs[0], x.to(GO.tdt(dt)), nbrs[2]]
    assert torch.equal(nbrs[1].float(), x)
    w, w0 = GO.weights(3)
    clip = GO.active_clip(x, nbrs)
    want = GO.mix_oracle(x, [nbrs[0], nbrs[2]], [w[0], w[2]], w0 + w[1], clip)
    GO.run_mix(K, cuda, x, nbrs, w, w0, clip, expect=want, what=f"zero-{dt}-D{D}")
    GO.run_mix(K, cuda, x, nbrs, w, w0, clip, what=f"zero-{dt}-D{D} (oracle with all three)")


@pytest.mark.parametrize("win", GO.LOCAL_WINDOWS, ids=lambda w: str(w).replace(" ", ""))
def test_mix_localised_distance(cuda, win):
    """Neighbour 0 differs from x in the elements one distance workgroup reads on one trip only:
    clip = half that window's norm, so a dropped partial gives c_0 = 1 for 0.5 and a
    double-counted one about 0.35."""
    D = GO.D_STRIDE2
    x, nbrs = GO.mix_inputs(D, 2, "bf16", x_bf16=True)
    s, e = GO.local_window(win)
    nb0 = x.clone()
    nb0[s:e] += 1.0
    nbrs = [nb0.bfloat16(), nbrs[1]]
    d0, d1 = GO.distances(x, nbrs)
    assert 0.9 * math.sqrt(e - s) < d0 < 1.1 * math.sqrt(e - s) and d1 > 10 * d0
    w, w0 = GO.weights(2)
    GO.run_mix(K, cuda, x, nbrs, w, w0, 0.5 * d0, what=f"local-{win}")


@pytest.mark.parametrize("k", GO.REST_KS + (1, 2, 8))
def test_mix_k2_ring_entry_and_order(cuda, k):
    """The neighbours' order matters (weight i pairs with neighbour i), and for k = 2 the ring
    entry point gives the same bits."""
    x, nbrs = GO.mix_inputs(GO.WG + 1, k, "bf16")
    w, w0 = GO.weights(k)
    clip = GO.active_clip(x, nbrs)
    a = GO.run_mix(K, cuda, x, nbrs, w, w0, clip, what=f"order-k{k}")
    if k > 1:
        b = GO.run_mix(K, cuda, x, nbrs[::-1], w, w0, clip, what=f"order-k{k}-reversed")
        assert not torch.equal(a, b)
    if k == 2:
        for c in (0.0, clip):
            m1, m2 = x.to(cuda).clone(), x.to(cuda).clone()
            p = torch.empty(x.numel(), dtype=torch.bfloat16, device=cuda)
            K.gossip_mix_k(m1, [n.to(cuda) for n in nbrs], w, w0, c)
            K.gossip_mix(m2, nbrs[0].to(cuda), nbrs[1].to(cuda), w0, w[0], w[1], c, param_out=p)
            assert torch.equal(m1.view(torch.int32), m2.view(torch.int32))
            assert torch.equal(p, m2.bfloat16())


# ----------------------------------------------------------------------------- mix: grid cap
@pytest.mark.parametrize("dt,k,D,cap", GO.GRID_CAP_CASES,
                         ids=[f"{dt}-k{k}-D{D}-cap{c}" for dt, k, D, c in GO.GRID_CAP_CASES])
def test_mix_grid_cap(cuda, dt, k, D, cap):
    x, nbrs = GO.mix_inputs(D, k, dt)
    w, w0 = GO.weights(k)
    GO.run_mix(K, cuda, x, nbrs, w, w0, GO.active_clip(x, nbrs), grid_cap=cap,
               what=f"cap{cap}-{dt}-k{k}-D{D}")
    # the per-element arithmetic does not depend on the grid
    a = GO.run_mix(K, cuda, x, nbrs, w, w0, 0.0, grid_cap=cap, what="capped, no clip")
    b = GO.run_mix(K, cuda, x, nbrs, w, w0, 0.0, what="default grid, no clip")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_mix_grid_cap_range(cuda):
    x, nbrs = GO.mix_inputs(GO.WG + 1, 1, "bf16")
    m = x.to(cuda).clone()
    for cap in (-1, (1 << 20) + 1):
        with pytest.raises(RuntimeError, match="grid_cap"):
            K.gossip_mix_k(m, [nbrs[0].to(cuda)], [0.5], 0.5, 1.0, grid_cap=cap)
    assert torch.equal(m.cpu(), x)


# ----------------------------------------------------------------------------- mix: engine shape
@pytest.mark.parametrize("dt", GO.DTYPES)
@pytest.mark.parametrize("D", GO.ENGINE_DS)
def test_mix_engine_call_shape(cuda, dt, D):
    """Slices of larger buffers (as ``master[s:e]`` / ``flat_param[s:e]``) and neighbour buffers
    longer than D: nothing past D enters the distance, nothing outside the slices is written."""
    dtype = GO.tdt(dt)
    x, nbrs = GO.mix_inputs(D, 2, dt)
    w, w0 = GO.weights(2)
    clip = GO.active_clip(x, nbrs)
    mb, master = GO.guarded(x, D, torch.float32, cuda)
    pb, p = GO.guarded(None, D, dtype, cuda)
    p2b, p2 = GO.guarded(None, D, dtype, cuda)
    long = []
    for i, nb in enumerate(nbrs):
        t = torch.empty(D + GO.GUARD, dtype=dtype)
        t[:D] = nb
        t[D:] = (1e30, math.nan)[i]
        long.append(t.to(cuda))
    work = torch.full((lib().gossip_workspace_bytes(D) // 4,), math.nan, device=cuda)
    K.gossip_mix_k(master, long, w, w0, clip, param_out=p, work=work, param_out2=p2)
    got = master.cpu()
    torch.testing.assert_close(got.double(), GO.mix_oracle(x, nbrs, w, w0, clip), rtol=GO.TOL,
                               atol=GO.TOL)
    assert torch.equal(p.cpu(), got.to(dtype)) and torch.equal(p2.cpu(), got.to(dtype))
    for name, buf in (("master", mb), ("param_out", pb), ("param_out2", p2b)):
        assert bool((buf[:GO.GUARD] == GO.SENT).all()), f"wrote before {name}"
        assert bool((buf[GO.GUARD + D:] == GO.SENT).all()), f"wrote after {name}"
    for i, (t, nb) in enumerate(zip(long, nbrs)):
        assert torch.equal(t[:D].cpu().view(torch.uint8), nb.view(torch.uint8)), f"neighbour {i}"


# ----------------------------------------------------------------------------- mix: non-finite
@pytest.mark.parametrize("kind", GO.NONFINITE_KINDS)
@pytest.mark.parametrize("dt", GO.DTYPES)
@pytest.mark.parametrize("D", GO.NONFINITE_DS)
def test_mix_nonfinite_neighbour(cuda, D, dt, kind):
    """With clipping a neighbour at a non-finite distance is dropped: exactly zero at every
    coordinate, its weight stays with x. Without clipping there is no protection."""
    x, nbrs = GO.mix_inputs(D, 3, dt)
    nbrs = list(nbrs)
    nbrs[1], idx = GO.make_bad(nbrs[1], kind)
    w, w0 = GO.weights(3)
    good = [nbrs[0], nbrs[2]]
    clip = GO.active_clip(x, good)
    want = GO.mix_oracle(x, good, [w[0], w[2]], w0 + w[1], clip)
    what = f"{kind}-{dt}-D{D}"
    if kind == "overflow":
        # the float64 oracle over all three does not overflow and legitimately moves by w_1 clip,
        # so it is no reference here: the norm bound (asserted by run_mix) holds either way
        got = GO.run_mix(K, cuda, x, nbrs, w, w0, clip, expect=False, what=what)
        # the kernel's fp32 squares are inf, so by its rule the neighbour is dropped
        torch.testing.assert_close(got.double(), want, rtol=GO.TOL, atol=GO.TOL)
    else:
        GO.run_mix(K, cuda, x, nbrs, w, w0, clip, expect=want, what=what)
    # the ring entry point shares the rule
    m = x.to(cuda).clone()
    K.gossip_mix(m, nbrs[1].to(cuda), nbrs[2].to(cuda), w0 + w[0], w[1], w[2], clip)
    ring = GO.mix_oracle(x, [nbrs[2]], [w[2]], w0 + w[0] + w[1], clip)
    torch.testing.assert_close(m.cpu().double(), ring, rtol=GO.TOL, atol=GO.TOL)
    # clip = 0: the documented behaviour is that the bad values come through
    m = x.to(cuda).clone()
    K.gossip_mix_k(m, [n.to(cuda) for n in nbrs], w, w0, 0.0)
    raw = m.cpu()
    if kind.startswith("nan"):
        assert bool(torch.isnan(raw[idx]).all())
    elif kind != "overflow":
        assert not bool(torch.isfinite(raw[idx]).any())     # w (inf - x) is inf, not NaN
    if kind != "overflow":
        keep = torch.ones(D, dtype=torch.bool)
        keep[idx] = False
        clean = [nbrs[0], torch.where(keep, nbrs[1], torch.zeros_like(nbrs[1])), nbrs[2]]
        torch.testing.assert_close(raw[keep].double(), GO.mix_oracle(x, clean, w, w0, 0.0)[keep],
                                   rtol=GO.TOL, atol=GO.TOL)


def test_mix_nonfinite_master_drops_every_neighbour(cuda):
    D = GO.WG + 1
    x, nbrs = GO.mix_inputs(D, 3, "bf16")
    x = x.clone()
    x[D - 1] = math.inf
    w, w0 = GO.weights(3)
    m = x.to(cuda).clone()
    p = torch.empty(D, dtype=torch.bfloat16, device=cuda)
    K.gossip_mix_k(m, [n.to(cuda) for n in nbrs], w, w0, 1.0, param_out=p)
    assert torch.equal(m.cpu(), x)                 # (w0 + sum w) = 1 exactly
    assert torch.equal(p.cpu(), x.bfloat16())


# ----------------------------------------------------------------------------- mix: arguments
def test_mix_argument_checks(cuda):
    D = GO.WG + 1
    x, nbrs = GO.mix_inputs(D, 8, "bf16")
    nb = [n.to(cuda) for n in nbrs]
    w, w0 = GO.weights(8)
    m = x.to(cuda).clone()
    pad = torch.empty(D + 8, device=cuda)
    pad[1:D + 1] = m
    bad_calls = {
        "k = 0": lambda: K.gossip_mix_k(m, [], [], w0, 1.0),
        "k = 9": lambda: K.gossip_mix_k(m, nb + nb[:1], w + w[:1], w0, 1.0),
        "len(w) != k": lambda: K.gossip_mix_k(m, nb[:3], w[:2], w0, 1.0),
        "short neighbour": lambda: K.gossip_mix_k(m, [nb[0], nb[1][:D - 1]], w[:2], w0, 1.0),
        "mixed dtypes": lambda: K.gossip_mix_k(m, [nb[0], nb[1].float()], w[:2], w0, 1.0),
        "param_out dtype": lambda: K.gossip_mix_k(m, nb[:2], w[:2], w0, 1.0,
                                                  param_out=torch.empty(D, device=cuda)),
        "param_out2 dtype": lambda: K.gossip_mix_k(m, nb[:2], w[:2], w0, 1.0,
                                                   param_out2=torch.empty(D, device=cuda)),
        "short param_out": lambda: K.gossip_mix_k(
            m, nb[:2], w[:2], w0, 1.0,
            param_out=torch.empty(D - 1, dtype=torch.bfloat16, device=cuda)),
        "small workspace": lambda: K.gossip_mix_k(m, nb[:2], w[:2], w0, 1.0,
                                                  work=torch.empty(16, device=cuda)),
        "fp64 workspace": lambda: K.gossip_mix_k(
            m, nb[:2], w[:2], w0, 1.0,
            work=torch.empty(8 * 1024, dtype=torch.float64, device=cuda)),
        "bf16 master": lambda: K.gossip_mix_k(m.bfloat16(), nb[:2], w[:2], w0, 1.0),
    }
    for name, call in bad_calls.items():
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            call()
            pytest.fail(f"{name}: accepted")
        assert torch.equal(m.cpu(), x), f"{name}: master changed"
    # a master slice off the 16-byte grid
    mis = pad[1:D + 1]
    with pytest.raises(RuntimeError):
        K.gossip_mix_k(mis, nb[:2], w[:2], w0, 1.0)
    with pytest.raises(RuntimeError):
        K.gossip_mix(mis, nb[0], nb[1], w0, w[0], w[1], 1.0)
    torch.cuda.synchronize()
    assert torch.equal(mis.cpu(), x)


# ----------------------------------------------------------------------------- fault injector
def _fault_buf(vals, D, dtype, dev):
    buf = torch.full((D + GO.GUARD,), GO.SENT, dtype=dtype)
    buf[:D] = vals
    buf = buf.to(dev)
    return buf, buf[:D]


def _sentinel_ok(buf, D):
    return bool((buf[D:] == GO.SENT).all())


def _gauss(cuda, dtype, D, seed, sigma):
    buf, g = _fault_buf(1.0, D, dtype, cuda)
    K.inject_fault(g, "gaussian", sigma=sigma, seed=seed)
    assert _sentinel_ok(buf, D), "gaussian wrote past D"
    return g.cpu()


@pytest.mark.parametrize("sigma", GO.GAUSS_SIGMAS)
@pytest.mark.parametrize("seed", GO.GAUSS_SEEDS)
@pytest.mark.parametrize("D", GO.FAULT_DS)
@pytest.mark.parametrize("dt", GO.DTYPES)
def test_fault_gaussian(cuda, dt, D, seed, sigma):
    dtype = GO.tdt(dt)
    got = _gauss(cuda, dtype, D, seed, sigma)
    model = torch.from_numpy(sigma * GO.gauss_model(seed, D))
    if dt == "f32":
        err = (got.double() - model).abs().max().item()
        print(f"gaussian f32 D={D} seed={seed} sigma={sigma}: max |kernel - model| / sigma = "
              f"{err / sigma:.3e}")
        assert err <= GAUSS_ATOL * sigma
    else:
        ref = model.float().bfloat16().float()
        ulps = ((got.float() - ref).abs() / GO.bf16_ulp(ref)).max().item()
        print(f"gaussian bf16 D={D} seed={seed} sigma={sigma}: max distance {ulps:.3f} bf16 ulp")
        assert ulps <= 1.0
    # same seed, same bits; another seed, other values
    again = _gauss(cuda, dtype, D, seed, sigma)
    assert torch.equal(got.view(torch.uint8), again.view(torch.uint8))
    other = _gauss(cuda, dtype, D, seed + 1, sigma)
    assert not torch.equal(got, other)
    if D >= 256:
        assert (got != other).float().mean().item() > 0.9


@pytest.mark.parametrize("dt", GO.DTYPES)
@pytest.mark.parametrize("sigma", GO.GAUSS_SIGMAS)
def test_fault_gaussian_grid_independent_and_moments(cuda, dt, sigma):
    """A value depends on (seed, i) only, not on the launch grid; the moments are the model's."""
    dtype = GO.tdt(dt)
    big = _gauss(cuda, dtype, GO.FAULT_BIG, 1, sigma)
    small = _gauss(cuda, dtype, 4096, 1, sigma)
    assert torch.equal(big[:4096].view(torch.uint8), small.view(torch.uint8))
    v = big.double()
    assert bool(torch.isfinite(v).all())
    mean, std = v.mean().item(), v.std().item()
    print(f"gaussian {dt} sigma={sigma}: mean / sigma = {mean / sigma:.5f}, std / sigma = "
          f"{std / sigma:.5f}")
    assert abs(mean) < 0.01 * sigma
    assert abs(std / sigma - 1.0) < 0.01


def _fault_input(D, dtype):
    gen = torch.Generator().manual_seed(D)
    g = torch.randn(D, generator=gen).to(dtype)
    special = torch.tensor([-0.0, 0.0, math.inf, -math.inf, math.nan, 2.0 ** -130]).to(dtype)
    n = min(D, special.numel())
    g[D - n:] = special[:n]
    return g


@pytest.mark.parametrize("D", GO.FAULT_DS)
@pytest.mark.parametrize("dt", GO.DTYPES)
def test_fault_exact_kinds(cuda, dt, D):
    """sign_flip / scaled / zero / nan against torch (multiply in fp32, then round), bit for bit;
    none leaves every bit alone, -0.0, NaN and Inf included."""
    dtype = GO.tdt(dt)
    g0 = _fault_input(D, dtype)
    bits = lambda t: t.cpu().contiguous().view(torch.uint8)     # noqa: E731

    def same(got, want, what):
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions"
        assert torch.equal(bits(got[~nan]), bits(want[~nan])), what

    for scale in (2.0, 10.0):
        for kind, factor in (("sign_flip", -scale), ("scaled", scale)):
            buf, g = _fault_buf(g0, D, dtype, cuda)
            K.inject_fault(g, kind, scale=scale)
            same(g.cpu(), (g0.float() * factor).to(dtype), f"{kind} x{scale}")
            assert _sentinel_ok(buf, D), f"{kind} wrote past D"
    buf, g = _fault_buf(g0, D, dtype, cuda)
    K.inject_fault(g, "zero")
    assert torch.equal(bits(g), bits(torch.zeros(D, dtype=dtype))) and _sentinel_ok(buf, D)
    buf, g = _fault_buf(g0, D, dtype, cuda)
    K.inject_fault(g, "nan")
    assert bool(torch.isnan(g).all()) and _sentinel_ok(buf, D)
    for call in (lambda t: K.inject_fault(t, "none"), lambda t: lib().fault(t, 0, 10.0, 1.0, 0)):
        buf, g = _fault_buf(g0, D, dtype, cuda)
        call(g)
        assert torch.equal(bits(g), bits(g0)), "none changed bits"
        assert _sentinel_ok(buf, D)
