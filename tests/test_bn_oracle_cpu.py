"""The BatchNorm oracle (tests/bn_oracle.py) checked without a GPU: its exact tier really is
independent of summation order and exact in fp32, its fp64-tier formulas agree with torch.autograd
through F.batch_norm, and the stated conditions on the inputs hold for the fixed seeds."""
import pytest
import torch
import torch.nn.functional as F

import bn_oracle as bo

SMALL = [(k, C) for k, C in bo.SHAPES if k[0] == "S"]
LARGE = [(k, C) for k, C in bo.SHAPES if k[0] == "G"]
_id = "{0[0]}-C{0[1]}".format


def _ordered_sum32(t, order):
    """fp32 sum of the rows of t [M, K] one row at a time in `order`."""
    acc = torch.zeros(t.shape[1], dtype=torch.float32)
    for r in order:
        acc += t[r]
    return acc


@pytest.mark.parametrize("shape", SMALL, ids=_id)
def test_exact_tier_is_order_independent(shape):
    kind, C = shape
    M = bo.rows(kind, C)
    d = bo._data(kind, C, False, "cpu")
    xf = d["x"].float()
    dsh = xf - xf[0]                                     # fp32, as the kernel forms it
    cols = [dsh, dsh * dsh]
    want = list(bo.shifted_sums(d["x"])[:2])
    xh = bo.xhat(d["x"], d)
    xh32 = (xf - d["mean"]) * d["invstd"]
    assert torch.equal(xh32.double(), xh)
    for relu, use_mask, use_dy2 in ((True, False, False), (True, True, True), (False, False, True)):
        _, dz, _, sums = bo._bwd_oracle(d, relu, use_mask, use_dy2)
        dz32 = dz.float()
        assert torch.equal(dz32.double(), dz)
        prod = dz32 * xh32
        assert torch.equal(prod.double(), dz * xh)
        cols += [dz32, prod]
        want += [sums["sdz"], sums["sdzx"]]
        assert torch.equal(sums["sdz32"].double(), sums["sdz"])
        assert torch.equal(sums["sdzx32"].double(), sums["sdzx"])
    t = torch.cat(cols, 1)
    want = torch.cat([w.double() for w in want])
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(M + C)).tolist()
    s64 = t.double().sum(0)
    assert torch.equal(s64, want)
    for order in (range(M), range(M - 1, -1, -1), perm):
        assert torch.equal(_ordered_sum32(t, order).double(), s64)


@pytest.mark.parametrize("shape", SMALL, ids=_id)
def test_eval_forward_is_exact_in_fp32(shape):
    """eval_fwd / eval_fwd2 assert every intermediate equal to its fp32 rounding and the share of
    exact zeros; here the same expressions in fp32 arithmetic must give the same z."""
    kind, C = shape
    d = bo._data(kind, C, False, "cpu")
    sc = d["invstd"] * d["gamma"].float()
    bi = d["beta"].float() - d["mean"] * sc
    sc2 = d["invstd2"] * d["gamma2"].float()
    bi2 = d["beta2"].float() - d["mean2"] * sc2
    for _, relu, use_res, _ in bo.EVAL_MODES:
        res = d["res"] if use_res else None
        y, mask, z, share = bo.eval_fwd(d["x"], res, d, relu)
        z32 = d["x"].float() * sc + bi
        if use_res:
            z32 = z32 + d["res"].float()
        assert torch.equal(z32.double(), z) and share >= 0.01
        assert torch.equal(bo.unpack_mask(mask), z > 0)
        assert torch.equal(y.double(), (z.clamp_min(0) if relu else z).float().bfloat16().double())
    y, mask, z, share = bo.eval_fwd2(d["x"], d["x2"], d)
    z32 = d["x"].float() * sc + (d["x2"].float() * sc2 + (bi + bi2))
    assert torch.equal(z32.double(), z) and share >= 0.01
    assert bool(((z == 0) & bo.unpack_mask(mask)).sum() == 0)     # z == 0 -> bit clear


def test_mask_packing_round_trip():
    g = torch.Generator().manual_seed(5)
    pos = torch.rand(37, 64, generator=g) < 0.5
    m = bo.pack_mask(pos)
    assert m.shape == (37, 8) and m.dtype == torch.uint8
    assert torch.equal(bo.unpack_mask(m), pos)
    assert int(m[3, 2]) == sum(int(pos[3, 16 + k]) << k for k in range(8))


def test_ulp_diff():
    a = torch.tensor([1.0, -1.0, 0.0, 3.5], dtype=torch.float32)
    b = torch.nextafter(a, torch.tensor([2.0, -2.0, -1.0, 3.5]))
    assert bo.ulp_diff(a, b).tolist() == [1, 1, 1, 0]


def _autograd_bn(x, gamma, beta, rm, rv, eps, mom):
    return F.batch_norm(x, rm, rv, gamma, beta, True, mom, eps)


def test_fp64_formulas_agree_with_autograd():
    """Independence: train_stats, train_fwd_ref, bwd_sums and dx_ref against autograd in fp64."""
    kind, C = "S4", 64
    M = bo.rows(kind, C)
    d = bo._data(kind, C, True, "cpu")
    eps, mom = bo.f32(bo.EPS), bo.f32(bo.MOMENTUM)
    st = bo.train_stats(d["x"], d["rmean"], d["rvar"])
    assert float(st["var"].min()) > 1.0                       # non-degenerate
    for relu, use_res in ((False, False), (True, False), (True, True), (False, True)):
        x = d["x"].double().requires_grad_(True)
        res = d["res"].double().requires_grad_(True) if use_res else None
        gamma = d["gamma"].double().requires_grad_(True)
        beta = d["beta"].double().requires_grad_(True)
        rm, rv = d["rmean"].double(), d["rvar"].double()
        z = _autograd_bn(x, gamma, beta, rm, rv, eps, mom)
        if use_res:
            z = z + res
        y = F.relu(z) if relu else z
        dy = d["dy"].double() + d["dy2"].double()
        y.backward(dy)
        # statistics: the oracle's are fp32 roundings of the same numbers
        mean64 = x.detach().mean(0)
        inv64 = 1.0 / torch.sqrt(x.detach().var(0, unbiased=False) + eps)
        for got, want in ((st["mean"], mean64), (st["invstd"], inv64), (st["rmean"], rm),
                          (st["rvar"], rv)):
            assert bool(((got.double() - want).abs() <= 2.0 ** -24 * want.abs() + 1e-12).all())
        zr, _ = bo.train_fwd_ref(d["x"], d["res"] if use_res else None, d, mean64, inv64, relu)
        torch.testing.assert_close(zr, z.detach(), rtol=0, atol=1e-10)
        keep = (z.detach() > 0) if relu else None
        dz = bo.masked_dz(d["dy"], d["dy2"], keep)
        xh = (d["x"].double() - mean64) * inv64
        sdz, sdzx = dz.sum(0), (dz * xh).sum(0)
        ref, _ = bo.dx_ref(dz, xh, inv64 * d["gamma"].double(), sdz, sdzx)
        torch.testing.assert_close(ref, x.grad, rtol=0, atol=1e-10)
        torch.testing.assert_close(sdzx, gamma.grad, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(sdz, beta.grad, rtol=1e-10, atol=1e-10)
        if use_res:
            torch.testing.assert_close(dz, res.grad, rtol=0, atol=1e-10)


def test_fp64_dual_bn_formulas_agree_with_autograd():
    kind, C = "S4", 64
    d = bo._data(kind, C, True, "cpu")
    eps = bo.f32(bo.EPS)
    x1 = d["x"].double().requires_grad_(True)
    x2 = d["x2"].double().requires_grad_(True)
    g1, b1 = d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    g2, b2 = d["gamma2"].double().requires_grad_(True), d["beta2"].double().requires_grad_(True)
    z = _autograd_bn(x1, g1, b1, None, None, eps, 0.1) + _autograd_bn(x2, g2, b2, None, None, eps, 0.1)
    F.relu(z).backward(d["dy"].double())
    st = []
    for x in (x1, x2):
        st.append({"mean": x.detach().mean(0),
                   "invstd": 1.0 / torch.sqrt(x.detach().var(0, unbiased=False) + eps)})
    zr, _ = bo.train_fwd2_ref(d["x"], d["x2"], d, st[0], st[1])
    torch.testing.assert_close(zr, z.detach(), rtol=0, atol=1e-10)
    dz = bo.masked_dz(d["dy"], None, z.detach() > 0)
    for x, s, g, gr, br in ((x1, st[0], g1, g1.grad, b1.grad), (x2, st[1], g2, g2.grad, b2.grad)):
        xh = (x.detach() - s["mean"]) * s["invstd"]
        sdz, sdzx = dz.sum(0), (dz * xh).sum(0)
        ref, _ = bo.dx_ref(dz, xh, s["invstd"] * g.detach(), sdz, sdzx)
        torch.testing.assert_close(ref, x.grad, rtol=0, atol=1e-10)
        torch.testing.assert_close(sdzx, gr, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(sdz, br, rtol=1e-10, atol=1e-10)


def _left_out_shares(kind, C):
    d = bo._data(kind, C, True, "cpu")
    st = bo.train_stats(d["x"], d["rmean"], d["rvar"])        # asserts var == the direct variance
    st2 = bo.train_stats(d["x2"], d["rmean2"], d["rvar2"])
    shares = []
    for res in (None, d["res"]):
        z, S = bo.train_fwd_ref(d["x"], res, d, st["mean"], st["invstd"], True)
        shares.append(bo.left_out(z, S)[1])                   # asserts <= 0.1 %
    z, S = bo.train_fwd2_ref(d["x"], d["x2"], d, st, st2)
    shares.append(bo.left_out(z, S)[1])
    return shares


@pytest.mark.parametrize("shape", SMALL + LARGE, ids=_id)
def test_left_out_share_of_mask_bits(shape):
    shares = _left_out_shares(*shape)
    print(shape, "left out", shares)
    assert max(shares) <= 0.001


@pytest.mark.parametrize("C", bo.ALL_C)
def test_single_row(C):
    """M = 1: var = 0, invstd = 1 / sqrt(eps), the running variance takes var itself."""
    d = bo._data("S1", C, True, "cpu")
    st = bo.train_stats(d["x"], d["rmean"], d["rvar"])
    eps, mom = bo.f32(bo.EPS), bo.f32(bo.MOMENTUM)
    assert torch.equal(st["var"], torch.zeros(C, dtype=torch.float64))
    assert torch.equal(st["mean"], d["x"][0].float())
    assert torch.equal(st["invstd"], torch.full((C,), 1.0 / eps ** 0.5, dtype=torch.float64).float())
    assert torch.equal(st["rvar"], ((1.0 - mom) * d["rvar"].double()).float())
    assert bool(torch.isfinite(st["rmean"]).all())


def test_input_ranges():
    d = bo._data("S4", 16, False, "cpu")
    for k in ("x", "x2", "res", "dy", "dy2"):
        v = d[k].double()
        assert torch.equal(v, v.round()) and float(v.abs().max()) <= 4
    for train in (False, True):
        p = bo.make_params(256, 7, train)
        for sfx in ("", "2"):
            assert set(p["gamma" + sfx].tolist()) <= set(bo.GAMMAS)
            assert min(p["gamma" + sfx].tolist()) < 0 < max(p["gamma" + sfx].tolist())
            assert set(p["invstd" + sfx].tolist()) <= set(bo.INVSTDS)
            b = p["beta" + sfx].double() * 4
            assert torch.equal(b, b.round()) and float(b.abs().max()) <= 8
            m = p["mean" + sfx].double()
            assert torch.equal(m, m.round()) and float(m.abs().max()) <= 2


def test_case_geometry_in_the_default_settings():
    """Every case lands in the branch it names (bn_geometry evaluates predicates only: no GPU)."""
    assert bo.check_settings({}) == bo.DEFAULTS
    for name, fn in bo.CASES.items():
        bo.check_geometry(fn.keywords["kind"], fn.keywords["C"])
    # 19389 R + 1 rows would fall short of the workgroup cap
    assert int(bo._lib().bn_geometry(19389 * 32 + 1, 64)[0]) < 1024


@pytest.mark.parametrize("expect", [{"bn_nt": 1}, {"bn_grid_cap": 3}, {"bn_grid_cap": 0}],
                         ids=["nt1", "cap3", "cap0"])
def test_case_geometry_under_the_switches(expect):
    """The switch cases of test_bn_exact_env_gpu.py: a fresh process reads the setting, and every
    case lands in its branch under it."""
    res = bo.run_child(expect, bo.ENV_NAMES, geometry_only=True)
    grids = {x["name"]: x["figures"]["grid"] for x in res}
    if expect.get("bn_grid_cap") == 3:
        assert set(grids.values()) == {3}
    if expect.get("bn_grid_cap") == 0:
        assert grids["G1-C8-eval"] == 2049
