"""tests/wgrad_oracle.py without a GPU: the reference against the fp64 library weight gradient
(stride 1 and 2 with padding 1, the single tap, each prologue formula), the input condition of
every bf16-output case, the routes of every case table (wgrad_route and wgrad_settings only
evaluate host predicates), and the mismatch report on three planted errors -- with the relative
Frobenius norm each of them has, which is what the norm tests of these kernels look at."""
import pytest
import torch

import wgrad_oracle as wo


def _lib_dw(dy, x, k, stride, padding):
    """torch.nn.grad.conv2d_weight in fp64 as [Co, taps, Ci]; dy [N, Ho, Wo, Co], x [N, H, W, Ci]"""
    Co, Ci = dy.shape[3], x.shape[3]
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Co, Ci, k, k),
                                      dy.double().permute(0, 3, 1, 2), stride=stride, padding=padding)
    return ref.permute(0, 2, 3, 1).reshape(Co, k * k, Ci)


@pytest.mark.parametrize("N,H,W,taps,stride", [(2, 5, 7, 9, 1), (3, 1, 6, 9, 1), (2, 8, 6, 9, 2),
                                               (2, 4, 10, 1, 2), (2, 3, 5, 1, 1)])
def test_sums_equal_fp64_conv2d_weight(N, H, W, taps, stride):
    """On integers the library's fp64 weight gradient is exact as well, whatever its order."""
    dy = wo.ints((N, H // stride, W // stride, 16), 2, 3)
    x = wo.ints((N, H, W, 8), 1, 4)
    s = wo.Taps(dy, x, taps, stride).sums()
    k = 3 if taps == 9 else 1
    assert torch.equal(s, _lib_dw(dy, x, k, stride, k // 2)) and s.abs().max() > 0
    a = wo.Taps(dy, x, taps, stride).sums(absolute=True)
    assert torch.equal(a, _lib_dw(dy.abs(), x.abs(), k, stride, k // 2))


@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("dmode", [wo.DP_NONE, wo.DP_FULL, wo.DP_MASK, wo.DP_BNRELU])
def test_prologue_formulas(pro, dmode):
    """The staged operands written out independently in fp64 (exact on the dyadic parameters) and
    their library weight gradient; the planted ReLU zeros are there."""
    P, Co, Ci = 70, 16, 24
    o = wo.ref_1x1(P, Co, Ci, pro, dmode, True)
    g, z, x = o["dy"].double(), o["z"].double(), o["x"].double()
    m = torch.tensor([[(int(o["mask"][p, c // 8]) >> (c % 8)) & 1 for c in range(Co)]
                      for p in range(P)], dtype=torch.float64)
    da, db, dc = o["da"].double(), o["db"].double(), o["dc"].double()
    D = {wo.DP_NONE: g, wo.DP_FULL: da * (m * g) + db * z + dc, wo.DP_MASK: da * (m * g) + dc,
         wo.DP_BNRELU: torch.relu(g * da + db)}[dmode]
    X = torch.relu(x * o["sc"].double() + o["bi"].double()) if pro else x
    ref = _lib_dw(D.view(P, 1, 1, Co), X.view(P, 1, 1, Ci), 1, 1, 0)
    assert torch.equal(o["sums"], ref)
    assert torch.equal(o["colsum"], D.sum(0))
    assert (o["sums"] * 4 == (o["sums"] * 4).round()).all() and o["sums"].abs().max() < 2 ** 22


def test_fused_and_unfused_staging_differ_by_ties_only():
    """On randn operands the two roundings of a prologue agree except on a few bf16 ties, and
    then by one bf16 ulp: the slack the fp64 tier adds is that and nothing more."""
    o = wo.ref_1x1(200, 64, 64, True, wo.DP_MASK, False)
    a = wo.stage_dy(o["dy"], wo.DP_MASK, o["da"], o["db"], o["dc"], o["mask"], o["z"], True).double()
    b = wo.stage_dy(o["dy"], wo.DP_MASK, o["da"], o["db"], o["dc"], o["mask"], o["z"], False).double()
    diff = (a - b).abs()
    assert float((diff > 0).double().mean()) < 0.02
    assert bool((diff <= 2.0 ** -7 * a.abs().clamp_min(b.abs())).all())


def test_share_small_of_every_bf16_case():
    """Asserted from the references alone; the smallest share is printed."""
    worst, n = 1.0, 0
    for name in wo.CASES:
        sums = wo.bf16_sums(name)
        if sums is not None:
            worst, n = min(worst, wo.share_small(sums)), n + 1
    print(f"smallest |s| < 256 share over the {n} bf16-output cases: {worst:.4%}")
    assert worst >= 0.99 and n > 100


# ------------------------------------------------------------------------------------ the report
def _planted(dy, x):
    """Three errors a wave of wgrad3x3.hip could make on (2, 14, 14) images (R = 7, 98-pixel
    chunks, 64 x 128 tiles; a wave owns one row of taps, 32 co rows and 64 ci columns):
      pixel   input pixel 137 dropped from taps 3..5 of co 32..63, ci 128..191
      halo    the bottom halo row of image 0 read from image 1's first row instead of the zero
              row: taps 0..2 of co 0..31, ci 0..63
      shift   tap 5 of co 8..15 (one 16-byte dy slot) reads one column off (tap 4's operand)
              throughout chunk 0, ci 0..63
    Returns {name: got} and the reference."""
    tp = wo.Taps(dy, x)
    want = tp.sums()
    N, H, W = tp.shape
    out = {}
    got = want.clone()
    for t in (3, 4, 5):
        A, B = tp.pair(t)
        got[32:64, t, 128:192] -= torch.outer(A[137, 32:64], B[137, 128:192])
    out["pixel"] = got
    bug = wo.Taps(dy, x)
    bug._padded(bug.dy)[0, H + 1, 1:W + 1] = bug.dy[1, 0]
    got = want.clone()
    rows = slice((H - 1) * W, H * W)          # the input pixels whose dy operand is that halo row
    for t in (0, 1, 2):
        Ab, B = bug.pair(t)
        A, _ = tp.pair(t)
        assert torch.equal(Ab[H * W:], A[H * W:]) and torch.equal(Ab[:(H - 1) * W], A[:(H - 1) * W])
        got[0:32, t, 0:64] += (Ab[rows, 0:32] - A[rows, 0:32]).t() @ B[rows, 0:64]
    out["halo"] = got
    A5, B = tp.pair(5)
    A4, _ = tp.pair(4)
    got = want.clone()
    got[8:16, 5, 0:64] += (A4[:98, 8:16] - A5[:98, 8:16]).t() @ B[:98, 0:64]
    out["shift"] = got
    return out, want, tp


def test_mismatch_report_localises_planted_errors():
    dy, x = wo.ints((2, 14, 14, 128), 2, 7), wo.ints((2, 14, 14, 256), 1, 8)
    out, want, tp = _planted(dy, x)
    assert wo.dw_report(want.clone(), want, 64, 128, tp, 98) is None
    rep = wo.dw_report(out["pixel"], want, 64, 128, tp, 98)
    print(rep)

    def taps_hit(rep):
        return [s.split(":")[0] for s in rep.split("by tap: ")[1].split("\n")[0].split(", ")]

    assert taps_hit(rep) == ["3", "4", "5"]
    assert "tile (co, ci): (0, 1):" in rep and "(co % 64 // 32): 1:" in rep
    assert "(ci % 128 // 64): 0:" in rep
    assert "dropped pixel [137]" in rep and "dropped chunk" not in rep
    rep = wo.dw_report(out["halo"], want, 64, 128, tp, 98)
    print(rep)
    assert taps_hit(rep) == ["0", "1", "2"]
    assert "tile (co, ci): (0, 0):" in rep and "(co % 64 // 32): 0:" in rep
    assert "no single pixel's or chunk's contribution" in rep
    rep = wo.dw_report(out["shift"], want, 64, 128, tp, 98)
    print(rep)
    assert taps_hit(rep) == ["5"] and "(co 8, tap 5, ci" in rep
    assert "tile (co, ci): (0, 0):" in rep
    # a whole chunk dropped from one tile: named as a chunk
    got = want.clone()
    for t in range(9):
        A, B = tp.pair(t)
        got[64:128, t, 128:256] -= A[98:196, 64:128].t() @ B[98:196, 128:256]
    rep = wo.dw_report(got, want, 64, 128, tp, 98)
    assert "dropped chunk [1] of 98 pixels" in rep and "tile (co, ci): (1, 1):" in rep
    with pytest.raises(AssertionError, match="elements differ"):
        wo.assert_dw(got, want, "chunk", 64, 128, tp, 98)


def test_planted_errors_pass_both_norm_bounds():
    """The same three errors on randn operands at 256 images of 14 x 14, 256 x 256 channels
    (P = 50176 pixels, a quarter of one ResNet-50 layer-3 call at batch 1024). Each relative
    Frobenius norm is below BOTH bounds test_wgrad3x3_vs_fp32 asserts: 1e-5 sqrt(P) + 1e-4 on the
    fp32 output and 5e-3 on the bf16 output (the 1x1 and stride-2 tests allow 1e-5 / 6e-3), so
    that test passes with the error in place, while the exact comparison sees every differing
    element. The norms fall as 1 / sqrt(P): at the few hundred pixels of the exact tables' own
    shapes every norm bound sees these errors, which is why the pixel count here is that of a
    real call and not of a table case. The figures are printed
    (profiles/wgrad_oracle/README.md records them)."""
    g = torch.Generator().manual_seed(11)
    dy = torch.randn(256, 14, 14, 256, generator=g).bfloat16()
    x = torch.randn(256, 14, 14, 256, generator=g).bfloat16()
    out, want, _ = _planted(dy, x)
    P = 256 * 14 * 14
    fp32_bound, bf16_bound = 1e-5 * P ** 0.5 + 1e-4, 5e-3
    for name, got in out.items():
        rel = float((got - want).norm() / want.norm())
        n = int((got != want).sum())
        print(f"planted {name}: {n} of {want.numel()} elements differ, relative Frobenius norm "
              f"{rel:.3e} (fp32 bound {fp32_bound:.2e}, bf16 bound {bf16_bound:.0e})")
        assert n > 0 and rel < fp32_bound and rel < bf16_bound, name


# ------------------------------------------------------------------------------------ the routes
ROUTE_ENVS = [({}, wo.W3_NAMES + wo.S2_NAMES + wo.C1_TAIL + wo.C1_TILES + wo.C1_DPRO + wo.C1_DMA +
               wo.C1_DMA_XF + wo.C1_DECLINED + wo.DIRECT_NAMES + wo.FOLD_NAMES),
              ({"wgrad_dma": 0}, wo.ENV_DMA_OFF), ({"wgrad_dma_xf": 0}, wo.ENV_XF_OFF),
              ({"wgrad_dma_ns128": 8}, wo.ENV_NS128), ({"fold_wide_min": 1}, wo.FOLD_ALL_WIDE),
              ({"fold_wide_min": 0}, wo.FOLD_ALL_NARROW),
              ({"wgrad3x3_direct": 0}, ["refused3x3", wo.S2_NAMES[0]])]


@pytest.mark.parametrize("expect,names", ROUTE_ENVS, ids=[str(i) for i in range(len(ROUTE_ENVS))])
def test_case_routes(expect, names):
    """One child per environment: wgrad_settings() shows it, and wgrad_route gives every case of
    that environment's table the kernel, tile and plan the table names."""
    wo.run_child(expect, names, routes_only=True)


def test_refusals_by_route():
    L = wo._lib()
    for s in wo.W3_REFUSED:
        assert dict(L.wgrad_route("3x3", *s)) == {"ok": False} and not L.wgrad3x3_direct_ok(*s)
    for s in wo.S2_REFUSED:
        for taps in (9, 1):
            assert dict(L.wgrad_route("s2", *s, taps)) == {"ok": False}
            assert not L.wgrad3x3s2_ok(*s, taps)


def test_gram_route_and_refused_reports():
    """same=True (dy and x one storage) reports the Gram kernel exactly where gram1x1_route takes
    it: square 64 / 128 / 256 channels, fp32 output, no prologue or the dmode-3 prologue on the x
    prologue's constants; its tile and fold are gram1x1.hip's own and are not reported. A refused
    call reports {"ok": False} alone."""
    L = wo._lib()
    for C in (64, 128, 256):
        for args in ((False, 0, False), (False, 0, True), (True, 3, True)):
            r = dict(L.wgrad_route("1x1", 200, C, C, *args, True))
            assert set(r) == {"ok", "path", "splits", "cps"} and r["ok"] and r["path"] == "gram", r
            assert r["splits"] >= 1 and r["splits"] * r["cps"] >= (200 + 63) // 64, r
        assert dict(L.wgrad_route("1x1", 200, C, C, False, 0, False, False))["path"] == "staged"
        assert dict(L.wgrad_route("1x1", 200, C, C, False, 3, False, True))["path"] == "staged"
        assert dict(L.wgrad_route("1x1", 200, C, C, True, 0, False, True))["path"] == "staged"
        if C > 64:
            assert dict(L.wgrad_route("1x1", 200, C, C, False, 0, False, True, True))["path"] == "staged"
    assert dict(L.wgrad_route("1x1", 200, 512, 512, False, 0, False, True))["path"] == "staged"
    assert dict(L.wgrad_route("1x1", 200, 64, 128, False, 0, False)) == {"ok": False}
    assert dict(L.wgrad_route("1x1", 200, 128, 128, False, 7, False)) == {"ok": False}
    # inside s2_tile's limits but past the binding's own (W >= 2^15)
    assert L.wgrad_route("s2", 1, 2, 65536, 128, 128, 9) == {"ok": False}
    assert not L.wgrad3x3s2_ok(1, 2, 65536, 128, 128, 9)


def test_mistyped_variable_fails(monkeypatch):
    """A child whose environment does not produce the expected settings must fail, not test the
    default."""
    monkeypatch.setitem(wo.ENV_OF, "fold_wide_min", "CML_FOLD_WIDE_MINN")
    with pytest.raises(AssertionError, match=r"wgrad_settings\(\)"):
        wo.run_child({"fold_wide_min": 1}, [], routes_only=True)
