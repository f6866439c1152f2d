"""tests/gemm_exact.py without a GPU: the reference's rounding points and its conv gather, the
input condition, the mismatch report, and -- since conv_gemm_route and dispatch_settings only
evaluate host predicates -- that every conv case table names the route its environment gives."""
import pytest
import torch
import torch.nn.functional as F

import gemm_exact as gx


def test_expected_rounds_twice_with_cin():
    """bf16 keeps 8 significant bits: 257 is a tie and rounds to the even 256. Adding cin = 1 after
    that rounding gives 257 -> 256; a single rounding of 258 would give 258."""
    s = torch.tensor([[257.0, 259.0, -3.0]], dtype=torch.float64)
    one = torch.ones(1, 3).bfloat16()
    assert gx.expected(s).tolist() == [[256.0, 260.0, -3.0]]
    assert gx.expected(s, cin=one).tolist() == [[256.0, 260.0, -2.0]]
    assert gx.expected(s, bias=one[0]).tolist() == [[258.0, 260.0, -2.0]]


@pytest.mark.parametrize("Nimg,C,Co,H,W,taps,stride", [(2, 64, 8, 5, 7, 9, 1), (2, 64, 8, 8, 6, 9, 2),
                                                       (3, 64, 8, 7, 5, 9, 2), (2, 64, 8, 4, 3, 1, 1)])
def test_conv_sums_equal_fp64_conv2d(Nimg, C, Co, H, W, taps, stride):
    """On integers the fp64 direct convolution of the CPU is exact as well, whatever its order."""
    x, w, s = gx.conv_ref(Nimg, C, Co, H, W, taps, stride)
    k = 3 if taps == 9 else 1
    w4 = w.double().view(Co, k, k, C).permute(0, 3, 1, 2)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w4, stride=stride, padding=k // 2)
    assert torch.equal(ref.permute(0, 2, 3, 1).reshape(-1, Co), s)
    assert s.abs().max() > 0


def test_share_small_asserts():
    assert gx.share_small(torch.tensor([1.0, -255.0])) == 1.0
    with pytest.raises(AssertionError):
        gx.share_small(torch.tensor([1.0] * 97 + [256.0] * 3))


def test_mismatch_report_localises():
    want = gx.ints((512, 512), 2, 5)
    assert gx.mismatch_report(want.clone(), want) is None
    got = want.clone()
    got[256 + 32:256 + 48, 64:72] += 8       # one 16-byte chunk of a 16-row fragment, tile (1, 0)
    rep = gx.mismatch_report(got, want)
    assert rep.startswith("128 of 262144 elements differ")
    assert "(row 288, col 64)" in rep
    assert "(1, 0): 128" in rep and "(row % 256 // 16): 2: 128" in rep
    assert "(col % 256 // 64): 1: 128" in rep
    with pytest.raises(AssertionError, match="128 of 262144"):
        gx.assert_exact(got, want, "chunk")


def test_case_tables_fit_the_exactness_bound():
    for name, fn in gx.CASES.items():
        kw = fn.keywords
        K = kw["taps"] * kw["C"] if name.startswith("conv-") else kw["K"]
        assert K % 64 == 0 and 2 * K < 2 ** 24 and K <= 4608, name
    assert len(set(gx.NT256_NAMES + gx.NT128_NAMES + gx.GELU_NAMES + gx.W4_NAMES)) == 8 + 5 + 4 + 36


ROUTE_ENVS = [({}, gx.CONV_DEFAULT),
              ({"conv_gemm_smallm": 0}, gx.CONV_GEMM2_SQUARE),
              ({"conv_gemm_smallm": 0, "conv_gemm2": 0}, gx.CONV_VARIANT4),
              ({"gemm2_tall": 1}, gx.CONV_TALL)] + \
             [({"conv_gemm2": 0, "conv_gemm_variant": k, "conv_gemm_narrow": k}, gx.CONV_AB[k])
              for k in (1, 2, 3)]


@pytest.mark.parametrize("expect,names", ROUTE_ENVS, ids=[str(i) for i in range(len(ROUTE_ENVS))])
def test_conv_case_routes(expect, names):
    """One child per environment: dispatch_settings() shows it, and conv_gemm_route gives every
    case of that environment's table the kernel and tile the table names."""
    gx.run_child(expect, names, routes_only=True)


def test_mistyped_variable_fails(monkeypatch):
    """A child whose environment does not produce the expected settings must fail, not test the
    default."""
    monkeypatch.setitem(gx.ENV_OF, "gemm_gm", "CML_GEMM_GMM")
    with pytest.raises(AssertionError, match=r"dispatch_settings\(\)"):
        gx.run_child({"gemm_gm": 8}, [], routes_only=True)
