"""The one-read symmetric Gram kernel (gram1x1.hip, reached through wgrad1x1_ex(z, z, ...)):
G = y^T y and the column sums of y, y = bf16(relu(z sc + bi)) or z, against the fp64 oracle with
the tolerance of test_bwd_fusion_gpu.py::test_bn_stats_gram_vs_fp64; bitwise symmetry and
run-to-run determinism; ragged pixel counts (padding rows must be zeroed after the transform); and
at many splits the error against that of the weight-gradient path (CML_GRAM_SYRK=0, child process).
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# N, H (square images): 9 pixels (less than one chunk), 243 (ragged), 1568
SHAPES = [(1, 3), (3, 9), (2, 28)]
BIG = (8, 56)   # 25088 pixels: many splits (p = 64)


def _lib():
    from consensusml_amd.ops.native import lib
    return lib()


def _inputs(dev, p, N, H, seed=7, bias=None):
    g0 = torch.Generator(device=dev).manual_seed(seed + 131 * p + H)
    z = torch.randn(N, p, H, H, device=dev, generator=g0).bfloat16()
    z = z.contiguous(memory_format=torch.channels_last)
    sc = torch.rand(p, device=dev, generator=g0) + 0.5
    bi = torch.randn(p, device=dev, generator=g0) * 0.1 + 0.2
    if bias is not None:
        bi = torch.full_like(bi, bias)
    return z, sc, bi


def _rows(z):
    return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).float()


def _oracle(z, sc, bi, pro):
    """fp64 Gram matrix and column sums of y. The prologue is one fused multiply-add per element
    rounded to fp32, then to bf16: z sc + bi is formed in fp64 (the product of a bf16 and an fp32
    is exact there) and rounded to fp32 once; an fp32 multiply followed by an add would round
    twice and now and then land on the neighbouring bf16."""
    if not pro:
        y = _rows(z).double()
    else:
        y = torch.relu((_rows(z).double() * sc.double() + bi.double()).float()).bfloat16().double()
    return y.t() @ y, y.sum(0)


def _gram(z, sc, bi, pro, colsum):
    if pro:
        return _lib().wgrad1x1_ex(z, z, sc, bi, 3, None, sc, bi, None, colsum)
    return _lib().wgrad1x1_ex(z, z, None, None, 0, None, None, None, None, colsum)


def _check(z, sc, bi, pro, colsum):
    G, cy = _gram(z, sc, bi, pro, colsum)
    G_ref, cy_ref = _oracle(z, sc, bi, pro)
    err = (G.double() - G_ref).abs().max().item()
    print(f"p={z.shape[1]} M={z.numel() // z.shape[1]} pro={pro} max abs err {err:.3e}")
    torch.testing.assert_close(G.double(), G_ref, rtol=1e-5, atol=1e-3)
    assert torch.equal(G, G.t())
    if colsum:
        torch.testing.assert_close(cy.double(), cy_ref, rtol=1e-5, atol=1e-3)
    else:
        assert cy is None or cy.numel() == 0
    G2, cy2 = _gram(z, sc, bi, pro, colsum)
    assert torch.equal(G, G2)
    if colsum:
        assert torch.equal(cy, cy2)


@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("N,H", SHAPES)
@pytest.mark.parametrize("p", [64, 128, 256])
def test_gram_vs_fp64(cuda, p, N, H, pro, colsum):
    z, sc, bi = _inputs(cuda, p, N, H)
    _check(z, sc, bi, pro, colsum)


@pytest.mark.parametrize("p", [64, 128, 256])
def test_gram_mostly_zero(cuda, p):
    """bi strongly negative: most of y is zero."""
    z, sc, bi = _inputs(cuda, p, 2, 28, bias=-3.0)
    _check(z, sc, bi, True, True)


@pytest.mark.parametrize("p", [64, 128, 256])
def test_gram_ragged_positive_bias(cuda, p):
    """bi > 0 on a ragged pixel count: a padding row that was transformed instead of zeroed would
    add relu(bi)^2 to every entry."""
    z, sc, bi = _inputs(cuda, p, 3, 9, bias=1.0)
    _check(z, sc, bi, True, True)


def _big_error(dev, pro):
    z, sc, bi = _inputs(dev, 64, *BIG)
    G, cy = _gram(z, sc, bi, pro, True)
    G_ref, cy_ref = _oracle(z, sc, bi, pro)
    return G, cy, (G.double() - G_ref).abs().max().item(), (cy.double() - cy_ref).abs().max().item()


@pytest.mark.parametrize("pro", [False, True])
def test_gram_many_splits_vs_parent_path(cuda, pro):
    """25088 pixels at p = 64. The two paths differ only in fp32 summation order, so the new
    kernel may have twice the weight-gradient path's maximum absolute error against the same fp64
    oracle: that covers the order and does not hide a lost chunk (one chunk is 64 of 25088 rows,
    about 0.3 % of every entry, thousands of times the rounding error)."""
    G, cy, err, err_cy = _big_error(cuda, pro)
    env = dict(os.environ, PYTHONPATH=ROOT, CML_GRAM_SYRK="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(int(pro))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    par = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"pro={pro} G max abs err: new {err:.3e} parent {par['err']:.3e}; "
          f"cy: new {err_cy:.3e} parent {par['err_cy']:.3e}")
    assert par["syrk"] == "0"
    assert err <= 2 * par["err"], (err, par["err"])
    torch.testing.assert_close(cy.double(), _oracle(*_inputs(cuda, 64, *BIG), pro)[1],
                               rtol=1e-5, atol=1e-3)
    assert torch.equal(G, G.t())
    G2, cy2, _, _ = _big_error(cuda, pro)
    assert torch.equal(G, G2) and torch.equal(cy, cy2)


if __name__ == "__main__":   # the parent path's errors, for test_gram_many_splits_vs_parent_path
    _, _, e, ec = _big_error(torch.device("cuda", 0), bool(int(sys.argv[1])))
    print(json.dumps({"syrk": os.environ.get("CML_GRAM_SYRK"), "err": e, "err_cy": ec}))
