"""The K pipelines of gemm.hip, gemm128.hip and gemm_w4.hip, element by element, in the default
environment: integer operands whose fp32 sums are exact in any order, so every output must equal
bf16_rne(exact sum [+ bias] [+ cin]) (tests/gemm_exact.py). The shapes step the number of K-tiles
through the prologue's clamp, both buffer parities and the wrap of gemm_w4's 4-deep ring, and the
tile grids through ragged m-tile groups and the XCD remap's G % 8 != 0 branch."""
import pytest

import gemm_exact as gx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(cuda):
    gx.check_settings({})       # the default dispatch: CML_GEMM_GM = 4, CML_W4_SCHED = 0
    return cuda


@pytest.mark.parametrize("name", gx.NT256_NAMES)
def test_gemm_nt_tile256_exact(dev, name):
    gx.run_case(name, dev)


@pytest.mark.parametrize("name", gx.NT128_NAMES)
def test_gemm_nt_tile128_exact(dev, name):
    gx.run_case(name, dev)


@pytest.mark.parametrize("name", gx.GELU_NAMES)
def test_gemm_gelu_epilogues_exact_h(dev, name):
    gx.run_case(name, dev)


@pytest.mark.parametrize("name", gx.W4_NAMES)
def test_gemm_w4_exact(dev, name):
    gx.run_case(name, dev)
