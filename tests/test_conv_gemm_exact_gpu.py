"""The implicit-GEMM gathers of conv_gemm.hip and of gemm.hip's conv mode, element by element
(tests/gemm_exact.py: integer operands, nine shifted slices and one fp64 matmul per tap as the
reference), on every dispatch branch: each case first asserts the kernel and tile that
conv_gemm_route reports, then compares conv_gemm bitwise, then conv_gemm_bn / conv_gemm_bnsums
(same y; statistics and sums against fp64 of the stored output).

Small shapes do not reach the 256 x 256 tiles by themselves (fewer than CML_CONV_GEMM_SMALLM = 512
of them), nor the 512 x 128 tile (fewer than CML_GEMM2_TALL = 1024), so those branches run in
child processes with the thresholds lowered: gemm.hip's square conv mode (what ResNet-50's layers
3 and 4 run at the benchmark's batch), conv_gemm.hip's own variant 4, the tall tile at stride 1
and 2, and the A/B variants 1-3 of the wide and narrow tiles."""
import pytest

import gemm_exact as gx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", gx.CONV_DEFAULT)
def test_conv_gemm_exact_default_route(cuda, name):
    gx.check_settings({})
    gx.run_case(name, cuda)


def test_conv_gemm_exact_gemm2_square(cuda):
    gx.run_child({"conv_gemm_smallm": 0}, gx.CONV_GEMM2_SQUARE)


def test_conv_gemm_exact_variant4(cuda):
    gx.run_child({"conv_gemm_smallm": 0, "conv_gemm2": 0}, gx.CONV_VARIANT4)


def test_conv_gemm_exact_gemm2_tall(cuda):
    gx.run_child({"gemm2_tall": 1}, gx.CONV_TALL)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_conv_gemm_exact_ab_variants(cuda, k):
    gx.run_child({"conv_gemm2": 0, "conv_gemm_variant": k, "conv_gemm_narrow": k}, gx.CONV_AB[k])
