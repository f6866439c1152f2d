"""The exact GEMM cases of test_gemm_exact_gpu.py under the read-once A/B switches nothing else
runs: CML_GEMM_GM = 0 (n fastest) and 8 (groups of 8 m-tiles) for gemm.hip's tile order, and
CML_W4_SCHED = 2, gemm_w4.hip's alternative steady-state schedule, in all four layouts. One fresh
child process per setting (tests/gemm_exact.py's child mode); each child asserts that
dispatch_settings() shows the value it was started with."""
import pytest

import gemm_exact as gx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gm", [0, 8])
def test_gemm_nt_exact_tile_order(cuda, gm):
    gx.run_child({"gemm_gm": gm}, gx.NT256_NAMES + gx.GELU_NAMES)   # every gemm.hip epilogue


def test_gemm_w4_exact_sched2(cuda):
    gx.run_child({"w4_sched": 2}, gx.W4_NAMES)
