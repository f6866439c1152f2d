"""The exact weight-gradient cases under the read-once A/B switches nothing else runs. One fresh
child process per setting (tests/wgrad_oracle.py's child mode, one at a time); each child asserts
that wgrad_settings() shows the value it was started with and each case the route it expects
there: CML_WGRAD_DMA=0 puts DMA-shaped calls on the staged kernel, CML_WGRAD_DMA_XF=0 only the
prologue ones, CML_WGRAD_DMA_NS128=8 runs the 128 x 128 stride-2 tile on 8 stages,
CML_FOLD_WIDE_MIN=1 / 0 makes every fold wide / narrow, CML_WGRAD3X3_DIRECT=0 turns the nine-tap
kernel off."""
import pytest

import wgrad_oracle as wo

pytestmark = pytest.mark.gpu


def test_wgrad_dma_off(cuda):
    wo.run_child({"wgrad_dma": 0}, wo.ENV_DMA_OFF)


def test_wgrad_dma_xf_off(cuda):
    wo.run_child({"wgrad_dma_xf": 0}, wo.ENV_XF_OFF)


def test_wgrad_s2_tile128_eight_stages(cuda):
    wo.run_child({"wgrad_dma_ns128": 8}, wo.ENV_NS128)


def test_fold_all_wide(cuda):
    wo.run_child({"fold_wide_min": 1}, wo.FOLD_ALL_WIDE)


def test_fold_all_narrow(cuda):
    wo.run_child({"fold_wide_min": 0}, wo.FOLD_ALL_NARROW)


def test_wgrad3x3_direct_off(cuda):
    """Every shape of the table is refused, and the other kernels are untouched."""
    wo.run_child({"wgrad3x3_direct": 0}, ["refused3x3", wo.S2_NAMES[0]])
