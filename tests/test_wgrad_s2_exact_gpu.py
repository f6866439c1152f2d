"""The stride-2 implicit-im2col gather of wgrad1x1.hip's LDS-DMA kernel (wgrad3x3s2, 9 taps and the
single tap) element by element in the default environment (tests/wgrad_oracle.py): exact integer
sums, the same inputs inside NaN-filled buffers with the zero row passed explicitly, and randn
inputs against the derived bound. All four tiles (128 / 256 x 128 / 256) at one chunk, one chunk
over eight images, image boundaries mid-chunk, non-square images and several splits; two 512 x 512
cases and a 384 x 384 one put several chunks into a split. Every case asserts tile, stages and
splits through wgrad_route first."""
import pytest

import wgrad_oracle as wo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(cuda):
    wo.check_settings({})
    return cuda


@pytest.mark.parametrize("name", wo.S2_NAMES)
def test_wgrad_s2_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("taps", [9, 1])
def test_wgrad_s2_refusals(dev, taps):
    """test_wgrad3x3s2_plan_limits' three (odd image, 25 output pixels, Co = 64) and Ci = 64."""
    L = wo._lib()
    for shape in wo.S2_REFUSED:
        assert dict(L.wgrad_route("s2", *shape, taps)) == {"ok": False}, shape
        assert not L.wgrad3x3s2_ok(*shape, taps), shape
