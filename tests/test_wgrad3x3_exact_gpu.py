"""wgrad3x3.hip element by element in the default environment (tests/wgrad_oracle.py): integer
operands whose fp32 sums are exact in any order, so fp32 dW must equal the fp64 sum and bf16 dW its
bf16 rounding; the same inputs inside NaN-filled buffers with the zero row passed explicitly; and
randn inputs against the derived per-element bound. Every case asserts its chunk geometry (R, G,
npx, nch, splits, cps, tci, dy_rows, grid) through wgrad_route first: multi-image, whole-image,
single-row and multi-row chunks, the LDS row limit, one-split, one-chunk-per-split and ragged
plans, grids below, off and on a multiple of the XCD remap's 8."""
import pytest

import wgrad_oracle as wo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(cuda):
    wo.check_settings({})
    return cuda


@pytest.mark.parametrize("name", wo.W3_NAMES)
def test_wgrad3x3_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("shape", wo.W3_REFUSED, ids=["x".join(map(str, s)) for s in wo.W3_REFUSED])
def test_wgrad3x3_refusals(dev, shape):
    """No chunk geometry (W = 113 is wider than a chunk) or one past the LDS row limit (W = 1 with
    H = 120; 28 images of 2 x 2): the route says so and wgrad3x3_direct_ok agrees, with
    CML_WGRAD3X3_DIRECT at its default."""
    L = wo._lib()
    assert dict(L.wgrad_settings())["wgrad3x3_direct"] == 1
    assert dict(L.wgrad_route("3x3", *shape)) == {"ok": False}
    assert not L.wgrad3x3_direct_ok(*shape)
