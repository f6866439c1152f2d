"""wgrad1x1.hip element by element in the default environment (tests/wgrad_oracle.py): the
register-staged kernel (tail chunks with the clamped prefetch, every tile, the x prologue and the
three dy prologues with column sums), the LDS-DMA kernel (plain and with in-LDS prologues), the
one-split direct write and the two split-K folds. Integer / dyadic operands make fp32 dW equal the
fp64 sum exactly; the same inputs run inside NaN-filled buffers with out= inside a NaN row; randn
inputs are held to the derived per-element bound. Every case asserts its path, tile, chunk and
fold through wgrad_route first."""
import pytest

import wgrad_oracle as wo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(cuda):
    wo.check_settings({})
    return cuda


@pytest.mark.parametrize("name", wo.C1_TAIL)
def test_wgrad1x1_staged_tail_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("name", wo.C1_TILES)
def test_wgrad1x1_staged_tiles_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("name", wo.C1_DPRO)
def test_wgrad1x1_staged_prologues_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("name", wo.C1_DMA)
def test_wgrad1x1_dma_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("name", wo.C1_DMA_XF)
def test_wgrad1x1_dma_prologues_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("name", wo.C1_DECLINED)
def test_wgrad1x1_dma_declined_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("name", wo.DIRECT_NAMES)
def test_wgrad1x1_direct_exact(dev, name):
    wo.run_case(name, dev)


@pytest.mark.parametrize("name", wo.FOLD_NAMES)
def test_split_fold_exact(dev, name):
    wo.run_case(name, dev)


def test_colsum_refusal_is_unreachable(dev):
    """The launch refuses column sums in a tile of more than 32768 elements (the 1024-thread
    256 x 256 tile has no registers for them), but column sums count as a prologue and the tile
    choice never gives a prologue call that tile: every channel pair the kernel accepts routes
    to a tile that has them."""
    L = wo._lib()
    for Co in (64, 128, 256, 512, 1024):
        for Ci in (64, 128, 256, 512, 1024):
            if not (Co == Ci == 64 or (Co % 256 == 0 if Ci == 64 else Co % 128 == 0)):
                assert dict(L.wgrad_route("1x1", 96, Co, Ci, False, 0, True)) == {"ok": False}
                continue
            for dmode in (0, 2, 3):
                r = dict(L.wgrad_route("1x1", 96, Co, Ci, False, dmode, True))
                assert r["ok"] and not r["direct"], (Co, Ci, dmode, r)
                assert r["path"] == "dma" or r["TM"] * r["TN"] <= 32768, (Co, Ci, dmode, r)
