"""The hand-off of bn1's deferred backward (``ops.bn.DeferredBN1``) without a GPU: the guard that
keeps conv1's backward from taking an unapplied gradient for dz1, and the slots' clearing."""
import pytest
import torch

from consensusml_amd.ops import bn as fbn


def test_pointer_mismatch_raises():
    """CPU-side: a gradient that is not the recorded dy1 must never be taken for dz1."""
    z1 = torch.zeros(1, 8, 2, 2)
    dy1 = torch.zeros(1, 8, 2, 2)
    hand = fbn.DeferredBN1()
    hand.rec = (z1, None, None, None, None, None, None, dy1.data_ptr())
    rec = hand.take()
    assert hand.rec is None and hand.take() is None          # cleared when taken
    fbn.check_deferred_grad(rec, dy1)                        # the very tensor: accepted
    with pytest.raises(RuntimeError, match="not the dy1"):
        fbn.check_deferred_grad(rec, dy1.clone())
    hand.rec, hand.armed = rec, True
    hand.clear()                                             # what conv1's forward does first
    assert hand.rec is None and not hand.armed
