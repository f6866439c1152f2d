"""Every form of ``agg_update.hip``'s dispatch space gives, bit for bit, what it gave before the
kernel and launch ladders were folded into one table (``agg_dispatch_golden.py`` lists the cases;
``test_meamed_gpu.py::test_plain_paths_bit_identical_to_parent`` pins the plain sorted combine)."""
import os

import pytest
import torch

from consensusml_amd.ops import kernels as K
from agg_dispatch_golden import golden_calls, multi_cases, single_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "agg_dispatch_parent.pt")


def test_dispatch_space_bit_identical_to_parent(cuda):
    """The file was recorded on an MI355X with
    ``python tests/agg_dispatch_golden.py tests/golden/agg_dispatch_parent.pt`` in a checkout of
    the commit before the fold (see ``agg_dispatch_golden.py``)."""
    want = torch.load(GOLDEN, weights_only=True)
    got = golden_calls(K, cuda)
    ncases = len(single_cases()) + len(multi_cases())
    assert sorted(got) == sorted(want) and len(got) == 3 * ncases == 129
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
