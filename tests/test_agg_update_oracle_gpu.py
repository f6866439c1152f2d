"""``csrc/kernels/agg_update.hip`` against the float64 oracle of ``agg_oracle.py`` across its
dispatch space: both row dtypes, every padded sort size and vector width, the weighted unroll
and remainder, every optimizer flag, ``rows`` indirection, both parameter dtypes, the scalar
tail and the fully scalar (misaligned) launch, and the multi-segment kernels including the
second and later trips of their grid-stride loop. The assertions are (a)-(e) of ``agg_oracle``.

Grid-stride sizes: one launch over ``nseg`` segments has at most ``2048 / nseg`` workgroups of
256 threads per segment, so with 16 segments one trip covers 128 * 256 = 32768 vectors of
8 (bf16 rows), 4 (fp32 rows) or 2 (n > 32) elements. The ``stride-`` cases hold one segment of
three such trips plus a ragged rest (3 * 262144 + 296, 3 * 131072 + 36 and 3 * 65536 + 22
elements); ``test_case_table_covers_the_dispatch_space`` ties these sizes to the cap."""
import pytest
import torch

import agg_oracle as AO
from consensusml_amd.ops import kernels as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", AO.CASES, ids=lambda c: c.id)
def test_agg_update_oracle(cuda, case):
    AO.run_case(case, cuda, K)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", AO.MULTI_CASES, ids=lambda c: c.id)
def test_agg_update_multi_oracle(cuda, case):
    AO.run_multi_case(case, cuda, K)
    torch.cuda.synchronize()
