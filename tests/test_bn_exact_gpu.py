"""bn_act.hip's launches (bn_stats, bn_fwd, bn_bwd, bn_bwd_sums, bn_bwd_apply, bn_fwd2, bn_bwd2)
against the exact and fp64 oracles of tests/bn_oracle.py across the kernels' dispatch space: one
row, fewer rows than row slots, the unrolled statistics loop and its tails, a short last workgroup
(S1 - S4, all nine channel counts), the capped apply grid with the second row in flight (G1), the
unrolled finalize fold and a third apply trip (G2), and the workgroup cap (G3). Every case first
asserts through bn_geometry that it reaches the branch it is named for; the bounds are the
oracle's (bit equality, one fp32 ulp for the statistics, the derived fp64-tier bound)."""
import pytest

import bn_oracle as bo

pytestmark = pytest.mark.gpu

NAMES = [n for n in bo.CASES if n not in bo.ENV_ONLY]


@pytest.mark.parametrize("name", NAMES)
def test_bn_exact(cuda, name):
    fig, _ = bo.run_case(name, cuda)
    # expected: every statistic bit-equal (1 ulp is what the comparison allows)
    print(f"{name}: channels not bit-equal {fig.get('not_bit_equal', 0)}, mask bits left out "
          f"{fig.get('left_out', 0.0):.4%}")
