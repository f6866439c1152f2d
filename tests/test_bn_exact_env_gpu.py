"""The exact BatchNorm cases of test_bn_exact_gpu.py under the read-once switches nothing else
runs: CML_BN_NT = 1 (nontemporal loads with their own bf16 unpacking), CML_BN_GRID_CAP = 3 (many
grid-stride trips already at S4's size) and CML_BN_GRID_CAP = 0 (no cap: one row iteration per
workgroup at G1). One fresh child process per setting (tests/bn_oracle.py's child mode), one after
another; each child asserts that bn_settings() shows the value it was started with and each case
its geometry under that value. S3, S4 and G1 at C = 8, 256, 2048."""
import pytest

import bn_oracle as bo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("expect", [{"bn_nt": 1}, {"bn_grid_cap": 3}, {"bn_grid_cap": 0}],
                         ids=["nt1", "cap3", "cap0"])
def test_bn_exact_switches(cuda, expect):
    res = bo.run_child(expect, bo.ENV_NAMES)
    print("channels not bit-equal:", sum(x["figures"].get("not_bit_equal", 0) for x in res),
          "seconds:", sum(x["seconds"] for x in res))
