"""The gradient-norm reduction over remote accumulators (csrc/include/ocm/acc_norm.h): the
per-tensor validator, every rule accepted at its edge and refused one past it (g_off + 4 n
overflow included); the launch shape (the host variant only for one host extent within 32 bits,
the proportional split, the grid forced, no work for all-empty lists) and the workspace bound;
the C++ reference of the reduction on integer-valued inputs, squares past FLT_MAX and fp32
subnormals among them; the non-finite count on bit patterns; the clip rule. The stand-alone
program csrc/tools/ocm_acc_norm_tests.cpp, as built and as built with ASan + UBSan (host code
only, run directly: nothing is preloaded and nothing is loaded into Python)."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("validator", "shape", "reference", "nonfinite", "clip_rule")


@pytest.mark.parametrize("binary", ["ocm_acc_norm_tests", "ocm_acc_norm_tests_asan"])
def test_acc_norm_rule_validator_and_shape(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}\n" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_acc_norm_tests\n" in out and "ocm_acc_norm_tests_asan\n" in out, out
