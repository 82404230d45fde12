"""The accumulator side of the fused Adam (csrc/include/ocm/optim.h): the per-tensor validator
adam_acc_check, every rule accepted at its edge and refused one past it, and the launch shape
over two state spaces, adam_acc_launch_shape (the PCIe variant only when both spaces are one
host extent within 32 bits; the span of each; the knobs; agreement with adam_launch_shape
where no accumulators are involved). The stand-alone program
csrc/tools/ocm_adam_acc_tests.cpp, as built and as built with ASan + UBSan (host code only,
run directly: nothing is preloaded and nothing is loaded into Python)."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("validator", "overlap", "variant", "knobs", "agrees_without_accumulators")


@pytest.mark.parametrize("binary", ["ocm_adam_acc_tests", "ocm_adam_acc_tests_asan"])
def test_adam_acc_validator_and_shape(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}\n" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_adam_acc_tests\n" in out and "ocm_adam_acc_tests_asan\n" in out, out
