"""The fused Adam launch shape (csrc/include/ocm/optim.h, adam_launch_shape): which kernel
variant runs and on what grid, for one tensor and for lists, on HBM and host-tier state and
under every knob, against numbers from the launcher's arithmetic before the function existed;
and the state space of the optimizer kernels (csrc/include/ocm/state_space.h): its launch-time
check at every edge and its address arithmetic, both branches, against the plain definition.
The stand-alone program csrc/tools/ocm_adam_plan_tests.cpp, as built and as built with
ASan + UBSan (host code only, run directly: nothing is preloaded and nothing is loaded into
Python)."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("one_tensor", "lists", "host_variant", "knobs", "space")


@pytest.mark.parametrize("binary", ["ocm_adam_plan_tests", "ocm_adam_plan_tests_asan"])
def test_adam_launch_shape(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}\n" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_adam_plan_tests" in out and "ocm_adam_plan_tests_asan" in out
