"""The library's knobs as csrc/src/lib/config.cpp reads them from the environment: defaults,
clamps at both ends, the couplings between variables, and that a second parse keeps nothing
from the first (what a second ocm_init in one process sees). The stand-alone program
csrc/tools/ocm_config_tests.cpp, as built and as built with ASan + UBSan (host code only,
run directly: nothing is preloaded and nothing is loaded into Python)."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("defaults", "clamps", "couplings", "determinism")


@pytest.mark.parametrize("binary", ["ocm_config_tests", "ocm_config_tests_asan"])
def test_config_from_env(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}\n" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_config_tests" in out and "ocm_config_tests_asan" in out
