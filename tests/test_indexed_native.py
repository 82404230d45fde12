"""The indexed ops' shared header (csrc/include/ocm/indexed.h, the functions the kernel and the host
path call): the stand-alone program csrc/tools/ocm_indexed_tests.cpp, as built and as built with
ASan + UBSan (host code only, run directly: nothing is preloaded and nothing is loaded into
Python), and the compiler's resource report of the kernel."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("geometry", "bounds", "validator", "plan")


@pytest.mark.parametrize("binary", ["ocm_indexed_tests", "ocm_indexed_tests_asan"])
def test_geometry_bounds_validator_and_plan(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_indexed_kernel_uses_no_scratch_no_spills_and_no_lds():
    # as tests/test_strided_native.py does for the strided kernel: the compiler's resource report
    from kernel_report import kernel_report

    k = kernel_report("xfer_indexed.hip")
    names = k.column("name")
    # three instantiations, as the strided kernel has: the index type is a branch, not a template parameter
    assert len(names) == 3 and all("xfer_indexed_kernel" in n for n in names), names
    for key in ("scratch", "vgpr_spills", "sgpr_spills", "lds"):
        assert all(v == 0 for v in k.column(key)), dict(zip(names, k.column(key)))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_indexed_tests" in out and "ocm_indexed_tests_asan" in out
