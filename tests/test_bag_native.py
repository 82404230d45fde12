"""The pooled lookup's shared header (csrc/include/ocm/bag.h, the functions the kernel and the host
path call): the stand-alone program csrc/tools/ocm_bag_tests.cpp, as built and as built with ASan +
UBSan (host code only, run directly: nothing is preloaded and nothing is loaded into Python), and the
compiler's resource report of the kernel."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("validator", "plan", "rule")


@pytest.mark.parametrize("binary", ["ocm_bag_tests", "ocm_bag_tests_asan"])
def test_validator_plan_and_rule(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_bag_kernel_uses_no_scratch_no_spills_and_no_lds():
    # as tests/test_indexed_native.py does for the indexed kernel: the compiler's resource report
    from kernel_report import kernel_report

    k = kernel_report("xfer_bag.hip")
    names = k.column("name")
    # two instantiations (the stores): element type, weights and index type are branches inside
    assert len(names) == 2 and all("xfer_bag_kernel" in n for n in names), names
    for key in ("scratch", "vgpr_spills", "sgpr_spills", "lds"):
        assert all(v == 0 for v in k.column(key)), dict(zip(names, k.column(key)))
    # the accumulators stay in registers with room to spare: full occupancy
    assert all(v <= 64 for v in k.column("vgprs")) and all(v == 8 for v in k.column("occupancy")), k


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_bag_tests" in out and "ocm_bag_tests_asan" in out
