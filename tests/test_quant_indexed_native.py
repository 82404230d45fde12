"""The indexed converting descriptor, validator, plan and host-path model
(csrc/include/ocm/quant_indexed.h, the functions the kernel and the host side call) against the
expanded plain converting ops: the stand-alone program csrc/tools/ocm_quant_indexed_tests.cpp, as
built and as built with ASan + UBSan (host code only, run directly: nothing is preloaded and
nothing is loaded into Python). And the compiler's resource report of the kernel."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("tile_rule", "plan", "validator", "host_model")


@pytest.mark.parametrize("binary", ["ocm_quant_indexed_tests", "ocm_quant_indexed_tests_asan"])
def test_tile_rule_plan_validator_and_host_model(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_kernel_uses_no_scratch_and_the_converting_kernels_lds():
    # as tests/test_quant_strided_native.py does for the strided converting kernel: two kernels, no
    # scratch, no spills, and the same 256 bytes of LDS per block (64 scale bytes per wave)
    from kernel_report import kernel_report

    k = kernel_report("xfer_quant_indexed.hip")
    names = k.column("name")
    assert len(names) == 2 and all("xfer_quant_indexed_kernel" in n for n in names), names
    for key in ("scratch", "vgpr_spills", "sgpr_spills"):
        assert all(v == 0 for v in k.column(key)), dict(zip(names, k.column(key)))
    assert all(v == 256 for v in k.column("lds")), dict(zip(names, k.column("lds")))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_quant_indexed_tests" in out and "ocm_quant_indexed_tests_asan" in out
