"""The strided tile geometry and validator (csrc/include/ocm/strided.h, the functions the
kernel calls) over every tile of a grid of layouts: the stand-alone program
csrc/tools/ocm_strided_tests.cpp, as built and as built with ASan + UBSan (host code only,
run directly: nothing is preloaded and nothing is loaded into Python)."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("geometry", "plan", "validator")


@pytest.mark.parametrize("binary", ["ocm_strided_tests", "ocm_strided_tests_asan"])
def test_tile_geometry_and_validator(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_strided_kernel_uses_no_scratch_and_no_lds():
    # as tests/test_quant_native.py does for the converting kernel: the compiler's resource report
    from kernel_report import kernel_report

    k = kernel_report("xfer_strided.hip")
    names = k.column("name")
    assert len(names) == 3
    for key in ("scratch", "vgpr_spills", "lds"):
        assert all(v == 0 for v in k.column(key)), dict(zip(names, k.column(key)))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_strided_tests" in out and "ocm_strided_tests_asan" in out
