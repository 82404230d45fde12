"""The MXFP8 host codec (csrc/include/ocm/mx8.h) on fixed vectors: the stand-alone
program csrc/tools/ocm_quant_tests.cpp, as built and as built with ASan + UBSan (host
code only, run directly: nothing is preloaded and nothing is loaded into Python)."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("edge_groups", "amax_sweep", "fp16_convert", "e4m3_codes", "record_layout")


@pytest.mark.parametrize("binary", ["ocm_quant_tests", "ocm_quant_tests_asan"])
def test_host_codec_vectors(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_quant_kernel_uses_no_scratch():
    # as tests/test_native_unit.py does for the other kernels: the extent table is indexed
    # per lane here, which must stay a load from the kernel arguments, never a scratch copy
    from kernel_report import kernel_report

    k = kernel_report("xfer_quant.hip")
    names = k.column("name")
    assert len(names) >= 2
    for key in ("scratch", "vgpr_spills"):
        assert all(v == 0 for v in k.column(key)), dict(zip(names, k.column(key)))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_quant_tests" in out and "ocm_quant_tests_asan" in out
