"""The MXFP4 host codec and the rules the kernel shares with it (csrc/include/ocm/mx4.h), and the
strided location of MXFP4 tiles (csrc/include/ocm/quant_strided.h): the stand-alone program
csrc/tools/ocm_mx4_tests.cpp, as built and as built with ASan + UBSan (host code only, run
directly: nothing is preloaded and nothing is loaded into Python). And the compiler's resource
report of both converting kernels, which now hold the MXFP4 tile bodies too."""
import pytest
from kernel_report import kernel_report

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("edge_groups", "amax_sweep", "e2m1_codes", "record_layout", "strided_tile_location")


@pytest.mark.parametrize("binary", ["ocm_mx4_tests", "ocm_mx4_tests_asan"])
def test_host_codec_and_shared_rules(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_mx4_tests" in out and "ocm_mx4_tests_asan" in out


@pytest.mark.parametrize("kernel", ["xfer_quant", "xfer_quant_strided"])
def test_kernels_hold_the_fp4_converts_and_use_no_scratch(kernel):
    # the MXFP4 bodies are inlined into the two kernels of each file: the packed fp4 converts are in
    # their code, and they still use no scratch, spill nothing and keep 64 scale bytes of LDS per wave
    k = kernel_report(f"{kernel}.hip", emit="asm")
    assert len(k) == 2, k.column("name")
    for key in ("scratch", "vgpr_spills", "sgpr_spills"):
        assert k.column(key) == [0, 0], (key, k.column(key))
    assert k.column("lds") == [256, 256]
    for insn in ("v_cvt_scalef32_pk_fp4_bf16", "v_cvt_scalef32_pk_fp4_f16", "v_cvt_scalef32_pk_bf16_fp4",
                 "v_cvt_scalef32_pk_f16_fp4"):
        assert k.asm.count(insn) >= 8, (insn, k.asm.count(insn))  # four per tile body, two kernels
