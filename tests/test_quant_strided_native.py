"""The strided converting tile rule, validator and plan (csrc/include/ocm/quant_strided.h,
the functions the kernel and the host side call) against the expanded plain converting
ops: the stand-alone program csrc/tools/ocm_quant_strided_tests.cpp, as built and as built
with ASan + UBSan (host code only, run directly: nothing is preloaded and nothing is
loaded into Python). And the compiler's resource report of the kernel."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("tile_rule", "plan", "validator")


@pytest.mark.parametrize("binary", ["ocm_quant_strided_tests", "ocm_quant_strided_tests_asan"])
def test_tile_rule_plan_and_validator(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_kernel_uses_no_scratch_and_the_converting_kernels_lds():
    # as tests/test_quant_native.py does for the converting kernel: no scratch, no spills, and the
    # same 256 bytes of LDS per block (64 scale bytes per wave)
    import os
    import re
    import subprocess

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{repo}/csrc/include",
                        "-c", f"{repo}/csrc/src/kernels/xfer_quant_strided.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    sspills = [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 2 and all("xfer_quant_strided_kernel" in n for n in names), names
    assert len(scratch) == len(spills) == len(sspills) == len(lds) == 2
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    assert all(s == 0 for s in spills + sspills), dict(zip(names, zip(spills, sspills)))
    assert all(s == 256 for s in lds), dict(zip(names, lds))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_quant_strided_tests" in out and "ocm_quant_strided_tests_asan" in out
