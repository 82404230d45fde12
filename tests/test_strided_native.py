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
    import os
    import re
    import subprocess

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{repo}/csrc/include",
                        "-c", f"{repo}/csrc/src/kernels/xfer_strided.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 3 and len(scratch) == len(names) == len(lds)
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    assert all(s == 0 for s in spills), dict(zip(names, spills))
    assert all(s == 0 for s in lds), dict(zip(names, lds))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_strided_tests" in out and "ocm_strided_tests_asan" in out
