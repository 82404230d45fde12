"""The accumulate element rule, validator and tile count (csrc/include/ocm/acc.h) on fixed
vectors: the stand-alone program csrc/tools/ocm_acc_tests.cpp, as built and as built with
ASan + UBSan (host code only, run directly: nothing is preloaded and nothing is loaded
into Python), and the kernel's resource usage."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("element_rule", "widen16", "apply_host", "validator", "tile_counts")


@pytest.mark.parametrize("binary", ["ocm_acc_tests", "ocm_acc_tests_asan"])
def test_rule_validator_and_tiles(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_acc_kernel_uses_no_scratch():
    # as tests/test_quant_native.py does for its kernel: the extent table is indexed per lane,
    # which must stay a load from the kernel arguments, never a scratch copy
    import os
    import re
    import subprocess

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{repo}/csrc/include",
                        "-c", f"{repo}/csrc/src/kernels/xfer_acc.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] + \
             [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) >= 2 and len(scratch) == len(names)
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    assert all(s == 0 for s in spills), spills
    assert all(v == 0 for v in lds), dict(zip(names, lds))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_acc_tests" in out and "ocm_acc_tests_asan" in out
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-R", "ocm_acc_tests"])
    assert rc == 0 and "100% tests passed" in out, out
