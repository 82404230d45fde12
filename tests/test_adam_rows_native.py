"""The row-sparse fused Adam's shared header (csrc/include/ocm/adam_rows.h: the validator, the
hyper-parameter and bounds rules, the tile geometry and the launch shape, with the walk of every wave
replayed on the host): the stand-alone program csrc/tools/ocm_adam_rows_tests.cpp, as built and as
built with ASan + UBSan (host code only, run directly: nothing is preloaded and nothing is loaded into
Python), and the compiler's resource report of the kernel."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("validator", "hyper", "bounds", "walk", "shape")


@pytest.mark.parametrize("binary", ["ocm_adam_rows_tests", "ocm_adam_rows_tests_asan"])
def test_validator_rules_walk_and_shape(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_rows_kernel_uses_no_scratch_no_vector_spills_and_no_lds():
    # as tests/test_indexed_native.py does for the indexed kernel: the compiler's resource report
    import os
    import re
    import subprocess

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{repo}/csrc/include",
                        "-c", f"{repo}/csrc/src/kernels/optim_rows.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vspills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # two instantiations, by table dtype: the index type is a branch, not a template parameter
    assert len(names) == 2 and all("adam_rows_kernel" in n for n in names), names
    assert len(scratch) == len(vspills) == len(lds) == 2
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    assert all(s == 0 for s in vspills), dict(zip(names, vspills))
    assert all(s == 0 for s in lds), dict(zip(names, lds))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_adam_rows_tests" in out and "ocm_adam_rows_tests_asan" in out
