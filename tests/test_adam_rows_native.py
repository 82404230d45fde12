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
    from kernel_report import kernel_report

    k = kernel_report("optim_rows.hip")
    names = k.column("name")
    # two instantiations, by table dtype: the index type is a branch, not a template parameter
    assert len(names) == 2 and all("adam_rows_kernel" in n for n in names), names
    for key in ("scratch", "vgpr_spills", "lds"):
        assert all(v == 0 for v in k.column(key)), dict(zip(names, k.column(key)))


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_adam_rows_tests" in out and "ocm_adam_rows_tests_asan" in out
