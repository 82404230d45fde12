"""The plan every descriptor list shares (csrc/include/ocm/list.h: the prefix-sum plan, the
wave table and the cut of a wave's tile range) under the batch, converting, strided and
accumulate tile-count rules, and the walk of the kernels whose ops have rows (list_enter_op,
list_locate, list_next_piece), against a brute-force walk: the stand-alone program
csrc/tools/ocm_list_tests.cpp, as built and as built with ASan + UBSan (host code only,
run directly: nothing is preloaded and nothing is loaded into Python)."""
import pytest

from oncilla_amd.utils.paths import BUILD_DIR

PARTS = ("batch", "batch_unit256", "quant", "strided", "acc", "row_walk", "wave_range")


@pytest.mark.parametrize("binary", ["ocm_list_tests", "ocm_list_tests_asan"])
def test_list_plan_and_wave_table(native, tool, binary):
    rc, out = tool([f"{native}/{binary}"])
    assert rc == 0, out
    for name in PARTS:
        assert f"PASS {name}\n" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out


def test_registered_with_ctest(native, tool):
    rc, out = tool(["ctest", "--test-dir", BUILD_DIR, "-N"])
    assert rc == 0, out
    assert "ocm_list_tests" in out and "ocm_list_tests_asan" in out
