"""The acoustic measurement's kernels (csrc/vs_acoustic.hip), compiled here with the SHIPPED flags (hipcc cross-compiles
gfx950 without a GPU): no scratch in any of them, and no trap instruction in the gfx950 listing -- a row the kernels
cannot measure says so in its record's status."""
import resource_checks as rc

SRC = "vs_acoustic.hip"


def test_no_kernel_of_the_measurement_uses_scratch():
    recs = rc.records(SRC)
    assert any("vs_ac_period_kernel" in n for n in recs) and any("vs_ac_marks_kernel" in n for n in recs), list(recs)
    rc.assert_no_scratch_or_spill(recs)


def test_no_trap_in_the_listing(tmp_path):
    rc.assert_no_trap(rc.listing(SRC, tmp_path), "vs_ac_marks_kernel", "vs_ac_period_kernel")
