"""The LPC analysis's kernel (csrc/vs_lpc.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950 without
a GPU): no scratch and no spill, and no trap instruction in the gfx950 listing -- a frame the kernel cannot analyse says
so in its record's status."""
import resource_checks as rc

SRC = "vs_lpc.hip"


def test_the_lpc_kernel_uses_no_scratch():
    recs = rc.records(SRC)
    assert any("vs_lpc_kernel" in n for n in recs), list(recs)
    rc.assert_no_scratch_or_spill(recs)


def test_no_trap_in_the_listing(tmp_path):
    rc.assert_no_trap(rc.listing(SRC, tmp_path), "vs_lpc_kernel")
