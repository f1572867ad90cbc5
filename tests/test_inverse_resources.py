"""The inverse filter's kernels (csrc/vs_inverse.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950
without a GPU): no scratch and no spill in any instantiation (the taps and the window of u are registers with static
indices, the reflection coefficients are in LDS), and no trap instruction in the gfx950 listing -- a row without a usable
set says so in its status record."""
import resource_checks as rc

SRC = "vs_inverse.hip"


def test_the_inverse_kernels_use_no_scratch():
    recs = rc.records(SRC)
    kernels = [n for n in recs if "vs_inverse_kernel" in n]
    assert len(kernels) == 8, list(recs)         # arithmetic x window class x mode
    rc.assert_no_scratch_or_spill(recs)


def test_no_trap_in_the_listing(tmp_path):
    rc.assert_no_trap(rc.listing(SRC, tmp_path), "vs_inverse_kernel")
