"""The two PSOLA kernels (csrc/vs_psola.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950 without a
GPU): both are found, neither uses scratch nor spills a register, vector or scalar, the overlap-add kernel's static LDS is
the figure vs_psola.h states and the plan kernel has none, and the listing holds no trap.  A resource test only."""
import os

import resource_checks as rc

SRC = "vs_psola.hip"
HEADER = os.path.join(rc.CSRC, "vs_psola.h")


def test_the_psola_kernels_use_no_scratch_and_spill_nothing():
    recs = rc.records(SRC)
    names = sorted(recs)
    assert len(names) == 2 and "vs_ps_ola_kernel" in names[0] and "vs_ps_plan_kernel" in names[1], names
    rc.assert_no_scratch_or_spill(recs, sgpr=True)
    ola, plan = recs[names[0]], recs[names[1]]
    assert plan["lds_static"] == 0 and plan["vgprs"] <= 84, plan
    assert ola["vgprs"] <= 72, ola                            # seven waves a SIMD; the shared core must not cost one
    assert ola["lds_static"] == 256 * 16 + 16 == 4112, ola    # VS_PS_LDS: t, a, periods, gain of 256 marks; the counter
    text = open(HEADER).read()
    assert "#define VS_PS_STAGE 256" in text and "#define VS_PS_BLOCK 256" in text and "#define VS_PS_PER_LANE 8" in text
    assert "#define VS_PS_LDS (VS_PS_STAGE * 16 + 16) /* 4112 bytes, static" in text


def test_no_trap_in_the_listing(tmp_path):
    text = rc.listing(SRC, tmp_path)
    rc.assert_no_trap(text, "vs_ps_plan_kernel")
    rc.assert_no_trap(text, "vs_ps_ola_kernel")
