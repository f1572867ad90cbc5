"""The two kernels of PSOLA with a time map (csrc/vs_psola_ts.hip), compiled here with the SHIPPED flags (hipcc
cross-compiles gfx950 without a GPU): both are found, neither uses scratch nor spills a register, vector or scalar, the
overlap-add kernel's static LDS is the figure vs_psola_ts.h and include/voice_synth.h state and the plan kernel has none,
and the listing holds no trap.  A resource test only."""
import os

import resource_checks as rc

SRC = "vs_psola_ts.hip"
HEADER = os.path.join(rc.CSRC, "vs_psola_ts.h")
PUBLIC = os.path.join(rc.ROOT, "include", "voice_synth.h")


def test_the_psola_ts_kernels_use_no_scratch_and_spill_nothing():
    recs = rc.records(SRC)
    names = sorted(recs)
    assert len(names) == 2 and "vs_pt_ola_kernel" in names[0] and "vs_pt_plan_kernel" in names[1], names
    rc.assert_no_scratch_or_spill(recs, sgpr=True)
    ola, plan = recs[names[0]], recs[names[1]]
    assert plan["lds_static"] == 0 and plan["vgprs"] <= 114, plan
    assert ola["vgprs"] <= 64, ola                            # eight waves a SIMD, one more than PSOLA's instantiation of the core
    assert ola["lds_static"] == 256 * 20 + 16 == 5136, ola    # VS_PT_LDS: t, both marks, periods, gain of 256 marks; the counter
    text = open(HEADER).read()
    assert "#define VS_PT_LDS (VS_PS_STAGE * 20 + 16) /* 5136 bytes, static" in text
    assert "#define VS_PS_STAGE 256" in open(os.path.join(rc.CSRC, "vs_psola.h")).read()
    assert "The overlap-add kernel has 5136 bytes of\n * static LDS" in open(PUBLIC).read()


def test_no_trap_in_the_listing(tmp_path):
    text = rc.listing(SRC, tmp_path)
    rc.assert_no_trap(text, "vs_pt_plan_kernel")
    rc.assert_no_trap(text, "vs_pt_ola_kernel")
