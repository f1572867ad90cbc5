"""The guided marks' kernels (csrc/vs_guided.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950
without a GPU): both are found, neither uses scratch or spills a vector register (the walk kernel keeps scalars in lanes
of a vector register, as the marks kernel it is modelled on does, which costs no memory traffic), the static LDS is the
figure vs_guided.h states, and the listing holds no trap.  A resource test only."""
import os

import resource_checks as rc

SRC = "vs_guided.hip"
HEADER = os.path.join(rc.CSRC, "vs_guided.h")


def test_the_guided_kernels_use_no_scratch_and_spill_nothing():
    recs = rc.records(SRC)
    plan = [r for n, r in recs.items() if "vs_mg_plan_kernel" in n]
    walk = [r for n, r in recs.items() if "vs_mg_walk_kernel" in n]
    assert len(plan) == 1 and len(walk) == 1 and len(recs) == 2, list(recs)
    rc.assert_no_scratch_or_spill(recs)
    rc.assert_no_scratch_or_spill({"plan": plan[0]}, sgpr=True)
    assert plan[0]["lds_static"] == 0, plan[0]
    assert walk[0]["lds_static"] == 64 * (128 + 2) * 2 == 16640, walk[0]      # VS_MG_WALK_LDS
    text = open(HEADER).read()
    assert "#define VS_MG_TILE 128" in text and "#define VS_MG_PAD 2" in text
    assert "#define VS_MG_WALK_LDS (64 * (VS_MG_TILE + VS_MG_PAD) * 2) /* 16640 bytes */" in text
    assert walk[0]["vgprs"] <= 256 and plan[0]["vgprs"] <= 64, (walk[0], plan[0])


def test_no_trap_in_the_listing(tmp_path):
    rc.assert_no_trap(rc.listing(SRC, tmp_path), "vs_mg_plan_kernel", "vs_mg_walk_kernel")
