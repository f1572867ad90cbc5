"""The source track's kernel (csrc/vs_strack.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950 without a
GPU): it is found, uses no scratch and spills no register, vector or scalar, stays within 128 vector registers, its
static LDS is the figure vs_strack.h states, and the listing holds no trap.  A resource test only."""
import os

import resource_checks as rc

SRC = "vs_strack.hip"
HEADER = os.path.join(rc.CSRC, "vs_strack.h")


def test_the_strack_kernel_uses_no_scratch_and_spills_nothing():
    recs = rc.records(SRC)
    assert len(recs) == 1 and "vs_strack_kernel" in list(recs)[0], list(recs)
    rc.assert_no_scratch_or_spill(recs, sgpr=True)
    r = list(recs.values())[0]
    assert r["vgprs"] <= 128, r
    assert r["lds_static"] == 2 * 2560 * 2 == 10240, r      # VS_ST_LDS: the cycle and its noise values, int16
    text = open(HEADER).read()
    assert "#define VS_ST_CYCLE_MAX 2560" in text
    assert "#define VS_ST_LDS (2 * VS_ST_CYCLE_MAX * 2) /* 10240 bytes, static */" in text


def test_no_trap_in_the_listing(tmp_path):
    rc.assert_no_trap(rc.listing(SRC, tmp_path), "vs_strack_kernel")
