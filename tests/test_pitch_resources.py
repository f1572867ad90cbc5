"""The pitch track's kernels (csrc/vs_pitch.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950
without a GPU): no scratch and no spill, the static LDS the code states (the candidate kernel's is dynamic, sized by the
lag range), and at most 128 VGPRs.  A resource test only."""
import os
import re

import resource_checks as rc

SRC = "vs_pitch.hip"
HEADER = os.path.join(rc.CSRC, "vs_pitch.h")


def test_the_pitch_kernels_use_no_scratch_and_spill_nothing():
    recs = rc.records(SRC)
    cand = [r for n, r in recs.items() if "vs_pt_cand_kernel" in n]
    path = [r for n, r in recs.items() if "vs_pt_path_kernel" in n]
    assert len(cand) == 1 and len(path) == 1 and len(recs) == 2, list(recs)
    rc.assert_no_scratch_or_spill(recs, sgpr=True)
    for name, r in recs.items():
        assert r["vgprs"] <= 128, (name, r)
    assert cand[0]["lds_static"] == 0, cand[0]
    assert path[0]["lds_static"] == (2048 + 1) * 4, path[0]          # VS_PT_PATH_LDS: the Lg table
    assert "#define VS_PT_PATH_LDS ((VS_AC_MAX_LAG + 1) * 4)" in open(HEADER).read()


def test_the_stated_lds_plan():
    """vs_pt_lds_doubles as vs_pitch.h computes it, at the two shapes its comment names, and within a CU's 160 KiB"""
    text = open(HEADER).read() + open(os.path.join(rc.CSRC, "vs_acoustic.h")).read()
    assert "return ((3 * tmax + 2 + 4) + 3) & ~3;" in text and "return tmax + 3 - tmin;" in text

    def doubles(tmin, tmax):
        nl = tmax + 3 - tmin
        G = (nl + 3) // 4
        S = 1 if G >= 256 else 256 // G
        e = (nl + 3) & ~3
        return (((3 * tmax + 2 + 4) + 3) & ~3) + 4 * G * S + e + 16 + e // 2

    assert doubles(2, 2048) * 8 == 90384 <= 160 * 1024
    assert doubles(32, 320) * 8 == 18384
    assert re.search(r"90384 bytes", text) and re.search(r"18384 bytes", text)
