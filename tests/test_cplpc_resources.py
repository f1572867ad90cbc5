"""The closed-phase covariance LPC's kernel (csrc/vs_cplpc.hip), compiled here with the SHIPPED flags (hipcc cross-compiles
gfx950 without a GPU): no scratch and no spill, of vector or scalar registers, the static LDS the code states (the
covariance triangle is dynamic LDS, sized by the order), registers for four wavefronts per SIMD, and no trap instruction
in the gfx950 listing -- a frame the kernel cannot solve says so in its status."""
import os
import re

import resource_checks as rc

SRC = "vs_cplpc.hip"
HEADER = os.path.join(rc.CSRC, "vs_cplpc.h")


def stated(name):
    return int(re.search(r"#define %s (\d+)" % name, open(HEADER).read()).group(1))


def test_the_cplpc_kernel_uses_no_scratch_and_spills_nothing():
    recs = rc.records(SRC)
    assert any("vs_cplpc_kernel" in n for n in recs), list(recs)
    rc.assert_no_scratch_or_spill(recs, sgpr=True)
    for name, r in recs.items():
        assert r["lds_static"] == stated("VS_CPLPC_LDS_STATIC") == 1752, (name, r)   # chunk, taps, the frame's words
        assert r["vgprs"] <= 128, (name, r)                                             # four wavefronts per SIMD or more


def test_the_stated_lds_plan():
    """the dynamic part, as vs_cplpc.h computes it: (order + 1) rows of an odd stride > order doubles; at order 40 a
    workgroup (one wavefront) takes 15856 bytes of the CU's 160 KiB"""
    text = open(HEADER).read()
    assert "return (order + 2) | 1;" in text and "return (order + 1) * vs_cplpc_stride(order) * 8;" in text
    assert stated("VS_CPLPC_CHUNK") == 256 and stated("VS_CPLPC_THREADS") == 64
    for order, want in ((1, 2 * 3 * 8), (22, 4600), (40, 14104)):
        assert (order + 1) * ((order + 2) | 1) * 8 == want
    assert 14104 + 1752 <= 160 * 1024 // 8


def test_no_trap_in_the_listing(tmp_path):
    rc.assert_no_trap(rc.listing(SRC, tmp_path), "vs_cplpc_kernel")
