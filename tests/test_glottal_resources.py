"""The glottal parameters' kernel (csrc/vs_glottal.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950
without a GPU): no scratch and no spill, of vector or scalar registers, the ring of two longest periods as its only LDS,
and no trap instruction in the gfx950 listing -- a row or a cycle the kernel cannot measure says so in its status."""
import resource_checks as rc

SRC = "vs_glottal.hip"


def test_the_glottal_kernel_uses_no_scratch_and_spills_nothing():
    recs = rc.records(SRC)
    assert any("vs_glottal_kernel" in n for n in recs), list(recs)
    rc.assert_no_scratch_or_spill(recs, sgpr=True)
    for name, r in recs.items():
        assert r["lds_static"] == 2 * 2 * 2048, (name, r)   # VS_GL_RING int16
        assert r["vgprs"] <= 128, (name, r)                   # four wavefronts per SIMD or more


def test_no_trap_in_the_listing(tmp_path):
    rc.assert_no_trap(rc.listing(SRC, tmp_path), "vs_glottal_kernel")
