"""The IAIF analysis's kernel (csrc/vs_iaif.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950
without a GPU): no scratch and no spill, of vector or scalar registers, and no trap instruction in the gfx950 listing --
a frame the kernel cannot analyse says so in its record's status.  Moving the root phase into csrc/vs_lpc_roots.h left
the LPC kernel's registers and LDS as they were."""
import resource_checks as rc

SRC = "vs_iaif.hip"


def test_the_iaif_kernel_uses_no_scratch_and_spills_nothing():
    recs = rc.records(SRC)
    assert any("vs_iaif_kernel" in n for n in recs), list(recs)
    rc.assert_no_scratch_or_spill(recs, sgpr=True)


def test_the_lpc_kernel_kept_its_registers_and_lds():
    """106 VGPRs, 88 SGPRs and 3584 bytes of static LDS before the root phase moved into the shared header, and
    (106, 88, 3584, 0) behind it; with the row of a frame, the recursion, the set store and the record in
    csrc/vs_lpc_frame.h one SGPR fewer, nothing higher, occupancy 4 as before"""
    (r,) = [r for name, r in rc.records("vs_lpc.hip").items() if "vs_lpc_kernel" in name]
    assert (r["vgprs"], r["sgprs"], r["lds_static"], r["scratch"]) == (106, 87, 3584, 0), r
    assert r["occupancy"] == 4, r


def test_no_trap_in_the_listing(tmp_path):
    rc.assert_no_trap(rc.listing(SRC, tmp_path), "vs_iaif_kernel")
