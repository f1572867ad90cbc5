"""The IAIF analysis's kernel (csrc/vs_iaif.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950
without a GPU): no scratch and no spill, of vector or scalar registers, and no trap instruction in the gfx950 listing --
a frame the kernel cannot analyse says so in its record's status.  Moving the root phase into csrc/vs_lpc_roots.h left
the LPC kernel's registers and LDS as they were."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "voice_synth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _need_hipcc():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc here")


def test_the_iaif_kernel_uses_no_scratch_and_spills_nothing():
    _need_hipcc()
    import kernel_resources
    recs = {r["name"]: r for r in kernel_resources.resources(src=os.path.join(CSRC, "vs_iaif.hip"))}
    assert any("vs_iaif_kernel" in n for n in recs), list(recs)
    for name, r in recs.items():
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)


def test_the_lpc_kernel_kept_its_registers_and_lds():
    """106 VGPRs, 88 SGPRs and 3584 bytes of static LDS before the root phase moved into the shared header"""
    _need_hipcc()
    import kernel_resources
    (r,) = [r for r in kernel_resources.resources(src=os.path.join(CSRC, "vs_lpc.hip")) if "vs_lpc_kernel" in r["name"]]
    assert (r["vgprs"], r["sgprs"], r["lds_static"], r["scratch"]) == (106, 88, 3584, 0), r


def test_no_trap_in_the_listing(tmp_path):
    _need_hipcc()
    import kernel_resources
    out = tmp_path / "vs_iaif.s"
    cmd = [HIPCC] + kernel_resources.hipflags() + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "vs_iaif.hip")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True)
    text = out.read_text()
    assert "vs_iaif_kernel" in text
    assert not re.search(r"^\s*s_trap\b", text, flags=re.M)
