"""The glottal parameters' kernel (csrc/vs_glottal.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950
without a GPU): no scratch and no spill, of vector or scalar registers, the ring of two longest periods as its only LDS,
and no trap instruction in the gfx950 listing -- a row or a cycle the kernel cannot measure says so in its status."""
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


def test_the_glottal_kernel_uses_no_scratch_and_spills_nothing():
    _need_hipcc()
    import kernel_resources
    recs = {r["name"]: r for r in kernel_resources.resources(src=os.path.join(CSRC, "vs_glottal.hip"))}
    assert any("vs_glottal_kernel" in n for n in recs), list(recs)
    for name, r in recs.items():
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)
        assert r["lds_static"] == 2 * 2 * 2048, (name, r)   # VS_GL_RING int16
        assert r["vgprs"] <= 128, (name, r)                   # four wavefronts per SIMD or more


def test_no_trap_in_the_listing(tmp_path):
    _need_hipcc()
    import kernel_resources
    out = tmp_path / "vs_glottal.s"
    cmd = [HIPCC] + kernel_resources.hipflags() + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "vs_glottal.hip")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True)
    text = out.read_text()
    assert "vs_glottal_kernel" in text
    assert not re.search(r"^\s*s_trap\b", text, flags=re.M)
