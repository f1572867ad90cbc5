"""The inverse filter's kernels (csrc/vs_inverse.hip), compiled here with the SHIPPED flags (hipcc cross-compiles gfx950
without a GPU): no scratch and no spill in any instantiation (the taps and the window of u are registers with static
indices, the reflection coefficients are in LDS), and no trap instruction in the gfx950 listing -- a row without a usable
set says so in its status record."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SRC = os.path.join(ROOT, "voice_synth_amd", "csrc", "vs_inverse.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _need_hipcc():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc here")


def test_the_inverse_kernels_use_no_scratch():
    _need_hipcc()
    import kernel_resources
    recs = {r["name"]: r for r in kernel_resources.resources(src=SRC)}
    kernels = [n for n in recs if "vs_inverse_kernel" in n]
    assert len(kernels) == 8, list(recs)         # arithmetic x window class x mode
    for name, r in recs.items():
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (name, r)


def test_no_trap_in_the_listing(tmp_path):
    _need_hipcc()
    import kernel_resources
    out = tmp_path / "vs_inverse.s"
    cmd = [HIPCC] + kernel_resources.hipflags() + ["-S", "--cuda-device-only", "-o", str(out), SRC]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True)
    text = out.read_text()
    assert "vs_inverse_kernel" in text
    assert not re.search(r"^\s*s_trap\b", text, flags=re.M)
