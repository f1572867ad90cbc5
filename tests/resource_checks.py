"""What the *_resources tests share: the kernels of one .hip file compiled here with the SHIPPED flags (hipcc cross-compiles
gfx950 without a GPU; tools/kernel_resources.py), their resource records and their gfx950 listing."""
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


def need_hipcc():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc here")


def records(src=None):
    """the compiler's resource record of every kernel of csrc/<src> (default: every file of synthesis kernels), by name"""
    need_hipcc()
    import kernel_resources
    kw = {} if src is None else dict(src=os.path.join(CSRC, src))
    return {r["name"]: r for r in kernel_resources.resources(**kw)}


def listing(src, tmp_path):
    """the gfx950 assembly of csrc/<src>"""
    need_hipcc()
    import kernel_resources
    out = tmp_path / (os.path.splitext(src)[0] + ".s")
    cmd = [HIPCC] + kernel_resources.hipflags() + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, src)]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True)
    return out.read_text()


def assert_no_scratch_or_spill(recs, sgpr=False):
    """no scratch and no vector register spilled in any of the kernels; sgpr: no scalar register spilled either (into
    lanes of a vector register, which costs no memory traffic: the acoustic, track and inverse kernels do it)"""
    for name, r in recs.items():
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (name, r)
        assert not sgpr or r.get("sgpr_spill", 0) == 0, (name, r)


def assert_no_trap(text, *symbols):
    """the listing holds the kernels named and no trap instruction"""
    for symbol in symbols:
        assert symbol in text, symbol
    assert not re.search(r"^\s*s_trap\b", text, flags=re.M)
