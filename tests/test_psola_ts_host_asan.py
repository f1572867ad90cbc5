"""The device-free half of PSOLA with a time map (csrc/vs_psola_ts_host.c) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/c/test_psola_ts_host_asan.c): the defaults, the refusals of
the sizes, strides and options in their order, the overlap of the input's and the output's rows, the row records and the
scratch, and the arguments of a launch and of the host-buffer call against stand-ins for the record upload, the block
cache and the launcher.  A CPU build: nothing sanitised is loaded into Python.  Needs the HIP runtime's C header only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]


def test_psola_ts_host_c_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_psola_ts_host_asan")
    rocm = os.environ.get("ROCM", "/opt/rocm")
    csrc = os.path.join(ROOT, "voice_synth_amd", "csrc")
    subprocess.run(["gcc", "-std=gnu11"] + SAN + ["-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                                                  os.path.join(ROOT, "tests", "c", "test_psola_ts_host_asan.c"),
                                                  os.path.join(csrc, "vs_psola_ts_host.c"),
                                                  os.path.join(csrc, "vs_psola_host.c"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.strip() == b"ok"
