#!/usr/bin/env python3
"""Records tests/golden/reference_runs.json.gz from the REFERENCE ITSELF (oracle/_ref, built by oracle/Makefile with
the Philox random() shim, and the reference's vowel_new.c under $VS_REFERENCE_DIR).  TEST INFRASTRUCTURE ONLY.

    make -C oracle VS_REFERENCE_DIR=<the reference's sources> && VS_REFERENCE_DIR=<the same> python3 oracle/gen_reference_runs.py

The tests that compare with the reference read its answers from the recording (oracle/pyoracle.py: reference_run,
reference_pipeline, reference_tables), so that they run where neither the reference's sources nor oracle/_ref exist.
This script makes the recording the way those tests draw their command lines: it runs them with VS_REFERENCE_RECORD
set, which makes every reference run a live one and adds it to the recording -- the CPU tests through pytest, and the
draw of tools/cli_fuzz.py that tests/test_gpu_cli.py makes (only the reference's side is recorded; without a GPU the
drop-in programs' side fails and is not looked at).  Then it adds the digests of the ten A(z) tables of the source
text.  Data only: digests of the reference's outputs and standard output, its .wav headers and draw counts.
"""
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pyoracle as po  # noqa: E402

REF_SOURCE = os.path.join(os.environ.get("VS_REFERENCE_DIR", ""), "vowel_new.c")
TESTS = ["tests/test_parser_vs_reference.py", "tests/test_vowel_files_vs_reference.py",
         "tests/test_host_logic.py::test_wav_header_72_equals_reference_bytes",
         "tests/test_host_logic.py::test_cli_usage_text_equals_reference",
         "tests/test_oracle_golden.py::test_live_reference_agrees_on_a_fresh_case",
         "tests/test_cycle_log_ref.py"]


def tables():
    src = re.sub(r"/\*.*?\*/", "", open(REF_SOURCE).read(), flags=re.S)
    out = {}
    for n in ["A_a", "A_i", "A_u"] + ["A_zz%d" % k for k in range(1, 8)]:
        m = re.search(r"double\s+%s\[22\+1\]\s*=\s*\{(.*?)\};" % n, src, flags=re.S)
        vals = np.array([float(t) for t in m.group(1).replace("\n", " ").split(",")], dtype="<f8")
        out[n] = {"n": int(vals.size), "sha256": hashlib.sha256(vals.tobytes()).hexdigest()}
    return out


def main():
    if not po.have_reference() or not os.path.exists(REF_SOURCE):
        sys.exit("needs oracle/_ref (make -C oracle) and VS_REFERENCE_DIR naming the reference's sources")
    path = po.RUNS_PATH
    if os.path.exists(path):
        os.remove(path)
    env = dict(os.environ, **{po.RECORD_ENV: path})
    subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu"] + TESTS,
                   cwd=ROOT, env=env, check=True)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cli_fuzz.py"), "2026", "10"], cwd=ROOT, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    data = json.loads(gzip.open(path, "rt").read())
    data["tables"] = tables()
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
        z.write(json.dumps(data, sort_keys=True, separators=(",", ":")).encode())
    print("%s: %d runs, %d tables, %d bytes" % (os.path.relpath(path, ROOT), len(data["runs"]), len(data["tables"]),
                                               os.path.getsize(path)))


if __name__ == "__main__":
    main()
