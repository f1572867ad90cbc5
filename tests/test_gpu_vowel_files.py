"""bin/vowel on files it did not write (tests/test_vowel_files_vs_reference.py builds them and holds the compiled
reference's recorded runs on them to the oracle): the same return code, standard output, header and payload as the
reference's run -- on the 72-byte files against the recording itself, on the 44-byte files against what follows from
it (the same text, the same payload behind the file's own header)."""
import os
import subprocess
import sys

import pytest

import voice_synth_amd as vs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vowel_files_vs_reference as files  # noqa: E402

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(vs.__file__), "bin")


@pytest.mark.parametrize("layout", [72, 44])
@pytest.mark.parametrize("name", list(files.FILES))
def test_vowel_on_foreign_files_equals_the_reference(tmp_path, name, layout):
    ref = files.recorded(name)
    (tmp_path / "in.wav").write_bytes(files.wav_file(name, layout))
    env = dict(os.environ, VS_SEED=str(files.SEED), VS_WAV_HEADER=str(layout))
    r = subprocess.run([os.path.join(BIN, "vowel")] + files.argv(name), cwd=tmp_path, env=env, capture_output=True,
                       stdin=subprocess.DEVNULL, timeout=60)
    assert r.returncode == ref["rc"], r.stderr
    assert po.digest(r.stdout) == ref["stdout_sha256"], r.stdout
    written = sorted(p.name for p in tmp_path.iterdir() if p.name != "in.wav")
    assert written == sorted(ref["files"])
    if not written:
        return
    o = ref["files"]["o.wav"]
    raw = (tmp_path / "o.wav").read_bytes()
    assert raw[:layout] == files.wav_file(name, layout)[:layout]          # the input's header, verbatim
    if layout == 72:
        assert raw[:72].hex() == o["header"]
    assert len(raw) == layout + 2 * o["n"] and po.digest(raw[layout:]) == o["payload_sha256"]
