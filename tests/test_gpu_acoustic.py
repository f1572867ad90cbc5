"""The acoustic measurement on the device (vs_measure / vs_measure_launch, bin/acoustic) against its numpy restatement
(tests/acoustic_ref.py): integer fields and marks bit for bit, the doubles equal (shimmer_db and hnr_db, which go
through log10 on both sides, within 1e-9 relative); and against the truth the synthesis logs for every cycle."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acoustic_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(vs.__file__), "bin")
EXACT = ("f0_hz", "jitter_local", "jitter_abs_s", "jitter_rap", "jitter_ppq5", "shimmer_local", "shimmer_apq3",
         "shimmer_apq5")
INTS = ("p0", "n_periods", "first_mark", "status")


def assert_same(got, want, gm=None, wm=None):
    for f in INTS:
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:8])
    for f in EXACT:
        assert np.array_equal(got[f], want[f], equal_nan=True), (f, np.nonzero(~((got[f] == want[f]) |
                                                                                   (np.isnan(got[f]) & np.isnan(want[f]))))[0][:8])
    for f in ("shimmer_db", "hnr_db"):
        g, w = got[f], want[f]
        assert np.array_equal(np.isnan(g), np.isnan(w)), f
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= 1e-9 * np.abs(w[ok])), f
    if gm is not None:
        assert np.array_equal(gm, wm)


def _config_pcm(engine, index, n):
    specs, fs, dur, _ = configs.config_specs(index, n)
    lanes, d = vs.lanes_from_specs(specs)
    return engine.synth(lanes, vs.num_samples(fs, d)), fs


@pytest.mark.parametrize("index,n", [(2, 256), (3, 256), (5, 256)])
def test_parity_with_the_restatement_on_config_batches(engine, index, n):
    pcm, fs = _config_pcm(engine, index, n)
    got, gm = engine.measure(pcm, fs, marks=160)
    want, wm = ar.measure(pcm, fs, marks=160)
    assert (got["status"] == 0).mean() > 0.8
    assert_same(got, want, gm, wm)


def test_parity_on_flows_and_minima(engine):
    lanes = [vs.lane_from_cli(["-d", "1", "-j", "2", "-s", "3", "-g", "300", "-f", "%d" % (90 + 3 * k)], ["-v", "a"], 50 + k)[0]
             for k in range(64)]
    flow = engine.source(lanes, vs.num_samples(22050, 1.0))
    for pol in (1, -1):
        got, gm = engine.measure(flow, 22050, polarity=pol, marks=200)
        want, wm = ar.measure(flow, 22050, polarity=pol, marks=200)
        assert_same(got, want, gm, wm)


def _flow_lane(fs, f0, jitter, seed):
    fa = (["-r", str(fs)] if fs != 22050 else []) + ["-d", "1", "-f", str(f0), "-g", "%.2f" % (f0 * 125 / 120 + 1),
                                                       "-j", str(jitter)]
    lane, _ = vs.lane_from_cli(fa, ["-v", "a"], seed)
    lane.DC = 0.0
    lane.Kvar = 0.0
    return lane


def test_marks_reproduce_the_cycle_log_on_the_device(engine):
    """vs_source with its cycle log: the differences of the measured marks are the logged periods, exactly"""
    for fs in (22050, 44100):
        lanes = [_flow_lane(fs, 90 + (7 * k) % 31, (0.5, 1, 2, 5)[k % 4], 700 + k) for k in range(32)]
        flow, recs, ncyc = engine.source(lanes, vs.num_samples(fs, 1.0), log_cycles=200)
        got, marks = engine.measure(flow, fs, marks=200)
        for i in range(len(lanes)):
            K = int(got["n_periods"][i])
            assert K >= 60 and got["status"][i] == 0
            T = np.diff(marks[i, :K + 1])
            assert np.array_equal(T, recs["T"][i, :K]), (fs, i)


def test_device_chained_measurement_equals_the_host_path(engine):
    """Plan.launch(VS_KIND_SYNTH) into device memory, then measure_dev on the same stream: the PCM never leaves the
    device, and the result is that of vs_measure on the downloaded PCM"""
    n = 16384
    specs, fs, dur, _ = configs.config_specs(3, n)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    plan = engine.plan(lanes, ns)
    pcm_d = engine.dev_alloc(n * pitch * 2)
    out_d = engine.dev_alloc(n * vs.ACOUSTIC_DTYPE.itemsize)
    mk_d = engine.dev_alloc(n * 100 * 4)
    try:
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        engine.measure_dev(pcm_d, pitch, n, ns, fs, out_d, marks_ptr=mk_d, marks_pitch=100)
        assert plan.status() == 0
        got = engine.dev_download(out_d, (n,), vs.ACOUSTIC_DTYPE)
        gm = engine.dev_download(mk_d, (n, 100), np.int32)
        pcm = engine.dev_download(pcm_d, (n, pitch))[:, :ns]
    finally:
        plan.close()
        for p in (pcm_d, out_d, mk_d):
            engine.dev_free(p)
    want, wm = engine.measure(pcm, fs, marks=100)
    assert_same(got, want)
    K = np.minimum(want["n_periods"] + 1, 100)
    for i in range(n):
        assert np.array_equal(gm[i, :K[i]], wm[i, :K[i]])
    ref, rm = ar.measure(pcm[:64], fs, marks=100)
    assert_same(got[:64], ref)


def test_ragged_rows_and_mixed_rates_in_one_call(engine):
    l22 = [_flow_lane(22050, 100 + k, 1, 900 + k) for k in range(8)]
    l44 = [_flow_lane(44100, 100 + k, 2, 950 + k) for k in range(8)]
    f22 = engine.source(l22, vs.num_samples(22050, 1.0))
    f44 = engine.source(l44, vs.num_samples(44100, 1.0))
    n = f44.shape[1]
    pcm = np.zeros((16, n), dtype=np.int16)
    fs = np.zeros(16, dtype=np.int32)
    lengths = np.zeros(16, dtype=np.int32)
    short = {3: 3 * 441 + 1, 11: 3 * 882 + 1}   # one sample short of 3*tmax + 2
    for k in range(8):
        for i, f, r in ((2 * k, f22[k], 22050), (2 * k + 1, f44[k], 44100)):
            L = len(f) - 37 * k
            pcm[i, :L] = f[:L]
            fs[i], lengths[i] = r, short.get(i, L)
    got, gm = engine.measure(pcm, fs, lengths=lengths, marks=220)
    for i in range(16):
        alone, am = engine.measure(pcm[i:i + 1, :lengths[i]], fs[i], marks=220)
        assert_same(got[i:i + 1], alone, gm[i:i + 1], am)
        if i in short:
            assert got["status"][i] == vs.VS_AC_TOO_SHORT and np.isnan(got["f0_hz"][i]) and got["first_mark"][i] == -1
            assert np.all(gm[i] == -1)
        else:
            assert got["status"][i] == 0
    want, wm = ar.measure(pcm, fs, lengths=lengths, marks=220)
    assert_same(got, want, gm, wm)


def test_bad_arguments_are_refused(engine):
    pcm = np.zeros((2, 4000), dtype=np.int16)
    for kw in ({"f0_min": 5}, {"f0_max": 10000}, {"f0_min": 600}, {"polarity": 0}):
        with pytest.raises(vs.VsError):
            engine.measure(pcm, 16000, **kw)
    with pytest.raises(vs.VsError):
        engine.measure(pcm, 16000, lengths=[4000, 4001])


# ---- bin/acoustic ----

def _wav(path, fs, payload, header=44, tag=1, bits=16):
    data = payload.tobytes() if hasattr(payload, "tobytes") else payload
    if header == 44:
        h = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, tag, 1, fs,
                        fs * bits // 8, bits // 8, bits, b"data", len(data))
    else:
        h = vs_header72(fs, len(data), tag, bits)
    open(path, "wb").write(h + data)


def vs_header72(fs, nbytes, tag, bits):
    """the LP64 layout, as vs_wav_header_write lays it out (the program reads the payload up to the end of the file)"""
    import ctypes as C
    buf = (C.c_ubyte * 72)()
    assert vs.load().vs_wav_header_write(buf, 72, fs, nbytes / 2.0 / fs) == 72
    assert tag == 1 and bits == 16
    return bytes(buf)


def _pipeline(tmp_path, name, fa, va, seed, header=44):
    env = dict(os.environ, VS_SEED=str(seed), VS_WAV_HEADER=str(header))
    g = name + "_g.wav"
    subprocess.run([os.path.join(BIN, "flowgen_shimmer"), "-o", g] + fa, cwd=tmp_path, env=env, check=True,
                   capture_output=True)
    subprocess.run([os.path.join(BIN, "vowel"), "-i", g, "-o", name + ".wav"] + va, cwd=tmp_path, env=env, check=True,
                   capture_output=True)
    return g, name + ".wav"


def _payload(path, header):
    return np.frombuffer(open(path, "rb").read()[header:], dtype=np.int16)


def test_cli_lines_equal_the_restatement(tmp_path):
    files = []
    for k, (fa, va) in enumerate([(["-d", "1", "-j", "1", "-s", "5.76"], ["-v", "a"]),
                                  (["-r", "44100", "-d", "1", "-j", "2", "-f", "100"], ["-v", "i"]),
                                  (["-d", "1", "-f", "150", "-g", "160"], ["-v", "u", "-n", "20"])]):
        files += _pipeline(tmp_path, "s%d" % k, fa, va, 11 + k)
    r = subprocess.run([os.path.join(BIN, "acoustic")] + files, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("#") and len(lines) == 1 + len(files)
    for f, line in zip(files, lines[1:]):
        x = _payload(tmp_path / f, 44)
        fs = struct.unpack("<I", open(tmp_path / f, "rb").read()[24:28])[0]
        rec, _ = ar.measure_row(x, fs)
        assert line == ar.format_line(f, rec)
    # the same data behind the 72-byte header: the same line
    x = _payload(tmp_path / files[1], 44)
    _wav(tmp_path / "h72.wav", 22050, x, header=72)
    _wav(tmp_path / "h44.wav", 22050, x, header=44)
    r = subprocess.run([os.path.join(BIN, "acoustic"), "h44.wav", "h72.wav"], cwd=tmp_path, capture_output=True,
                       text=True)
    assert r.returncode == 0
    a, b = r.stdout.splitlines()[1:]
    assert a.split()[1:] == b.split()[1:] and a.split()[0] == "h44.wav"


def test_cli_marks_and_bad_files(tmp_path):
    _, good = _pipeline(tmp_path, "g", ["-d", "1", "-j", "1"], ["-v", "a"], 5)
    x = _payload(tmp_path / good, 44)
    _wav(tmp_path / "bits8.wav", 22050, x[:4000].astype(np.uint8), bits=8)
    _wav(tmp_path / "tag3.wav", 22050, x.astype(np.float32), tag=3, bits=32)
    open(tmp_path / "trunc.wav", "wb").write(open(tmp_path / good, "rb").read()[:30])
    r = subprocess.run([os.path.join(BIN, "acoustic"), "-m", "bits8.wav", good, "tag3.wav", "trunc.wav"],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2
    for f in ("bits8.wav", "tag3.wav", "trunc.wav"):
        assert f in r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 3 and lines[1].split()[0] == good
    rec, m = ar.measure_row(x, 22050, marks_pitch=10 ** 6)
    assert lines[1] == ar.format_line(good, rec)
    assert lines[2] == "# marks %s: %s" % (good, " ".join(str(v) for v in m))
