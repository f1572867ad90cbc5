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
import hostile_signals as hs  # noqa: E402

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
    with engine.scope() as dev:
        plan = dev.plan(lanes, ns)
        pcm_d = dev.room(n * pitch * 2)
        out_d = dev.room(n * vs.ACOUSTIC_DTYPE.itemsize)
        mk_d = dev.room(n * 100 * 4)
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        engine.measure_dev(pcm_d, pitch, n, ns, fs, out_d, marks_ptr=mk_d, marks_pitch=100)
        assert plan.status() == 0
        got = engine.dev_download(out_d, (n,), vs.ACOUSTIC_DTYPE)
        gm = engine.dev_download(mk_d, (n, 100), np.int32)
        pcm = engine.dev_download(pcm_d, (n, pitch))[:, :ns]
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


# ---- signals the project does not synthesise (tests/hostile_signals.py; tests/test_hostile_signals_ref.py shows on the
# CPU which paths of the two kernels each case takes) ----

@pytest.mark.parametrize("polarity", [1, -1])
@pytest.mark.parametrize("case", hs.ACOUSTIC_CASES, ids=lambda c: "%dHz" % c[0])
def test_hostile_signals_equal_the_restatement(engine, case, polarity):
    """noise, silence, DC, full-scale squares and alternations, tones outside the bounds, period jumps: the 96 kHz case
    needs 64 000 bytes of LDS (the opt-in above 48 KB), it and the 44.1 kHz case more than 256 lag groups (a second pass
    of the group loop), the 16 kHz case 3 and the 8 kHz case 25 k segments"""
    fs, n, f0_min, f0_max = case
    names, pcm = hs.matrix(hs.bank(fs, n, 0))
    got, gm = engine.measure(pcm, fs, f0_min=f0_min, f0_max=f0_max, polarity=polarity, marks=1024)
    want, wm = ar.measure(pcm, fs, f0_min=f0_min, f0_max=f0_max, polarity=polarity, marks=1024)
    assert want["n_periods"].max() < 1024
    assert_same(got, want, gm, wm)
    for k in hs.UNVOICED_ROWS:
        i = names.index(k)
        assert got["status"][i] == vs.VS_AC_UNVOICED and got["p0"][i] == 0 and np.all(gm[i] == -1), k
    for k in hs.ZERO_AMPLITUDE_ROWS:
        i = names.index(k)
        assert got["status"][i] == vs.VS_AC_ZERO_AMPLITUDE and np.isnan(got["shimmer_local"][i]), k
        assert not np.isnan(got["jitter_local"][i]), k
    assert (got["status"] == 0).any()
    assert got["p0"][names.index("constant")] == ar.lag_bounds(fs, f0_min, f0_max)[0]   # no local peak of r
    if polarity == -1:   # -32768 is a marked peak, 32768 after the sign change
        i = names.index("alternating")
        assert (pcm[i, gm[i, 1:got["n_periods"][i] + 1]] == -32768).all()


def _pulse_train(periods, amps, n, start, w):
    """triangular pulses 2*w - 1 samples wide on a zero baseline (as in tests/test_acoustic_ref.py)"""
    x = np.zeros(n, dtype=np.int16)
    pos = start
    for k, a in enumerate(amps):
        if pos >= n:
            break
        for j in range(-w + 1, w):
            if 0 <= pos + j < n:
                x[pos + j] = a * (w - abs(j)) // w
        if k < len(periods):
            pos += periods[k]
    return x


def _mixed_rate_rows(f0_min, f0_max, extra=()):
    """rows of the banks at 8, 16, 44.1 and 96 kHz, the rates alternating from row to row, each rate with a row one
    sample too short and a row of the shortest measured length; extra: (row, fs) pairs appended"""
    picks = ("noise_full", "chirp", "jump_320", "zeros", "alternating", "sine_150_noise")
    rows = []
    for k in range(len(picks) + 2):
        for fs, n in ((8000, 3000), (16000, 5000), (44100, 9000), (96000, 20000)):
            b = hs.bank(fs, n, 1)
            tmax = ar.lag_bounds(fs, f0_min, f0_max)[1]
            assert n >= 3 * tmax + 2
            if k < len(picks):
                rows.append((b[picks[k]], fs, n - 11 * k))
            else:
                rows.append((b["am_sine_120"], fs, 3 * tmax + 1 + (k - len(picks))))
    rows += [(x, fs, len(x)) for x, fs in extra]
    width = max(len(r[0]) for r in rows)
    pcm = np.zeros((len(rows), width), dtype=np.int16)
    for i, (x, _, _) in enumerate(rows):
        pcm[i, :len(x)] = x
    return pcm, np.array([r[1] for r in rows], dtype=np.int32), np.array([r[2] for r in rows], dtype=np.int32)


def test_mixed_rates_up_to_96_khz_in_one_call(engine):
    """bounds 47..500 Hz: the 96 kHz rows set the LDS size of the launch (64 000 bytes), and the rows of the other rates,
    which ask for as little as 12 KB, run inside it with their own offsets.  One call cannot hold the 260-sample row of
    tests/test_acoustic_ref.py (4 periods: no PPQ5 / APQ5), which needs f0_min = 200 Hz to be long enough: it goes into
    a second mixed call with that bound."""
    four = _pulse_train([50, 52, 49, 51, 50], [8000, 7000, 7400, 6900, 7100, 7000], 260, start=5, w=8)
    for f0_min, extra in ((47.0, ()), (200.0, ((four, 16000),))):
        pcm, fs, lengths = _mixed_rate_rows(f0_min, 500.0, extra)
        got, gm = engine.measure(pcm, fs, f0_min=f0_min, lengths=lengths, marks=64)
        want, wm = ar.measure(pcm, fs, f0_min=f0_min, lengths=lengths, marks=64)
        assert_same(got, want, gm, wm)
        for i in range(len(fs)):
            alone, am = engine.measure(pcm[i:i + 1, :lengths[i]], fs[i], f0_min=f0_min, marks=64)
            assert_same(got[i:i + 1], alone, gm[i:i + 1], am)
        tmax = np.array([ar.lag_bounds(int(r), f0_min, 500.0)[1] for r in fs])
        short = lengths == 3 * tmax + 1
        assert short.sum() == 4 and (got["status"][short] == vs.VS_AC_TOO_SHORT).all()
        shortest = lengths == 3 * tmax + 2
        assert shortest.sum() == 4 and (got["status"][shortest] & vs.VS_AC_TOO_SHORT == 0).all()
        assert (got["first_mark"][shortest] >= 0).all()
        if extra:
            assert got["status"][-1] == 0 and 3 <= got["n_periods"][-1] < 5
            assert np.isnan(got["jitter_ppq5"][-1]) and np.isnan(got["shimmer_apq5"][-1])
            assert not np.isnan(got["jitter_rap"][-1]) and not np.isnan(got["shimmer_apq3"][-1])


def test_marks_kernel_batch_geometry(engine):
    """70 rows (the last workgroup has 6), rows that are finished before the walk starts next to live ones in every
    wavefront, a pitch above n_samples, an n_samples that is no multiple of the 128-sample tile, fewer mark slots than
    marks, and sentinels around everything the call must not write"""
    fs, n, rows, mp = 16000, 8000, 70, 8
    ns, pitch = n - 61, n - 61 + 37
    assert ns % 128 and (rows - 64) == 6
    b = hs.bank(fs, n, 2)
    live = [k for k in b if k not in hs.UNVOICED_ROWS]
    loud = np.where(np.arange(pitch) % 7 < 3, 32767, -32768).astype(np.int16)
    buf = np.tile(loud, (rows + 1, 1))          # what no row covers is a loud square wave: it must not be read
    lengths = np.zeros(rows, dtype=np.int32)
    kind = np.arange(rows) % 3                  # 0: too short, 1: unvoiced, 2: live
    for i in range(rows):
        name = live[(i // 3) % len(live)]
        lengths[i] = (3 * 320 + 1, ns - 5 * (i % 4), ns - 13 * (i % 5))[kind[i]]
        buf[i, :lengths[i]] = (b[name], b["zeros"], b[name])[kind[i]][:lengths[i]]
    want, wm = ar.measure(buf[:rows, :ns], fs, lengths=lengths, marks=mp)
    assert (want["status"][kind == 0] == ar.AC_TOO_SHORT).all() and (want["status"][kind == 1] == ar.AC_UNVOICED).all()
    assert (want["n_periods"][kind == 2] + 1 > mp).all()      # marks_pitch is smaller than every live row's mark count
    rec = vs.ACOUSTIC_DTYPE.itemsize
    with engine.scope() as dev:
        pcm_d, out_d, out2_d, mk_d = (dev.room(v) for v in (buf.nbytes, (rows + 1) * rec, (rows + 1) * rec,
                                                            (rows + 1) * mp * 4))
        engine.dev_upload(pcm_d, buf)
        for p, v in ((out_d, (rows + 1) * rec), (out2_d, (rows + 1) * rec), (mk_d, (rows + 1) * mp * 4)):
            engine.dev_upload(p, np.full(v, 0x5A, dtype=np.uint8))
        engine.measure_dev(pcm_d, pitch, rows, ns, fs, out_d, lengths=lengths, marks_ptr=mk_d, marks_pitch=mp)
        engine.measure_dev(pcm_d, pitch, rows, ns, fs, out2_d, lengths=lengths, marks_ptr=None)
        engine.synchronize()
        got = engine.dev_download(out_d, (rows + 1,), vs.ACOUSTIC_DTYPE)
        got2 = engine.dev_download(out2_d, (rows + 1,), vs.ACOUSTIC_DTYPE)
        gm = engine.dev_download(mk_d, (rows + 1, mp), np.int32)
    sentinel = 0x5A5A5A5A
    walked = kind == 2
    assert_same(got[:rows], want, gm[:rows][walked], wm[walked])
    assert (gm[:rows][~walked] == sentinel).all() and (gm[rows] == sentinel).all()
    assert (got[rows:].view(np.uint8) == 0x5A).all() and (got2[rows:].view(np.uint8) == 0x5A).all()
    assert got[:rows].tobytes() == got2[:rows].tobytes()


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
