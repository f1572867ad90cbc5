"""The guided marks on the device (csrc/vs_guided.hip) against their numpy restatement (tests/guided_ref.py): integer
fields, marks, counts and segment records bit for bit, the doubles equal (shimmer_db and hnr_db, which go through log10 on
both sides, within 1e-9 relative: the allowance tests/test_gpu_acoustic.py gives them), every output inside a guard band,
at the smallest shapes that can go wrong.  The frames the walk is steered by are the device's pitch track
(tests/test_gpu_pitch.py holds that to its restatement) or fabricated records."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acoustic_ref as ar  # noqa: E402
import gpu_support as gs  # noqa: E402
import guided_ref as gr  # noqa: E402
import hostile_signals as hs  # noqa: E402
import pitch_ref as pr  # noqa: E402
import pitch_signals as ps  # noqa: E402

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voice_synth_amd", "bin")
S32 = 0x5A5A5A5A
S64 = 0x5A5A5A5A5A5A5A5A
EXACT = ("f0_hz", "jitter_local", "jitter_abs_s", "jitter_rap", "jitter_ppq5", "shimmer_local", "shimmer_apq3",
         "shimmer_apq5")
INTS = ("p0", "n_periods", "first_mark", "status")
PITCH_KEYS = ("f0_min", "f0_max", "hop_s")


@pytest.fixture(scope="module")
def eng():
    e = vs.Engine(0)
    yield e
    e.close()


def assert_same(got, want):
    for f in INTS:
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:8], got[f][:8], want[f][:8])
    for f in EXACT:
        assert np.array_equal(got[f], want[f], equal_nan=True), (f, got[f][:8], want[f][:8])
    for f in ("shimmer_db", "hnr_db"):
        g, w = got[f], want[f]
        assert np.array_equal(np.isnan(g), np.isnan(w)), f
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= 1e-9 * np.abs(w[ok])), f


def track_of(eng, pcm, fs, lengths, opts):
    frames, _ = eng.pitch(pcm, fs, lengths=lengths, **{k: v for k, v in opts.items() if k in PITCH_KEYS})
    return frames


def check_dev(eng, pcm, fs, lengths=None, frames=None, marks=400, segs=6, pad=5, **opts):
    """vs_guided_launch on device pointers: the PCM staged at a pitch above its length inside a pad that is not silence,
    every output inside a sentinel band (marks_pitch and seg_pitch are both the row stride and the number of slots).  Everything equals the restatement's, the
    sentinel where the definition writes nothing included.  Returns the restatement's (records, marks, rec, segs)."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    n, ns = pcm.shape
    if frames is None:
        frames = track_of(eng, pcm, fs, lengths, opts)
    frames = np.ascontiguousarray(frames, dtype=vs.PITCH_FRAME_DTYPE)
    fp = frames.shape[1]
    want, wm, wrec, wseg = gr.guided(pcm, fs, frames, lengths, marks=marks, segs=segs or 1,
                                     marks_fill=np.full((n, marks), S32, np.int32),
                                     segs_fill=np.full((n, (segs or 1) * 4), S32, np.int32).view(gr.SEG_DTYPE), **opts)
    pitch = ns + pad
    with eng.scope() as dev:
        src = dev.put(gs.staged_input(pcm, pitch)) + 2 * gs.GUARD
        d_fr = dev.put(frames)
        g_out = gs.GuardedRows(n, 12, 12, 0, S64, np.int64).on(dev)
        g_mk = gs.GuardedRows(n, marks, marks, 0, S32, np.int32).on(dev)
        g_rec = gs.GuardedRows(n, 4, 4, 0, S32, np.int32).on(dev)
        g_seg = gs.GuardedRows(n, 4 * max(segs, 1), 4 * max(segs, 1), 0, S32, np.int32).on(dev)
        eng.measure_guided_dev(src, pitch, n, ns, fs, d_fr, fp, g_out.first(12), g_rec.first(4), g_mk.first(marks),
                               marks, g_seg.first(4 * segs) if segs else None, segs, lengths=lengths, **opts)
        eng.synchronize()
        out = np.ascontiguousarray(g_out.rows_back(12)).view(vs.ACOUSTIC_DTYPE).reshape(n)
        mk = g_mk.rows_back(marks)
        rec = np.ascontiguousarray(g_rec.rows_back(4)).view(vs.GUIDED_REC_DTYPE).reshape(n)
        seg = g_seg.rows_back(4 * max(segs, 1))
        assert np.array_equal(dev.get(d_fr, frames.shape, vs.PITCH_FRAME_DTYPE).view(np.uint8), frames.view(np.uint8))
    assert_same(out, want)
    assert np.array_equal(mk, wm), np.argwhere(mk != wm)[:6]
    for f in gr.REC_DTYPE.names:
        assert np.array_equal(rec[f], wrec[f]), (f, rec[f][:8], wrec[f][:8])
    if segs:
        assert np.array_equal(seg, wseg.view(np.int32).reshape(n, 4 * segs))
    else:
        assert (seg == S32).all()
    return want, wm, wrec, wseg


def rows_of(n, ns, fs=16000, seed=0):
    """n rows of ns samples: the constructed signals and the hostile bank, in turn"""
    pool = []
    for sig in (ps.glide()[0], ps.gaps(), ps.octave_trap(), ps.subharmonic()):
        row = np.zeros(ns, np.int16)
        row[:min(ns, len(sig))] = sig[:ns]
        pool.append(row)
    pool += list(hs.bank(fs, ns, seed).values())
    return np.stack([pool[k % len(pool)] for k in range(n)])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_rows_and_ragged_lengths(eng, n):
    """lengths around 3*tmax + 2 (no frame, one frame) and around a frame boundary, and anything up to the row"""
    ns = 4000
    tmin, tmax = ar.lag_bounds(16000)
    base = 3 * tmax + 2
    pcm = rows_of(n, ns)
    rng = np.random.default_rng(n)
    lengths = rng.integers(900, ns + 1, n).astype(np.int32)
    edge = [ns, base + 160, base - 1, base, base + 159, 0, base + 5 * 160 - 1, base + 5 * 160]
    lengths[:min(n, len(edge))] = edge[:n]
    want, wm, wrec, wseg = check_dev(eng, pcm, 16000, lengths)
    assert want["status"][0] == 0 and want["n_periods"][0] >= 10
    if n >= 3:
        assert want["status"][2] == vs.VS_AC_TOO_SHORT and wrec["n_marks"][2] == 0


def test_the_constructed_signals_whole(eng):
    sigs = [ps.glide()[0], ps.gaps(), ps.octave_trap(), ps.subharmonic()]
    ns = max(len(s) for s in sigs)
    pcm = np.zeros((4, ns), np.int16)
    for i, s in enumerate(sigs):
        pcm[i, :len(s)] = s
    lengths = np.array([len(s) for s in sigs], np.int32)
    want, wm, wrec, wseg = check_dev(eng, pcm, 16000, lengths)
    assert wrec["n_segments"].tolist()[:3] == [1, 2, 1] and wrec["n_marks"].tolist()[:3] == [101, 120, 100]
    assert want["jitter_local"][1] == 0.0 and want["shimmer_local"][1] == 0.0 and want["status"][1] == 0
    for kw in (dict(edge_frames=0), dict(segments="longest"), dict(min_frames=50), dict(edge_frames=16, min_frames=1)):
        if "segments" in kw:
            kw = dict(segments=vs.VS_MG_LONGEST)
        check_dev(eng, pcm, 16000, lengths, **kw)
    # the host-buffer call: the track and the walk in one, the same records
    got = eng.measure_guided(pcm, 16000, lengths=lengths, marks=400, segs=6)
    frames = track_of(eng, pcm, 16000, lengths, {})
    assert np.array_equal(got[4].view(np.uint8), frames.view(np.uint8))
    w = gr.guided(pcm, 16000, frames, lengths, marks=400, segs=6)
    assert_same(got[0], w[0])
    assert np.array_equal(got[1], w[1]) and np.array_equal(got[2], w[2]) and np.array_equal(got[3], w[3])
    got = eng.measure_guided(pcm, 16000, lengths=lengths, pitch=dict(octave_q=3277), edge_frames=2)
    frames, _ = eng.pitch(pcm, 16000, lengths=lengths, octave_q=3277)
    assert got[1] is None and got[3] is None
    assert_same(got[0], gr.guided(pcm, 16000, frames, lengths, edge_frames=2)[0])


@pytest.mark.parametrize("polarity", [1, -1])
def test_four_rates_in_one_call(eng, polarity):
    """hostile_signals.ACOUSTIC_CASES' rates and lengths in one call (one pitch range for all), rows of the bank"""
    picks = ("am_sine_120", "sine_150_noise", "impulses_110", "two_tones")
    cases = hs.ACOUSTIC_CASES
    ns = max(c[1] for c in cases)
    fs = np.array([c[0] for c in cases for _ in picks], np.int32)
    lengths = np.array([c[1] for c in cases for _ in picks], np.int32)
    pcm = np.zeros((len(fs), ns), np.int16)
    i = 0
    for c in cases:
        b = hs.bank(c[0], c[1], 2)
        for k in picks:
            pcm[i, :c[1]] = b[k]
            i += 1
    want, *_ = check_dev(eng, pcm, fs, lengths, marks=600, polarity=polarity, f0_min=60.0, f0_max=400.0)
    assert (want["status"] == 0).sum() >= 8


@pytest.mark.parametrize("polarity", [1, -1])
def test_the_hostile_bank(eng, polarity):
    """noise, silence, DC, squares, tones outside the range, and the jump trains whose third window begins inside the
    stretch already walked (the walk-again path)"""
    names, pcm = hs.matrix(hs.bank(16000, 8000, 0))
    want, wm, wrec, wseg = check_dev(eng, pcm, 16000, marks=1200, polarity=polarity)
    assert want["status"][names.index("zeros")] == vs.VS_AC_UNVOICED
    frames = track_of(eng, pcm, 16000, None, {})
    for k in ("jump_300", "jump_320"):
        i = names.index(k)
        events = []
        r = gr.guided_row(pcm[i], 16000, frames[i], events, polarity=polarity)
        assert r["rec"]["n_periods"] >= 100 and "again" in events, k   # a window begins inside the stretch already walked


def fabricated(n, fp, lag, q=20000):
    fr = np.frombuffer(bytes([0xA5]) * (n * fp * 96), dtype=vs.PITCH_FRAME_DTYPE).reshape(n, fp).copy()
    fr["lag"] = lag
    fr["q"] = q
    return fr


def test_fabricated_frames(eng):
    """records no pitch launch wrote: only lag (inside the range) and q are believed"""
    fs, ns = 16000, 12000
    tmin, tmax = ar.lag_bounds(fs)
    F = pr.frame_count(ns, tmax, 160)
    x, _ = ps.train([123] * 110, lambda p: 70, lambda c: 9000.0)
    short, _ = ps.train([90] * 140, lambda p: 50, lambda c: 9000.0)   # under a lag of 123 every run's third window begins
    pcm = np.stack([x[:ns], x[:ns], x[:ns], x[:ns], short[:ns]])         # inside its second: walked again
    f = np.arange(F + 4)
    lag = np.stack([np.where(f % 7 == 0, -5, np.where(f % 7 == 1, tmax + 1, np.where(f % 7 == 2, tmin - 1, 123))),
                    np.where(f % 2 == 0, 123, 0),                   # voiced and unvoiced alternating every frame
                    np.where(f % 2 == 0, tmin, tmax),               # the track jumps: empty windows
                    np.full(F + 4, 2 ** 31 - 1), np.where(f % 4 == 3, 0, 123)]).astype(np.int32)
    q = np.stack([np.where(f % 3 == 0, -2 ** 31, 2 ** 31 - 1), f * 1000 - 7, np.full(F + 4, 32768), f, np.full(F + 4, 0)])
    fr = fabricated(5, F + 4, lag, q.astype(np.int32))
    want, wm, wrec, wseg = check_dev(eng, pcm, fs, frames=fr, marks=300, segs=3, edge_frames=0, min_frames=1)
    assert wrec["n_segments"][1] == (F + 1) // 2 > 3 and wrec["n_segments"][0] > 3    # more runs than seg_pitch
    assert want["status"][3] == vs.VS_AC_UNVOICED and wrec["n_segments"][4] >= 15
    events = []
    gr.guided_row(pcm[2], fs, fr[2], events, edge_frames=0, min_frames=1)
    assert "empty" in events
    events = []
    gr.guided_row(pcm[4], fs, fr[4], events, edge_frames=0, min_frames=1)
    assert events.count("again") >= 20
    check_dev(eng, pcm, fs, frames=fr, marks=7, segs=0, edge_frames=0, min_frames=1)  # fewer slots than marks, no segs
    assert wrec["n_marks"].max() > 7
    check_dev(eng, pcm, fs, frames=fr, marks=300, segs=2)
    check_dev(eng, pcm, fs, frames=fr, marks=300, segs=2, segments=vs.VS_MG_LONGEST, edge_frames=0, min_frames=1)


def test_a_long_track(eng):
    """hop 1 ms: 940 frames, runs that cross the 64-frame chunks of the plan kernel"""
    x = np.zeros(16000, np.int16)
    g = ps.gaps()
    x[:16000] = g[:16000]
    for kw in (dict(), dict(segments=vs.VS_MG_LONGEST), dict(edge_frames=16, min_frames=64)):
        want, wm, wrec, wseg = check_dev(eng, x[None], 16000, hop_s=0.001, **kw)
        assert wrec["n_frames_walked"][0] > 64


def _vowels(n=4):
    from oracle import pyoracle
    specs = [(["-d", "1", "-f", "100", "-s", "10"], ["-v", "a"], 300 + k) for k in (6, 0, 1, 2)[:n]]
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(22050, d)
    return pyoracle.synth(lanes, ns), 1.0 / lanes[0].gain


def test_the_device_chain_on_oracle_vowels(eng):
    """pitch -> guided -> glottal -> cplpc on device pointers against Engine.closed_phase(guided=True) and against the
    restatements' chain: 4 of the 16 vowels at -s 10, the row the one-window estimate marks at 440 first"""
    pcm, scale = _vowels()
    fs = 22050
    got = eng.closed_phase(pcm, fs, de_emphasis=1.0, scale=scale, guided=True)
    want = gr.closed_phase(pcm, fs, de_emphasis=1.0, scale=scale)
    assert np.array_equal(got["residual"], want["residual"])
    assert np.array_equal(got["frames"].view(np.uint8), want["frames"].astype(vs.PITCH_FRAME_DTYPE).view(np.uint8))
    assert_same(got["meas"], want["meas"])
    assert np.array_equal(got["marks"], want["marks"])
    assert (got["meas"]["n_periods"] == 99).all() and (got["sets"]["status"][:, 0] == 0).all()
    for f in ("n_cycles", "n_rejected", "status"):
        assert np.array_equal(got["glottal"][f], want["glottal"][f]), f
    for i in range(len(pcm)):                                   # (the slots behind a row's cycles keep each side's fill)
        nc = int(want["glottal"]["n_cycles"][i] + want["glottal"]["n_rejected"][i])
        assert nc >= 90 and np.array_equal(got["cycles"][i, :nc], want["cycles"][i, :nc].astype(vs.GLOTTAL_CYCLE_DTYPE))
    assert np.array_equal(got["flow"], want["flow"])
    plain = eng.closed_phase(pcm, fs, de_emphasis=1.0, scale=scale)
    assert plain["meas"]["p0"][0] == 440 and "frames" not in plain
    # the same first-pass chain by hand, on the residual
    n, ns = pcm.shape
    mp, fp = ns // 2 + 2, got["frames"].shape[1]
    with eng.scope() as dev:
        d_res = dev.put(got["residual"])
        d_fr = dev.put(np.zeros((n, fp), vs.PITCH_FRAME_DTYPE))
        d_meas, d_rec = dev.room(n * 96), dev.room(n * 16)
        d_marks = dev.filled(n * mp, -1, np.int32)
        d_gl = dev.room(n * vs.GLOTTAL_DTYPE.itemsize)
        d_cyc = dev.put(np.zeros((n, mp), vs.GLOTTAL_CYCLE_DTYPE))
        eng.pitch_dev(d_res, ns, n, ns, fs, fp, d_fr)
        eng.measure_guided_dev(d_res, ns, n, ns, fs, d_fr, fp, d_meas, d_rec, d_marks, mp, segments=vs.VS_MG_LONGEST)
        eng.glottal_dev(d_res, ns, n, ns, d_meas, d_marks, mp, d_gl, cycles_ptr=d_cyc, cycles_pitch=mp)
        eng.synchronize()
        assert np.array_equal(dev.get(d_marks, (n, mp), np.int32), got["marks"])
        assert np.array_equal(dev.get(d_cyc, (n, mp), vs.GLOTTAL_CYCLE_DTYPE), got["cycles"])
        assert dev.get(d_rec, (n,), vs.GUIDED_REC_DTYPE)["n_segments"].tolist() == [1] * n
    g = eng.glottal(got["flow"], fs, guided=True)
    w = gr.measure_and_glottal(want["flow"], fs)
    assert np.array_equal(g["marks"], w[1]) and np.array_equal(g["glottal"]["oq"], w[2]["oq"], equal_nan=True)
    assert np.array_equal(g["glottal"]["n_cycles"], w[2]["n_cycles"])


def test_refusals(eng):
    pcm = rows_of(2, 2000)
    E = vs._ffi

    def code(fn, *a, **kw):
        with pytest.raises(vs.VsError) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(eng.measure_guided, pcm, 16000, polarity=0) == E.VS_ERR_ARG
    assert code(eng.measure_guided, pcm, 16000, segments=2) == E.VS_ERR_ARG
    assert code(eng.measure_guided, pcm, 16000, hop_s=float("nan")) == E.VS_ERR_ARG
    assert code(eng.measure_guided, pcm, 16000, edge_frames=17) == E.VS_ERR_RANGE
    assert code(eng.measure_guided, pcm, 16000, edge_frames=-1) == E.VS_ERR_RANGE
    assert code(eng.measure_guided, pcm, 16000, min_frames=0) == E.VS_ERR_RANGE
    assert code(eng.measure_guided, pcm, [16000, 3]) == E.VS_ERR_RANGE
    assert code(eng.measure_guided, pcm, 16000, pitch=dict(jump_q=-1)) == E.VS_ERR_ARG
    with eng.scope() as dev:
        src, d_fr = dev.put(pcm), dev.put(np.zeros((2, 7), vs.PITCH_FRAME_DTYPE))
        d_out, d_rec, d_seg = dev.room(2 * 96), dev.room(2 * 16), dev.room(2 * 16)
        ok = (src, 2000, 2, 2000, 16000, d_fr, 7, d_out, d_rec)
        eng.measure_guided_dev(*ok)
        eng.synchronize()
        assert code(eng.measure_guided_dev, src, 2000, 2, 2000, 16000, d_fr, 6, d_out, d_rec) == E.VS_ERR_RANGE  # 7 frames
        assert code(eng.measure_guided_dev, src, 2000, 2, 2000, 16000, d_fr, 0, d_out, d_rec) == E.VS_ERR_ARG
        assert code(eng.measure_guided_dev, src, 2000, 2, 2000, 16000, None, 7, d_out, d_rec) == E.VS_ERR_ARG
        assert code(eng.measure_guided_dev, src, 2000, 2, 2000, 16000, d_fr, 7, None, d_rec) == E.VS_ERR_ARG
        assert code(eng.measure_guided_dev, src, 2000, 2, 2000, 16000, d_fr, 7, d_out, None) == E.VS_ERR_ARG
        assert code(eng.measure_guided_dev, *ok, segs_ptr=d_seg, seg_pitch=0) == E.VS_ERR_ARG
        assert code(eng.measure_guided_dev, *ok, marks_ptr=d_seg, marks_pitch=0) == E.VS_ERR_ARG
        assert code(eng.measure_guided_dev, src, 1999, 2, 2000, 16000, d_fr, 7, d_out, d_rec) == E.VS_ERR_ARG
        assert code(eng.measure_guided_dev, *ok, segs_ptr=d_seg, seg_pitch=1 << 31) == E.VS_ERR_UNSUPPORTED
        assert code(eng.measure_guided_dev, *ok, lengths=[2001, 5]) == E.VS_ERR_ARG


def _wav(path, fs, x, header):
    data = x.tobytes()
    if header == 44:
        h = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, 1, 1, fs, fs * 2, 2, 16, b"data",
                        len(data))
    else:
        buf = (C.c_ubyte * 72)()
        assert vs.load().vs_wav_header_write(buf, 72, fs, len(data) / 2.0 / fs) == 72
        h = bytes(buf)
    open(path, "wb").write(h + data)


def _payload(path, header=44):
    return np.frombuffer(open(path, "rb").read()[header:], dtype=np.int16)


def test_the_programs(eng, tmp_path):
    """acoustic -T, glottal -T and vclosed -T on small files against the restatements' lines"""
    import cplpc_ref as cp
    import glottal_ref as gl
    sigs = {"glide.wav": (ps.glide()[0], 16000, 44), "gaps.wav": (ps.gaps(), 16000, 72),
            "trap.wav": (ps.octave_trap()[:9000], 16000, 44), "short.wav": (np.zeros(100, np.int16), 8000, 72)}
    for name, (x, fs, header) in sigs.items():
        _wav(str(tmp_path / name), fs, x, header)
    r = subprocess.run([os.path.join(BIN, "acoustic"), "-T", "-m"] + list(sigs), cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    want = ["# file " + " ".join(gr.COLUMNS[1:])]
    for name, (x, fs, header) in sigs.items():
        out, mk, rec, _, _ = gr.track_and_guided(x[None], fs, marks=len(x) // 2 + 2)
        want.append(gr.format_line(name, out[0], rec[0]))
        want.append("# marks %s:" % name + "".join(" %d" % v for v in mk[0][:rec["n_marks"][0]]))
    assert r.stdout.splitlines() == want
    assert want[3].split()[-2:] == ["2", "87"] and want[7].split()[-3:] == ["1", "0", "0"]
    r = subprocess.run([os.path.join(BIN, "acoustic"), "-T", "-f", "70", "-F", "400", "gaps.wav"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    out, _, rec, _, _ = gr.track_and_guided(sigs["gaps.wav"][0][None], 16000, f0_min=70.0, f0_max=400.0)
    assert r.returncode == 0 and r.stdout.splitlines()[1:] == [gr.format_line("gaps.wav", out[0], rec[0])]
    plain = subprocess.run([os.path.join(BIN, "acoustic"), "gaps.wav"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert plain.stdout.splitlines() == ["# file " + " ".join(ar.COLUMNS[1:]),
                                         ar.format_line("gaps.wav", ar.measure(sigs["gaps.wav"][0][None], 16000)[0])]

    # glottal -T: two flows of the oracle's source, one cut short, in one call
    from oracle import pyoracle
    lanes, d = vs.lanes_from_specs([(["-d", "0.5", "-f", "100", "-s", "10"], ["-v", "a"], 306 + k) for k in range(2)])
    ns = vs.num_samples(22050, d)
    flow = pyoracle.source(lanes, ns)
    files = {"flow0.wav": flow[0], "flow1.wav": flow[1, :7000]}
    for name, x in files.items():
        _wav(str(tmp_path / name), 22050, x, 44)
    r = subprocess.run([os.path.join(BIN, "glottal"), "-T", "-c"] + list(files), cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    want = ["# file OQ ClQ SQ QOQ NAQ cycles rejected status"]
    for name, x in files.items():
        meas, mk, rec, cyc, _ = gr.measure_and_glottal(x[None], 22050, cycles_pitch=len(x) // 2)
        want.append(gl.format_line(name, rec[0]))
        want += [gl.format_cycle_line(c) for c in cyc[0, :rec["n_cycles"][0] + rec["n_rejected"][0]]]
        assert rec["n_cycles"][0] >= 20
    assert r.stdout.splitlines() == want

    # vclosed -T: the -s 10 vowel whose one-window estimate is an octave low
    pcm, scale = _vowels(1)
    _wav(str(tmp_path / "speech.wav"), 22050, pcm[0], 44)
    out = str(tmp_path / "flow.wav")
    r = subprocess.run([os.path.join(BIN, "vclosed"), "-T", "-i", str(tmp_path / "speech.wav"), "-o", out, "-d", "1", "-s",
                        "%.17g" % scale], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    w = gr.closed_phase(pcm, 22050, de_emphasis=1.0, scale=scale, n_formants=0)
    s = w["sets"]
    assert r.stdout.splitlines() == [cp.format_line(out, w["flow_stat"][0], s["counts"][0], s["r0"][0], s["err"][0],
                                                    s["status"][0])]
    assert np.array_equal(_payload(out), w["flow"][0]) and s["status"][0, 0] == 0 and w["meas"]["n_periods"][0] == 99
