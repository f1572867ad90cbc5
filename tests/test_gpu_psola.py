"""PSOLA on the device (csrc/vs_psola.hip) against the restatement (tests/psola_ref.py), byte for byte: the output rows, the
status records and the synthesis records.  Rows with the guided marks of the pitch track's signals and rows with drawn
hostile marks, runs and targets; lengths around the overlap-add kernel's tile; output rows at several pitches and odd
bases, so that the 16-byte and the sample-by-sample stores both run; dense marks that take several stagings; the target
read in place from a vs_strack_launch cycle log behind the pitch track and the guided marks; identity; the program.
Every output sits inside a guard band and what a launch must not write keeps its sentinel."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_support as gs  # noqa: E402
import guided_ref as gr  # noqa: E402
import pitch_signals as ps  # noqa: E402
import psola_ref as pp  # noqa: E402
import strack_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voice_synth_amd", "bin")
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
S8 = 0x5A
TILE = 2048                  # VS_PS_TILE
NS = 6000


@pytest.fixture(scope="module")
def eng():
    e = vs.Engine(0)
    yield e
    e.close()


def sentinel_records(shape, dtype):
    n = int(np.prod(shape))
    return np.frombuffer(bytes([S8]) * (n * dtype.itemsize), dtype=dtype).reshape(shape).copy()


def same_records(got, want, what):
    assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, what
    g, w = got.view(np.uint8).reshape(got.shape + (-1,)), want.view(np.uint8).reshape(want.shape + (-1,))
    bad = np.argwhere((g != w).any(axis=-1))
    assert len(bad) == 0, (what, bad[:6], got[tuple(bad[0])], want[tuple(bad[0])])


def run_dev(eng, b, pitch, offset_bytes, segs=True, gain=True, in_pitch=None):
    """vs_psola_launch of the batch b on device pointers: the output rows in GuardedRows at that pitch and base, the PCM
    staged at in_pitch between padding that is not silence, the status and synthesis records in sentinel-filled memory"""
    n, ns = b["x"].shape
    in_pitch = ns if in_pitch is None else in_pitch
    out = gs.GuardedRows(n, ns, pitch, offset_bytes)
    sp = b["sp"]
    with eng.scope() as dev:
        out.on(dev)
        d_x = dev.put(gs.staged_input(b["x"], in_pitch)) + 2 * gs.GUARD
        d_mk, d_rec = dev.put(b["marks"]), dev.put(b["rec"])
        d_sg = dev.put(b["segs"]) if segs else None
        d_st, d_T, d_cnt = dev.put(b["start"]), dev.put(b["T"]), dev.put(b["count"])
        d_g = dev.put(b["gain"]) if gain else None
        d_stat = dev.filled(n * vs.PSOLA_STAT_DTYPE.itemsize, S8, np.uint8)
        d_sy = dev.filled(n * sp * vs.PSOLA_MARK_DTYPE.itemsize, S8, np.uint8)
        eng.psola_dev(d_x, in_pitch, n, ns, d_mk, b["marks"].shape[1], d_rec, d_st, 4, d_T, 4, d_cnt, 4, b["start"].shape[1],
                      out.first(pitch, offset_bytes), pitch, d_stat, d_sy, sp, segs_ptr=d_sg,
                      seg_pitch=b["segs"].shape[1] if segs else 0, gain_ptr=d_g, gain_stride=4 if gain else 0,
                      lengths=b["lengths"], pmin=b["pmin"], pmax=b["pmax"])
        eng.synchronize()
        y = out.rows_back(pitch, offset_bytes, (pitch, offset_bytes)).copy()
        stat = dev.get(d_stat, (n,), vs.PSOLA_STAT_DTYPE)
        sy = dev.get(d_sy, (n, sp), vs.PSOLA_MARK_DTYPE)
    return y, stat, sy


def expected(b, segs=True, gain=True):
    n, ns = b["x"].shape
    return pp.psola(b["x"], b["lengths"], b["marks"], b["rec"], b["segs"] if segs else None, b["start"], b["T"],
                    b["gain"] if gain else None, b["count"], b["pmin"], b["pmax"], b["sp"],
                    out=np.full((n, ns), gs.SENTINEL, dtype=np.int16), synth=sentinel_records((n, b["sp"]), pp.MARK_DTYPE))


# ---- the batch: 48 rows of at most 6000 samples ----

def drawn_row(rng, i, ns, mp, sgp, tp):
    """a hostile row: (x, length, marks [mp], n_segments, n_marks, segs [(first, m)], start, T, gain, count)"""
    length = (777, 1, 0)[i - 4] if 4 <= i < 7 else int(rng.choice([ns, ns, ns, ns - 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]))
    x = rng.integers(-32768, 32768, ns).astype(np.int16) if i % 3 else rng.integers(-9000, 9001, ns).astype(np.int16)
    marks, runs, at = [], [], int(rng.integers(0, 200))
    for r in range(int(rng.integers(1, 5))):
        P = int(rng.choice([33, 40, 47, 80, 123, 200, 700]))
        m = int(rng.integers(2, 50))
        steps = np.maximum(1, (P * rng.uniform(0.8, 1.25, m - 1)).astype(np.int64))
        run = at + np.concatenate([[0], np.cumsum(steps)])
        if (run < length).sum() >= 2:
            run = run[run < length]                          # (a row of 777 samples has runs too)
        flaw = int(rng.integers(0, 20))
        if flaw == 0:
            run = run[:1]                                    # one mark
        elif flaw == 1:
            run[len(run) // 2] = run[len(run) // 2 - 1]      # not increasing
        elif flaw == 2:
            run = run + max(0, length - int(run[-1]))        # the last mark at len
        elif flaw == 3 and len(run) > 2:
            run[-1] = run[-2] + 2049                         # a period above the longest lag
        elif flaw == 4 and marks:
            run = run - (int(run[0]) - marks[-1])            # begins at the end of the run before
        elif flaw == 5 and length > 0:
            run = run + (length - 1 - int(run[-1]))          # E is the row's last sample
        if len(marks) + len(run) > mp:
            break
        runs.append((len(marks), len(run)))
        marks += [int(v) for v in run]
        at = int(run[-1]) + int(rng.integers(1, 400))
    segs = list(runs)
    n_segments = len(segs)
    which = int(rng.integers(0, 16))
    if which == 0 and segs:
        segs[0] = (segs[0][0], segs[0][1] + mp)              # marks past the array
    elif which == 1 and segs:
        segs[-1] = (-1, segs[-1][1])
    elif which == 2:
        n_segments = sgp + 3                                 # more runs than slots: the slots behind hold what they hold
    elif which == 3:
        n_segments = -1
    while len(segs) < sgp:
        segs.append((int(rng.integers(0, mp)), int(rng.integers(0, 6))))
    # the target: contiguous stretches with holes between them, periods around the row's, some of them out of range
    start, T = [], []
    g = int(rng.integers(-200, 400))
    while len(start) < tp and g < ns + 500:
        P = int(rng.choice([40, 60, 100, 150, 250, 320]))
        for _ in range(int(rng.integers(1, 25))):
            t = int(P * rng.uniform(0.9, 1.1))
            if rng.random() < 0.05:
                t = int(rng.choice([0, 1, 31, 321, -5, INT32_MAX, INT32_MIN, 2049]))
            start.append(g)
            T.append(t)
            g += t if abs(t) < 5000 else 100
        if rng.random() < 0.5:
            g += int(rng.integers(1, 600))                   # a hole
        elif rng.random() < 0.2:
            g -= int(rng.integers(1, 300))                   # start decreases
    start, T = start[:tp], T[:tp]
    J = len(start)
    if rng.random() < 0.1:
        start[int(rng.integers(0, J))] = int(rng.choice([INT32_MIN, INT32_MAX]))
    start += [0] * (tp - J)
    T += [100] * (tp - J)
    gain = rng.integers(int(0.5 * pp.Q), int(1.9 * pp.Q), tp)
    bad = rng.random(tp) < 0.08
    gain[bad] = rng.choice([0, 65535, -1, 65536, INT32_MIN, INT32_MAX], int(bad.sum()))
    count = int(rng.choice([J, J, J, tp + 50, -1, 0, max(0, J - 3)]))
    return x, length, marks, n_segments, len(marks), segs, start, T, gain, count


def make_batch():
    rng = np.random.default_rng(20261)
    n, ns, mp, sgp, tp = 48, NS, 160, 5, 200
    b = dict(x=np.zeros((n, ns), np.int16), lengths=np.zeros(n, np.int32), marks=np.full((n, mp), -1, np.int32),
             rec=np.zeros(n, vs.GUIDED_REC_DTYPE), segs=np.zeros((n, sgp), vs.GUIDED_SEG_DTYPE),
             start=np.zeros((n, tp), np.int32), T=np.zeros((n, tp), np.int32), gain=np.zeros((n, tp), np.int32),
             count=np.zeros(n, np.int32), pmin=32, pmax=320, sp=50)
    # the three signals of the definition's consequences, cut to the batch's length, with the restatement's guided marks
    train = ps.train([123] * 100, lambda p: int(0.6 * p), lambda c: 8000.0)[0]
    g = ps.gaps()                # cut to 20 cycles, 540 zeros, 540 samples of the noise, 20 cycles
    gaps = np.concatenate([g[:2460], g[7380:7920], g[11380:11920], g[-2460:]])
    signals = [ps.glide()[0][:ns], gaps, train[:ns], train[:TILE + 1]]
    T140 = rng.integers(119, 128, tp)
    for i, s in enumerate(signals):
        out, mk, rec, sg, _ = gr.track_and_guided(s[None], 16000, marks=mp, segs=sgp)
        b["x"][i, :len(s)] = s
        b["lengths"][i] = len(s)
        b["marks"][i], b["rec"][i], b["segs"][i] = mk[0], tuple(rec[0]), sg[0]
        b["T"][i] = T140
        b["start"][i] = np.cumsum(T140) - T140
        b["gain"][i] = rng.integers(int(0.85 * pp.Q), int(1.15 * pp.Q) + 1, tp)
        b["count"][i] = tp
    assert b["rec"]["n_segments"][:3].tolist() == [1, 2, 1] and (b["rec"]["n_marks"][:4] < mp).all()
    for i in range(len(signals), n):
        x, length, marks, nseg, nm, segs, start, T, gain, count = drawn_row(rng, i, ns, mp, sgp, tp)
        b["x"][i], b["lengths"][i] = x, length
        b["marks"][i, :len(marks)] = marks
        b["rec"][i] = (nseg, nm, 0, 0)
        b["segs"]["first_mark_index"][i], b["segs"]["n_marks"][i] = [s[0] for s in segs], [s[1] for s in segs]
        b["start"][i], b["T"][i], b["gain"][i], b["count"][i] = start, T, gain, count
    return b


@pytest.fixture(scope="module")
def batch():
    b = make_batch()
    return dict(b=b, full=expected(b), no_segs=expected(b, segs=False), no_gain=expected(b, gain=False))


def test_the_batch_is_what_it_claims(batch):
    """no GPU work: the restatement's answers cover the status bits, both kinds of run, full and cut rows, clamps"""
    y, st, sy = batch["full"]
    s = st["status"]
    assert (s & pp.BAD_RUN).any() and (s & pp.OVERFLOW).any() and (s & pp.NO_RUN).any() and (s == 0).any()
    assert (st["n_runs_done"] > 1).any() and (st["n_clipped"] > 0).any() and (st["n_governed"] > 0).any()
    assert ((st["n_runs"] > st["n_runs_done"]) & (st["n_runs_done"] > 0)).any()
    assert st["n_synth"].max() > batch["b"]["sp"] - 10 and (batch["no_segs"][1]["n_runs"] == 1).all()
    lengths = batch["b"]["lengths"]
    for want in (0, 1, TILE - 1, TILE, TILE + 1, NS):
        assert (lengths == want).any(), want
    # an interval that straddles the first tile's edge in a resynthesised run, and a run whose E is the row's last sample
    t = sy["t"]
    straddle = E_last = False
    for i in range(len(st)):
        k = int(st["n_synth"][i])
        for j in range(k - 1):
            if sy["cycle"][i, j] != pp.RUN_END and t[i, j] < TILE <= t[i, j + 1]:
                straddle = True
        E_last |= k > 0 and t[i, k - 1] == lengths[i] - 1
    assert straddle and E_last


@pytest.mark.parametrize("pitch,offset_bytes", ((NS, 0), (NS + 3, 2), (NS + 8, 6), (NS + 1, 14)))
def test_device_is_the_restatement(eng, batch, pitch, offset_bytes):
    y, st, sy = run_dev(eng, batch["b"], pitch, offset_bytes, in_pitch=NS + (offset_bytes // 2))
    wy, wst, wsy = batch["full"]
    same_records(st, wst.astype(vs.PSOLA_STAT_DTYPE), "stat")
    same_records(sy, wsy.astype(vs.PSOLA_MARK_DTYPE), "synth")
    gs.same_rows(y, wy, "y")


def test_without_segment_records_and_without_gains(eng, batch):
    for key, kw in (("no_segs", dict(segs=False)), ("no_gain", dict(gain=False))):
        y, st, sy = run_dev(eng, batch["b"], NS + 5, 4, **kw)
        wy, wst, wsy = batch[key]
        same_records(st, wst.astype(vs.PSOLA_STAT_DTYPE), key + " stat")
        same_records(sy, wsy.astype(vs.PSOLA_MARK_DTYPE), key + " synth")
        gs.same_rows(y, wy, key + " y")


def test_the_host_path_is_the_device_path(eng, batch):
    b = batch["b"]
    wy, wst, wsy = batch["full"]
    n = len(b["x"])
    y, st, sy = eng.psola(b["x"], 16000, b["marks"], b["rec"], b["start"], b["T"], count=b["count"], segs=b["segs"],
                          gain=b["gain"], lengths=b["lengths"], synth=b["sp"], pmin=b["pmin"], pmax=b["pmax"],
                          out=np.full((n, NS), gs.SENTINEL, np.int16),
                          synth_fill=sentinel_records((n, b["sp"]), vs.PSOLA_MARK_DTYPE))
    same_records(st, wst.astype(vs.PSOLA_STAT_DTYPE), "stat")
    same_records(sy, wsy.astype(vs.PSOLA_MARK_DTYPE), "synth")
    gs.same_rows(y, wy, "y")


def test_identity_on_the_device(eng, batch):
    b = dict(batch["b"])
    b["count"] = np.zeros(len(b["x"]), np.int32)
    y, st, sy = run_dev(eng, b, NS + 2, 2)
    for i, length in enumerate(b["lengths"]):
        assert np.array_equal(y[i, :length], b["x"][i, :length]), i
        assert (y[i, length:] == gs.SENTINEL).all(), i
    assert (st["n_governed"] == 0).all() and (st["n_clipped"] == 0).all() and (st["n_runs_done"] > 0).any()


def test_dense_marks_take_several_stagings(eng):
    """periods of 2..7 samples: more than VS_PS_STAGE synthesis marks in one tile, and more than one round of the section"""
    rng = np.random.default_rng(7)
    n, ns, mp, tp = 6, 5000, 1800, 2400
    b = dict(x=rng.integers(-20000, 20001, (n, ns)).astype(np.int16), lengths=np.array([ns, ns - 1, 4097, 2048, ns, 300], np.int32),
             marks=np.full((n, mp), -1, np.int32), rec=np.zeros(n, vs.GUIDED_REC_DTYPE),
             segs=np.zeros((n, 1), vs.GUIDED_SEG_DTYPE), start=np.zeros((n, tp), np.int32), T=np.zeros((n, tp), np.int32),
             gain=np.zeros((n, tp), np.int32), count=np.full(n, tp, np.int32), pmin=2, pmax=2048, sp=2500)
    for i in range(n):
        steps = rng.integers(1, 6, mp - 1) if i % 2 else rng.integers(2, 8, mp - 1)
        m = 3 + np.concatenate([[0], np.cumsum(steps)])
        m = m[m < b["lengths"][i]]
        b["marks"][i, :len(m)] = m
        b["rec"][i] = (1, len(m), 0, 0)
        T = rng.integers(2, 7, tp)
        b["T"][i], b["start"][i] = T, np.cumsum(T) - T
    b["sp"] = 2500
    b["count"][4] = 0
    y, st, sy = run_dev(eng, b, ns + 6, 10, segs=False, gain=False)
    wy, wst, wsy = expected(b, segs=False, gain=False)
    assert wst["n_synth"].max() > 1000 and (wst["status"] == 0).all() and (wst["n_governed"][:4] > 500).all()
    same_records(st, wst.astype(vs.PSOLA_STAT_DTYPE), "stat")
    same_records(sy, wsy.astype(vs.PSOLA_MARK_DTYPE), "synth")
    gs.same_rows(y, wy, "y")


# ---- the whole chain on the device: pitch -> guided -> source track -> psola, the target read in place ----

def test_chained_behind_the_source_track(eng):
    fs, ns, n = 16000, 4000, 6
    train = ps.train([123] * 100, lambda p: int(0.6 * p), lambda c: 8000.0)[0]
    x = np.stack([train[:ns], ps.glide()[0][:ns], ps.gaps()[5000:5000 + ns], ps.gaps()[:ns], ps.octave_trap()[:ns],
                  np.zeros(ns, np.int16)])
    lanes = [vs.lane_from_cli(["-j", j, "-r", "16000"], ["-v", "a"], seed=900 + k)[0]
             for k, j in enumerate(("2", "0.5", "3", "1", "2", "2"))]
    row = vs.strack_row_from_pitch(fs, ns)
    fp, mp, sgp, cp, sp = int(row["n_frames"]), 140, 4, 130, 150
    out = gs.GuardedRows(n, ns, ns + 3, 2)
    with eng.scope() as dev:
        out.on(dev)
        d_x = dev.put(x)
        d_fr = dev.put(np.zeros((n, fp), vs.PITCH_FRAME_DTYPE))
        d_meas = dev.room(n * vs.ACOUSTIC_DTYPE.itemsize)
        d_mk = dev.filled(n * mp, -1, np.int32)
        d_rec = dev.room(n * vs.GUIDED_REC_DTYPE.itemsize)
        d_sg = dev.put(np.zeros((n, sgp), vs.GUIDED_SEG_DTYPE))
        d_flow = dev.room(n * ns * 2)
        d_sst = dev.room(n * vs.STRACK_STAT_DTYPE.itemsize)
        d_cyc = dev.filled(n * cp * vs.STRACK_CYCLE_DTYPE.itemsize, S8, np.uint8)
        d_stat = dev.filled(n * vs.PSOLA_STAT_DTYPE.itemsize, S8, np.uint8)
        d_sy = dev.filled(n * sp * vs.PSOLA_MARK_DTYPE.itemsize, S8, np.uint8)
        eng.pitch_dev(d_x, ns, n, ns, fs, fp, d_fr)
        eng.measure_guided_dev(d_x, ns, n, ns, fs, d_fr, fp, d_meas, d_rec, d_mk, mp, d_sg, sgp)
        lag_at = vs.PITCH_FRAME_DTYPE.fields["lag"][1]
        eng.source_track_dev(lanes, ns, row, d_fr + lag_at, vs.PITCH_FRAME_DTYPE.itemsize, fp, d_flow, ns, d_sst,
                             cycles_ptr=d_cyc, cycles_pitch=cp)
        cyc, sst = vs.STRACK_CYCLE_DTYPE, vs.STRACK_STAT_DTYPE
        assert (cyc.fields["start"][1], cyc.fields["T"][1], cyc.itemsize) == (0, 4, 32)
        assert (sst.fields["n_cycles"][1], sst.itemsize) == (4, 24)
        eng.psola_dev(d_x, ns, n, ns, d_mk, mp, d_rec, d_cyc, 32, d_cyc + 4, 32, d_sst + 4, 24, cp,
                      out.first(ns + 3, 2), ns + 3, d_stat, d_sy, sp, segs_ptr=d_sg, seg_pitch=sgp, pmin=int(row["pmin"]),
                      pmax=int(row["pmax"]))
        eng.synchronize()
        y = out.rows_back(ns + 3, 2).copy()
        stat = dev.get(d_stat, (n,), vs.PSOLA_STAT_DTYPE)
        sy = dev.get(d_sy, (n, sp), vs.PSOLA_MARK_DTYPE)
    # the chain of restatements
    _, mk, rec, sg, frames = gr.track_and_guided(x, fs, marks=mp, segs=sgp)
    lags = np.ascontiguousarray(frames["lag"][:, :fp])
    _, wsst, _, logs = sr.source_track(lanes, ns, [row] * n, lags)
    start, T = np.zeros((n, cp), np.int32), np.zeros((n, cp), np.int32)
    for i, log in enumerate(logs):
        k = min(len(log), cp)
        start[i, :k], T[i, :k] = log["start"][:k], log["T"][:k]
    wy, wst, wsy = pp.psola(x, [ns] * n, mk, rec, sg, start, T, None, wsst["n_cycles"], int(row["pmin"]), int(row["pmax"]), sp,
                            synth=sentinel_records((n, sp), pp.MARK_DTYPE))
    same_records(stat, wst.astype(vs.PSOLA_STAT_DTYPE), "stat")
    same_records(sy, wsy.astype(vs.PSOLA_MARK_DTYPE), "synth")
    gs.same_rows(y, wy, "y")
    assert (wst["n_governed"][:5] > 10).all() and wst["status"][5] == pp.NO_RUN and np.array_equal(y[5], x[5])
    assert (wsst["n_cycles"][:5] >= 15).all()               # 4000 samples of periods between 80 and 220
    assert not np.array_equal(y[0], x[0])


# ---- the program ----

def _wav(path, fs, x):
    data = np.ascontiguousarray(x, dtype=np.int16).tobytes()
    h = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, 1, 1, fs, fs * 2, 2, 16, b"data",
                    len(data))
    open(path, "wb").write(h + data)


def _payload(path, header=44):
    return np.frombuffer(open(path, "rb").read()[header:], dtype=np.int16)


def _vpsola(tmp_path, *args):
    env = dict(os.environ, VS_SEED="77", VS_WAV_HEADER="44")
    return subprocess.run([os.path.join(BIN, "vpsola")] + list(args), cwd=tmp_path, capture_output=True, text=True,
                          timeout=120, env=env)


def test_the_program(eng, tmp_path):
    """no option: the input's samples; -x: the restatement chain (track, guided marks, periods, staircase, PSOLA); -j: the
    Engine's chain; a bad file gives 2"""
    fs = 16000
    x = np.concatenate([ps.gaps()[:7380 + 2000], ps.glide()[0][:5000]])
    N = len(x)
    _wav(str(tmp_path / "in.wav"), fs, x)
    r = _vpsola(tmp_path, "-i", "in.wav", "-o", "same.wav")
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "same.wav", "rb").read() == open(tmp_path / "in.wav", "rb").read()
    row = vs.strack_row_from_pitch(fs, N)
    tmin, tmax, F = int(row["pmin"]), int(row["pmax"]), int(row["n_frames"])
    mp, sgp = N // tmin + 2, F
    _, mk, rec, sg, frames = gr.track_and_guided(x[None], fs, marks=mp, segs=sgp)
    words = r.stdout.split()
    assert words[0] == "same.wav" and words[1:3] == [str(rec["n_segments"][0])] * 2 and words[4:] == ["0", "0", "0"]
    assert int(words[3]) == rec["n_marks"][0] and rec["n_segments"][0] == 2
    # -x 1.25
    r = _vpsola(tmp_path, "-i", "in.wav", "-o", "up.wav", "-x", "1.25")
    assert r.returncode == 0, r.stderr
    lags = frames["lag"][0, :F].astype(np.int64)
    voiced = (lags >= tmin) & (lags <= tmax)
    period = np.where(voiced, np.floor(lags / 1.25 + 0.5), 0).astype(np.int64)
    cap = N // tmin + 2
    start, T = pp.staircase(period, int(row["hop"]), int(row["offset"]), F, N, tmin, tmax, cap)
    J = len(start)
    st_, T_ = np.zeros((1, cap), np.int32), np.zeros((1, cap), np.int32)
    st_[0, :J], T_[0, :J] = start, T
    wy, wst, _ = pp.psola(x[None], [N], mk, rec, sg, st_, T_, None, [J], tmin, tmax, mp + 2 * sgp + 2)
    assert np.array_equal(_payload(tmp_path / "up.wav"), wy[0])
    assert r.stdout.split() == ["up.wav"] + [str(int(wst[f][0])) for f in ("n_runs", "n_runs_done", "n_synth", "n_governed",
                                                                           "n_clipped", "status")]
    assert wst["n_governed"][0] > 100 and not np.array_equal(wy[0], x)
    up = gr.track_and_guided(wy, fs)[0]["f0_hz"][0]
    base = gr.track_and_guided(x[None], fs)[0]["f0_hz"][0]
    assert 1.2 < up / base < 1.3
    # -j 2: the cycle log of the source track on the file's own lags, read in place
    r = _vpsola(tmp_path, "-i", "in.wav", "-o", "jit.wav", "-j", "2", "-S", "5")
    assert r.returncode == 0, r.stderr
    lane = vs.lane_from_cli(["-j", "2", "-r", "16000"], ["-v", "a"], seed=5)[0]
    _, sst, cyc = eng.source_track([lane], N, frames["lag"][:, :F], int(row["hop"]), int(row["offset"]), pmin=tmin, pmax=tmax,
                                   log_cycles=cap)
    wy, wst, _ = pp.psola(x[None], [N], mk, rec, sg, cyc["start"], cyc["T"], None, sst["n_cycles"], tmin, tmax,
                          mp + 2 * sgp + 2)
    assert np.array_equal(_payload(tmp_path / "jit.wav"), wy[0]) and int(r.stdout.split()[4]) == wst["n_governed"][0] > 50
    # refusals
    open(tmp_path / "bad.wav", "wb").write(b"RIFF")
    assert _vpsola(tmp_path, "-i", "bad.wav", "-o", "o.wav").returncode == 2
    assert _vpsola(tmp_path, "-i", "none.wav", "-o", "o.wav").returncode == 2
    _wav(str(tmp_path / "short.wav"), 16000, np.zeros(100, np.int16))
    assert _vpsola(tmp_path, "-i", "short.wav", "-o", "o.wav").returncode == 2
    for bad in (["-o", "o.wav"], ["-i", "in.wav"], ["-i", "in.wav", "-o", "o.wav", "-x", "0"],
                ["-i", "in.wav", "-o", "o.wav", "-x", "2", "-C", "100,200"], ["-i", "in.wav", "-o", "o.wav", "-C", "100"],
                ["-i", "in.wav", "-o", "o.wav", "-p", "2"], ["-i", "in.wav", "-o", "o.wav", "-q", "2"]):
        assert _vpsola(tmp_path, *bad).returncode == 1, bad


def test_refusals(eng):
    x = np.zeros((1, 500), np.int16)
    mk = np.array([[100, 200, 300]], np.int32)
    rec = np.zeros(1, vs.GUIDED_REC_DTYPE)
    one = np.array([[100]], np.int32)

    def rc(**kw):
        a = dict(lengths=None, synth=8, pmin=32, pmax=320)
        a.update(kw)
        with pytest.raises(vs.VsError) as e:
            eng.psola(x, 16000, mk, rec, one, one, **a)
        return e.value.code
    R, A = vs._ffi.VS_ERR_RANGE, vs._ffi.VS_ERR_ARG
    assert rc(pmin=1) == R and rc(pmax=2049) == R and rc(pmin=321) == R and rc(lengths=501) == R and rc(lengths=-1) == R
    assert rc(synth=1) == A
    with eng.scope() as dev:
        p = dev.room(4096)
        for bad in (dict(start_stride=2), dict(period_stride=6), dict(count_stride=0), dict(gain_ptr=p, gain_stride=3),
                    dict(segs_ptr=p, seg_pitch=0), dict(out_pitch=499), dict(synth_pitch=1)):
            a = dict(start_stride=4, period_stride=4, count_stride=4, out_pitch=500, synth_pitch=8)
            a.update(bad)
            with pytest.raises(vs.VsError) as e:
                eng.psola_dev(p, 500, 1, 500, p, 3, p, p, a["start_stride"], p, a["period_stride"], p, a["count_stride"], 1, p,
                              a["out_pitch"], p, p, a["synth_pitch"], segs_ptr=a.get("segs_ptr"),
                              seg_pitch=a.get("seg_pitch", 0), gain_ptr=a.get("gain_ptr"), gain_stride=a.get("gain_stride", 0))
            assert e.value.code == A, bad
