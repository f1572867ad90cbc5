"""The glottal parameters on the device (vs_glottal / vs_glottal_launch, bin/glottal) against their numpy restatement
(tests/glottal_ref.py) on the device's own marks: records and cycle records BIT FOR BIT, the doubles compared as bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acoustic_ref as ar  # noqa: E402
import glottal_ref as gr  # noqa: E402
import hostile_signals as hs  # noqa: E402
from test_glottal_ref import LEVELS, check_cycle_order, fabricated_marks  # noqa: E402
from test_gpu_acoustic import _payload, _pipeline, _wav  # noqa: E402

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(vs.__file__), "bin")
CANARY = 0x5A


def canaries(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, CANARY, dtype=np.uint8).view(dtype).reshape(shape)


def assert_bytes(got, want, what):
    """structured arrays equal byte for byte (NaNs and canaries included); names the first fields and slots that are not"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = []
        for f in got.dtype.names:
            g = np.ascontiguousarray(got[f]).view(np.uint8).reshape(got.size, -1)
            w = np.ascontiguousarray(want[f]).view(np.uint8).reshape(want.size, -1)
            for i in np.nonzero((g != w).any(axis=1))[0][:3]:
                bad.append((f, int(i), got[f].ravel()[i], want[f].ravel()[i]))
        raise AssertionError("%s differ: %s" % (what, bad[:10]))


def assert_host_result(res, pcm, lo, mid, pol, cp):
    """the result dict of Engine.glottal against the restatement on the marks that came back with it"""
    want, wc = gr.glottal(pcm, res["meas"], res["marks"], lo, mid, pol, cycles_pitch=cp, cycles_fill=canaries((1,), gr.CYCLE_DTYPE)[0])
    assert_bytes(res["glottal"], want, "records")
    assert_bytes(res["cycles"], wc, "cycle records")
    return want, wc


# ---- the oracle's batches

def _config_signals(engine, index, n=64):
    specs, fs, dur, _ = configs.config_specs(index, n)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    return engine.source(lanes, ns), engine.synth(lanes, ns), fs


@pytest.mark.parametrize("index", [2, 3, 5])
def test_config_batches_equal_the_restatement(engine, index):
    """64 flows and 64 vowels of a configuration at the three level pairs; configuration 3 (glottal noise, mixed vowels)
    under both polarities"""
    flow, pcm, fs = _config_signals(engine, index)
    accepted = 0
    for x in (flow, pcm):
        for pol in ((1, -1) if index == 3 else (1,)):
            for lo, mid in (LEVELS if pol == 1 else LEVELS[1:2]):
                cp = 510
                res = engine.glottal(x, fs, lo, mid, pol, marks=cp + 2, cycles=canaries((64, cp), vs.GLOTTAL_CYCLE_DTYPE))
                assert (res["meas"]["status"] == 0).mean() > 0.8 and res["meas"]["n_periods"].max() < cp   # (<= 484)
                want, _ = assert_host_result(res, x, lo, mid, pol, cp)
                accepted += int(want["n_cycles"].sum())
    assert accepted > 10000


# ---- signals the project does not synthesise

@pytest.mark.parametrize("polarity", [1, -1])
@pytest.mark.parametrize("case", hs.ACOUSTIC_CASES, ids=lambda c: "%dHz" % c[0])
def test_hostile_signals_equal_the_restatement(engine, case, polarity):
    """through the device's own marks: the 8 kHz case has periods of 4 samples (several cycles inside one 64-sample
    chunk), the 96 kHz case spans of 3491 samples (55 chunks; the bank has no longer one -- the ring at its fullest, 4096,
    and beyond it is test_valid_marks_with_spans_beyond_the_ring's)"""
    fs, n, f0_min, f0_max = case
    names, pcm = hs.matrix(hs.bank(fs, n, 0))
    cp = n // 4 + 1
    acc = rej = 0
    for lo, mid in LEVELS:
        res = engine.glottal(pcm, fs, lo, mid, polarity, f0_min, f0_max, marks=cp + 2,
                             cycles=canaries((len(names), cp), vs.GLOTTAL_CYCLE_DTYPE))
        assert res["meas"]["n_periods"].max() <= cp + 1
        want, wc = assert_host_result(res, pcm, lo, mid, polarity, cp)
        a, r = check_cycle_order(wc, want)
        acc += a
        rej += r
    assert acc > 0 and rej > 0
    m = res["marks"]
    if fs == 8000:
        assert (m[:, 1:] - m[:, :-1])[m[:, 1:] >= 0].min() == 4
    if fs == 96000 and polarity == 1:
        assert (m[:, 2:] - m[:, :-2])[m[:, 2:] >= 0].max() > 3000


# ---- geometry

def dev_chain(engine, buf, pitch, rows, ns, fs, lo, mid, pol, lengths, mp, cp, f0=(50.0, 500.0)):
    """measure_dev and glottal_dev on one stream with canaries in everything they write; buf holds one row more than
    `rows`.  Returns (meas, marks, records, cycle records or None), each with its canary row."""
    A, G, Cy = vs.ACOUSTIC_DTYPE, vs.GLOTTAL_DTYPE, vs.GLOTTAL_CYCLE_DTYPE
    sizes = [buf.nbytes, (rows + 1) * A.itemsize, (rows + 1) * mp * 4, (rows + 1) * G.itemsize, (rows + 1) * max(cp, 1) * Cy.itemsize]
    with engine.scope() as dev:
        ptrs = [dev.room(v) for v in sizes]
        engine.dev_upload(ptrs[0], buf)
        for p, v in zip(ptrs[1:], sizes[1:]):
            engine.dev_upload(p, np.full(v, CANARY, dtype=np.uint8))
        engine.measure_dev(ptrs[0], pitch, rows, ns, fs, ptrs[1], f0[0], f0[1], pol, lengths, ptrs[2], mp)
        engine.glottal_dev(ptrs[0], pitch, rows, ns, ptrs[1], ptrs[2], mp, ptrs[3], lo, mid, pol,
                           ptrs[4] if cp else None, cp)
        engine.synchronize()
        meas = engine.dev_download(ptrs[1], (rows + 1,), A)
        marks = engine.dev_download(ptrs[2], (rows + 1, mp), np.int32)
        rec = engine.dev_download(ptrs[3], (rows + 1,), G)
        cyc = engine.dev_download(ptrs[4], (rows + 1, max(cp, 1)), Cy)
    return meas, marks, rec, cyc


def assert_dev_result(buf, rows, ns, got, lo, mid, pol, cp):
    meas, marks, rec, cyc = got
    want = gr.glottal(buf[:rows, :ns], meas[:rows], marks[:rows], lo, mid, pol, cycles_pitch=cp,
                      cycles_fill=canaries((1,), gr.CYCLE_DTYPE)[0])
    want, wc = want if cp else (want, None)
    assert_bytes(rec[:rows], want, "records")
    assert (rec[rows:].view(np.uint8) == CANARY).all()
    if cp:
        assert_bytes(cyc[:rows], wc, "cycle records")
        assert (cyc[rows:].view(np.uint8) == CANARY).all()
    else:
        assert (cyc.view(np.uint8) == CANARY).all()
    return want


def _geometry_rows(rows, ns, pitch, seed):
    """rows of the 16 kHz bank (and what no row covers a loud square wave), ragged lengths"""
    b = hs.bank(16000, ns, seed)
    live = [k for k in b if k not in ("sine_30", "sine_1500")]
    loud = np.where(np.arange(pitch) % 7 < 3, 32767, -32768).astype(np.int16)
    buf = np.tile(loud, (rows + 1, 1))
    lengths = np.zeros(rows, dtype=np.int32)
    for i in range(rows):
        lengths[i] = ns - 13 * (i % 5) if i % 7 != 3 else 3 * 320 + 1 + (i % 2)  # every 14th row one sample too short
        buf[i, :ns] = 0
        buf[i, :lengths[i]] = b[live[i % len(live)]][:lengths[i]]
    return buf, lengths


@pytest.mark.parametrize("rows,extra,mp,cp", [(1, 1, 400, 400), (63, 7, 5, 2), (64, 1, 3, 1), (65, 7, 2, 4),
                                              (130, 1, "K+1", 0), (130, 7, "K+1", 7), (65, 1, 400, 2)])
def test_batch_geometry_and_untouched_slots(engine, rows, extra, mp, cp):
    """row counts around the wavefront, unaligned pitches, ragged lengths, marks_pitch 2 (no cycles), 3, 5, K + 1 of a
    middle row and more than any row's marks, no cycle records, one slot, fewer and more slots than cycles; canaries in
    every slot the definition leaves untouched (glottal_ref.glottal keeps them in its own copy)"""
    ns = 2500
    pitch = ns + extra
    buf, lengths = _geometry_rows(rows, ns, pitch, 3)
    if mp == "K+1":
        K = ar.measure(buf[:rows, :ns], 16000, lengths=lengths)["n_periods"]
        mp = int(np.sort(K)[len(K) // 2]) + 1
        assert (K + 1 < mp).any() and (K + 1 > mp).any() and mp >= 5
    lo, mid = LEVELS[rows % 3]
    got = dev_chain(engine, buf, pitch, rows, ns, 16000, lo, mid, 1, lengths, mp, cp)
    want = assert_dev_result(buf, rows, ns, got, lo, mid, 1, cp)
    total = want["n_cycles"] + want["n_rejected"]
    if mp == 2:
        assert np.all(want["status"] == gr.GL_NO_CYCLES)
    else:
        assert (want["n_cycles"] > 0).any() and total.max() == min(mp, int(got[0]["n_periods"][:rows].max()) + 1) - 2
    if rows > 7:
        assert (want["status"] & gr.GL_NO_CYCLES).any()
    if cp == 2:
        assert (total > cp).any()
    if cp == 400:
        assert (total < cp).all()


# ---- marks that are not the measurement's

def _foreign(engine, pcm, meas, marks, lo, mid, pol, cp):
    """vs_glottal_launch alone on uploaded records and marks; the PCM lies in the middle third of its allocation, so that
    a mark anywhere in [-n_samples, 2*n_samples) stays inside it"""
    rows, ns = pcm.shape
    mp = marks.shape[1]
    loud = np.where(np.arange(rows * ns) % 5 < 2, 32767, -32768).astype(np.int16).reshape(rows, ns)
    three = np.concatenate([loud, pcm, loud])
    A, G, Cy = vs.ACOUSTIC_DTYPE, vs.GLOTTAL_DTYPE, vs.GLOTTAL_CYCLE_DTYPE
    m = np.zeros(rows, dtype=A)
    m["n_periods"], m["status"] = meas["n_periods"], meas["status"]
    with engine.scope() as dev:
        ptrs = [dev.room(v) for v in (three.nbytes, m.nbytes, marks.nbytes, rows * G.itemsize, rows * cp * Cy.itemsize)]
        engine.dev_upload(ptrs[0], three)
        engine.dev_upload(ptrs[1], m)
        engine.dev_upload(ptrs[2], np.ascontiguousarray(marks, dtype=np.int32))
        engine.dev_upload(ptrs[3], np.full(rows * G.itemsize, CANARY, dtype=np.uint8))
        engine.dev_upload(ptrs[4], np.full(rows * cp * Cy.itemsize, CANARY, dtype=np.uint8))
        engine.glottal_dev(ptrs[0] + pcm.nbytes, ns, rows, ns, ptrs[1], ptrs[2], mp, ptrs[3], lo, mid, pol, ptrs[4], cp)
        engine.synchronize()
        rec = engine.dev_download(ptrs[3], (rows,), G)
        cyc = engine.dev_download(ptrs[4], (rows, cp), Cy)
    want, wc = gr.glottal(pcm, m, marks, lo, mid, pol, cycles_pitch=cp, cycles_fill=canaries((1,), gr.CYCLE_DTYPE)[0])
    assert_bytes(rec, want, "records")
    assert_bytes(cyc, wc, "cycle records")
    return want, wc


def test_fabricated_marks_give_bad_marks_records_and_touch_nothing(engine):
    n = 600
    meas, marks = fabricated_marks(n)
    assert marks.min() >= -n and marks.max() < 2 * n
    pcm = np.random.default_rng(5).integers(-3000, 3000, size=(len(meas), n)).astype(np.int16)
    want, wc = _foreign(engine, pcm, meas, marks, 26, 128, 1, 4)
    assert want["n_cycles"][0] + want["n_rejected"][0] == 3
    assert np.all(want["status"][1:12] == gr.GL_BAD_MARKS) and np.all(want["status"][12:] == gr.GL_NO_CYCLES)
    assert (wc[1:].view(np.uint8) == CANARY).all()


def test_valid_marks_with_spans_beyond_the_ring(engine):
    """increasing marks nobody measured: spans of more than 4096 samples (read from the row in memory) between short
    ones (read from the ring), through every change from the one to the other; more than 64 marks in a row"""
    n = 40000
    rng = np.random.default_rng(9)
    t = np.arange(n)
    pcm = np.stack([(9000 * np.sin(2 * np.pi * t / (130.0 + 40 * k)) + rng.normal(0, 300, n)).astype(np.int16)
                    for k in range(6)])
    steps = [[150] * 4 + [5000, 150, 150, 4097, 4096, 150, 6000, 7000, 150, 150, 2047, 2049, 2048, 2048, 150],
             [4095, 1, 1, 4095, 1, 4096, 2, 2, 9000, 3],
             [100] * 150,
             [7000, 8000, 9000],
             [2048] * 12,
             [3] * 40 + [20000, 3, 3]]
    mp = 160
    marks = np.full((6, mp), -1, dtype=np.int32)
    meas = np.zeros(6, dtype=ar.DTYPE)
    for i, s in enumerate(steps):
        m = 7 + np.concatenate([[0], np.cumsum(s)])
        assert m[-1] < n
        marks[i, :len(m)] = m
        meas["n_periods"][i] = len(s)
    for lo, mid in LEVELS[:2]:
        want, _ = _foreign(engine, pcm, meas, marks, lo, mid, 1, 150)
        assert np.array_equal(want["n_cycles"] + want["n_rejected"], [len(s) - 1 for s in steps])
        print("spans beyond the ring, levels %d %d: accepted %s rejected %s" % (lo, mid, want["n_cycles"], want["n_rejected"]))
        assert want["n_cycles"].sum() > 20 and want["n_rejected"].sum() > 20


# ---- the two paths

def test_chained_device_path_equals_the_host_path(engine):
    """synthesis into device memory, measure_dev and glottal_dev behind it on the same stream: the PCM never leaves the
    device, and the result is that of vs_glottal on the downloaded PCM"""
    n = 256
    specs, fs, dur, _ = configs.config_specs(2, n)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    A, G, Cy = vs.ACOUSTIC_DTYPE, vs.GLOTTAL_DTYPE, vs.GLOTTAL_CYCLE_DTYPE
    mp, cp = 200, 198
    with engine.scope() as dev:
        plan = dev.plan(lanes, ns)
        ptrs = [dev.room(v) for v in (n * pitch * 2, n * A.itemsize, n * mp * 4, n * G.itemsize, n * cp * Cy.itemsize)]
        engine.dev_upload(ptrs[2], np.full((n, mp), -1, dtype=np.int32))
        engine.dev_upload(ptrs[4], np.zeros((n, cp), dtype=Cy))
        plan.launch(vs.VS_KIND_SYNTH, ptrs[0], pitch)
        engine.measure_dev(ptrs[0], pitch, n, ns, fs, ptrs[1], marks_ptr=ptrs[2], marks_pitch=mp)
        engine.glottal_dev(ptrs[0], pitch, n, ns, ptrs[1], ptrs[2], mp, ptrs[3], cycles_ptr=ptrs[4], cycles_pitch=cp)
        assert plan.status() == 0
        pcm = engine.dev_download(ptrs[0], (n, pitch))[:, :ns]
        marks = engine.dev_download(ptrs[2], (n, mp), np.int32)
        rec = engine.dev_download(ptrs[3], (n,), G)
        cyc = engine.dev_download(ptrs[4], (n, cp), Cy)
    res = engine.glottal(pcm, fs, marks=mp, cycles=cp)
    assert np.array_equal(res["marks"], marks)
    assert_bytes(rec, res["glottal"], "records")
    assert_bytes(cyc, res["cycles"], "cycle records")
    assert rec["n_cycles"].min() > 0


def test_bad_arguments_are_refused(engine):
    pcm = np.zeros((2, 4000), dtype=np.int16)
    for kw in ({"level_open": -1}, {"level_open": 200, "level_mid": 100}, {"level_mid": 256}, {"polarity": 0}, {"marks": 0}):
        with pytest.raises(vs.VsError):
            engine.glottal(pcm, 16000, **kw)
    mo, go = vs.measure_opts(polarity=1), vs.glottal_opts(polarity=-1)      # the two polarities differ
    import ctypes as C
    fs = np.full(2, 16000, dtype=np.int32)
    meas, marks, out = np.zeros(2, vs.ACOUSTIC_DTYPE), np.zeros((2, 8), np.int32), np.zeros(2, vs.GLOTTAL_DTYPE)
    rc = engine._lib.vs_glottal(engine._ctx, C.byref(mo), C.byref(go), pcm.ctypes.data, 4000, 2, 4000, fs.ctypes.data, None,
                                8, meas.ctypes.data, marks.ctypes.data, out.ctypes.data, None, 0)
    assert rc == vs._ffi.VS_ERR_ARG


# ---- bin/glottal

def test_cli_lines_equal_the_restatement(tmp_path):
    files = []
    for k, (fa, va) in enumerate([(["-d", "1", "-j", "1", "-s", "5.76"], ["-v", "a"]),
                                  (["-r", "44100", "-d", "1", "-j", "2", "-f", "100"], ["-v", "i"])]):
        files += _pipeline(tmp_path, "s%d" % k, fa, va, 11 + k)
    for extra, kw in (([], {}), (["-l", "13", "-L", "100", "-c"], {"level_open": 13, "level_mid": 100}),
                      (["-p", "-1", "-f", "60", "-F", "400"], {"polarity": -1, "f0_min": 60.0, "f0_max": 400.0})):
        r = subprocess.run([os.path.join(BIN, "glottal")] + extra + files, cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert lines[0] == "# " + " ".join(gr.COLUMNS)
        want = []
        for f in files:
            x = _payload(tmp_path / f, 44)
            fs = (22050, 44100)[f.startswith("s1")]
            _, _, rec, cyc = gr.measure_and_glottal(x[None, :], fs, cycles_pitch=len(x) // 2, **kw)
            want.append(gr.format_line(f, rec[0]))
            if "-c" in extra:
                want += [gr.format_cycle_line(c) for c in cyc[0, :rec["n_cycles"][0] + rec["n_rejected"][0]]]
        assert lines[1:] == want


def test_cli_bad_files_and_usage(tmp_path):
    _, good = _pipeline(tmp_path, "g", ["-d", "1", "-j", "1"], ["-v", "a"], 5)
    x = _payload(tmp_path / good, 44)
    _wav(tmp_path / "bits8.wav", 22050, x[:4000].astype(np.uint8), bits=8)
    open(tmp_path / "trunc.wav", "wb").write(open(tmp_path / good, "rb").read()[:30])
    r = subprocess.run([os.path.join(BIN, "glottal"), "bits8.wav", good, "trunc.wav", "missing.wav"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 2
    for f in ("bits8.wav", "trunc.wav", "missing.wav"):
        assert f in r.stderr
    lines = r.stdout.splitlines()
    _, _, rec = gr.measure_and_glottal(x[None, :], 22050)
    assert lines[1:] == [gr.format_line(good, rec[0])]
    for bad in (["-l", "300", good], ["-l", "100", "-L", "50", good], ["-p", "2", good], ["-x", good], []):
        assert subprocess.run([os.path.join(BIN, "glottal")] + bad, cwd=tmp_path, capture_output=True).returncode == 1
