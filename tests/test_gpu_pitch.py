"""The pitch track on the device (csrc/vs_pitch.hip) against its numpy restatement (tests/pitch_ref.py): every field of
every frame record byte for byte, nothing written past a row's frames, at the smallest shapes that can go wrong."""
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
import hostile_signals as hs  # noqa: E402
import pitch_ref as pr  # noqa: E402
import pitch_signals as ps  # noqa: E402

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voice_synth_amd", "bin")
FILL = 0xA5


@pytest.fixture(scope="module")
def eng():
    e = vs.Engine(0)
    yield e
    e.close()


def filled(n, fp):
    return np.frombuffer(bytes([FILL]) * (n * fp * 96), dtype=vs.PITCH_FRAME_DTYPE).reshape(n, fp).copy()


def compare(eng, pcm, fs, lengths=None, extra=3, **opts):
    """the host-buffer call on records filled with a pattern, at a frames_pitch above every n_frames: the whole array
    equals the restatement's, the pattern past every row's frames included"""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    want0, nfr = pr.track(pcm, fs, lengths, **opts)
    fp = max(1, int(nfr.max())) + extra
    fill = filled(pcm.shape[0], fp)
    want, _ = pr.track(pcm, fs, lengths, frames_pitch=fp, fill=fill, **opts)
    got, gn = eng.pitch(pcm, fs, lengths=lengths, frames=fill, **opts)
    assert np.array_equal(gn, nfr)
    for name in pr.FRAME_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:6])
    gs.same_bits(got.view(np.uint8), want.astype(vs.PITCH_FRAME_DTYPE).view(np.uint8))
    return want, nfr


def rows_of(n, ns, fs=16000, seed=0):
    """n rows of ns samples: the hostile bank and the constructed signals, in turn"""
    pool = list(hs.bank(fs, ns, seed).values())
    for sig in (ps.glide()[0], ps.gaps(), ps.octave_trap(), ps.subharmonic()):
        row = np.zeros(ns, np.int16)
        row[:min(ns, len(sig))] = sig[:ns]
        pool.append(row)
    return np.stack([pool[k % len(pool)] for k in range(n)])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_rows_and_ragged_lengths(eng, n):
    ns = 4000
    pcm = rows_of(n, ns)
    rng = np.random.default_rng(n)
    lengths = rng.integers(900, ns + 1, n).astype(np.int32)
    lengths[0] = ns
    want, nfr = compare(eng, pcm, 16000, lengths)
    assert nfr.max() == 19 and (n < 3 or nfr.min() < nfr.max())


def test_the_constructed_signals_whole(eng):
    sigs = [ps.glide()[0], ps.gaps(), ps.octave_trap(), ps.subharmonic()]
    ns = max(len(s) for s in sigs)
    pcm = np.zeros((4, ns), np.int16)
    for i, s in enumerate(sigs):
        pcm[i, :len(s)] = s
    want, nfr = compare(eng, pcm, 16000, np.array([len(s) for s in sigs], np.int32))
    assert (want[2, :nfr[2]]["lag"] == 160).all() and (want[3, :nfr[3]]["lag"] == 200).all()
    compare(eng, pcm[3:4], 16000, octave_q=3277)


def test_the_lengths_around_a_frame(eng):
    tmin, tmax = ar.lag_bounds(16000)
    base, H = 3 * tmax + 2, 160
    lengths = np.array([0, base - 1, base, base + H - 1, base + H], np.int32)
    pcm = rows_of(5, base + H, seed=3)
    want, nfr = compare(eng, pcm, 16000, lengths)
    assert nfr.tolist() == [0, 0, 1, 1, 2]


def test_four_rates_in_one_call(eng):
    fs = np.array([8000, 16000, 22050, 44100], np.int32)
    ns = 6000
    pcm = np.stack([hs.bank(int(f), ns, 7)[k] for f, k in zip(fs, ("noise_full", "constant", "noise_small", "noise_full"))])
    t = np.arange(ns)
    pcm[2] = np.round(9000 * np.sin(2 * np.pi * t / 147.0) + 3000 * np.sin(2 * np.pi * t / 49.0)).astype(np.int16)
    want, nfr = compare(eng, pcm, fs)
    assert (want[3, :nfr[3]]["n_cand"] == 7).all()              # noise at 44100 Hz: more than 7 local maxima
    assert (want[1, :nfr[1]]["n_cand"] == 0).all() and (want[1, :nfr[1]]["status"] == 6).all()   # a constant: no candidate


def test_the_largest_lag_range(eng):
    """96000 Hz with f0_min 47: tmax 2043, the largest LDS"""
    tmin, tmax = ar.lag_bounds(96000, 47.0)
    assert tmax == 2043
    ns = 3 * tmax + 2 + 960
    x, _ = ps.train([1311] * 6, lambda p: 700, lambda c: 9000.0)
    want, nfr = compare(eng, x[None, :ns], 96000, f0_min=47.0)
    assert nfr.tolist() == [2] and (want[0, :2]["lag"] == 1311).all()


def test_seven_lags(eng):
    """F0 400..500 Hz at 8000 Hz: tmin 16, tmax 20"""
    assert ar.lag_bounds(8000, 400.0, 500.0) == (16, 20)
    ns = 700
    t = np.arange(ns)
    pcm = np.stack([np.round(8000 * np.sin(2 * np.pi * t / 18.0)).astype(np.int16), hs.bank(8000, ns, 2)["noise_full"],
                    np.where((t // 9) % 2 == 0, 32767, -32767).astype(np.int16)])
    want, nfr = compare(eng, pcm, 8000, f0_min=400.0, f0_max=500.0)
    assert (want[0, :nfr[0]]["lag"] == 18).all() and (want[2, :nfr[2]]["q"] == 32768).all()


def test_a_long_path(eng):
    """hop 1 ms on 16000 samples: 940 frames, with voiced and unvoiced stretches"""
    x = np.zeros(16000, np.int16)
    g = ps.gaps()
    x[:len(g[:16000])] = g[:16000]
    want, nfr = compare(eng, x[None], 16000, hop_s=0.001)
    assert nfr.tolist() == [940]
    v = want[0]["lag"][:940] > 0
    assert v.any() and (~v).any()


def test_full_scale_and_ties(eng):
    t = np.arange(3000)
    pcm = np.stack([np.where((t // 20) % 2 == 0, 32767, -32767), np.where((t // 25) % 2 == 0, 32767, -32768),
                    np.full(3000, -32768), np.zeros(3000), np.where((t // 40) % 2 == 0, 1, -1)]).astype(np.int16)
    want, nfr = compare(eng, pcm, 8000)
    assert (want[0, :nfr[0]]["q"] == 32768).all() and (want[0, :nfr[0]]["n_cand"] >= 2).all()   # ties at 40, 80, 120
    assert (want[3, :nfr[3]]["status"] == 3).all()                                                # zeros: silent
    compare(eng, pcm, 8000, silence_rms=0)


@pytest.mark.parametrize("name", ["voicing_q", "octave_q", "jump_q", "vuv_q"])
def test_every_cost_at_its_ends(eng, name):
    pcm = rows_of(13, 3000, seed=11)
    for v in (0, 1 << 20):
        compare(eng, pcm, 16000, **{name: v})


def test_device_pointers_and_guards(eng):
    """vs_pitch_launch behind an upload on the context's stream, at a frames_pitch above every n_frames and two bases:
    nothing in front of, between or behind the rows' records is written"""
    n, ns = 5, 3000
    pcm = rows_of(n, ns, seed=4)
    lengths = np.array([3000, 961, 0, 2000, 1500], np.int32)
    want0, nfr = pr.track(pcm, 16000, lengths)
    fp = int(nfr.max()) + 2
    sentinel = 0x5A5A5A5A5A5A5A5A
    with eng.scope() as dev:
        src = dev.put(pcm)
        g = gs.GuardedRows(n, fp * 12, fp * 12 + 24, 64, sentinel, np.int64).on(dev)
        for pitch, off in ((fp * 12, 0), (fp * 12 + 24, 64)):
            g.fill()
            eng.pitch_dev(src, ns, n, ns, 16000, pitch // 12, g.first(pitch, off), lengths=lengths)
            eng.synchronize()
            body = g.rows_back(pitch, off, "pitch %d" % pitch)
            fill = np.full((n, fp * 12), sentinel, np.int64).view(vs.PITCH_FRAME_DTYPE).reshape(n, fp)
            want, _ = pr.track(pcm, 16000, lengths, frames_pitch=fp, fill=fill)
            gs.same_bits(np.ascontiguousarray(body).view(np.uint8), want.view(np.uint8).reshape(n, -1))


def test_refusals(eng):
    pcm = rows_of(2, 2000)
    with pytest.raises(vs.VsError) as e:
        eng.pitch(pcm, 16000, frames=3)                       # a row with more frames than frames_pitch
    assert e.value.code == vs._ffi.VS_ERR_RANGE
    with pytest.raises(vs.VsError) as e:
        eng.pitch(pcm, 16000, jump_q=(1 << 20) + 1)
    assert e.value.code == vs._ffi.VS_ERR_ARG
    with pytest.raises(vs.VsError) as e:
        eng.pitch(pcm, [16000, 3], frames=20)
    assert e.value.code == vs._ffi.VS_ERR_RANGE


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


def test_the_program(eng, tmp_path):
    sigs = {"glide.wav": (ps.glide()[0], 16000, 44), "gaps.wav": (ps.gaps(), 16000, 72),
            "noise.wav": (hs.bank(22050, 5000, 1)["noise_full"], 22050, 44), "short.wav": (np.zeros(100, np.int16), 8000, 72)}
    for name, (x, fs, header) in sigs.items():
        _wav(str(tmp_path / name), fs, x, header)
    open(str(tmp_path / "bad.wav"), "wb").write(b"RIFF")
    r = subprocess.run([os.path.join(BIN, "pitch"), "-l"] + list(sigs), cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    want = ["# file frames voiced segments F0_mean_Hz F0_min_Hz F0_max_Hz status"]
    for name, (x, fs, header) in sigs.items():
        rec, nfr = eng.pitch(x[None], fs)
        rec = rec[0, :nfr[0]]
        want.append(pr.format_line(name, rec, fs))
        want += [pr.format_frame(name, f) for f in rec]
    assert r.stdout.splitlines() == want
    r = subprocess.run([os.path.join(BIN, "pitch"), "-V", "0.3", "-J", "0.2", "-t", "5", "-f", "70", "-F", "400", "-O", "0.1",
                        "-U", "0.2", "-S", "30", "bad.wav", "gaps.wav"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "bad.wav" in r.stderr
    x, fs, _ = sigs["gaps.wav"]
    rec, nfr = eng.pitch(x[None], fs, voicing_q=9830, jump_q=6554, hop_s=0.005, f0_min=70.0, f0_max=400.0, octave_q=3277,
                         vuv_q=6554, silence_rms=30)
    assert r.stdout.splitlines()[1:] == [pr.format_line("gaps.wav", rec[0, :nfr[0]], fs)]
    assert subprocess.run([os.path.join(BIN, "pitch"), "-V", "40", "gaps.wav"], cwd=tmp_path, capture_output=True).returncode == 1
