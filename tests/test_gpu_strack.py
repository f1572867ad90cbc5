"""The source track on the device (csrc/vs_strack.hip): on a constant track it is vs_source byte for byte (flow, periods,
counts, draws); on drawn tracks -- hostile hops, offsets, lengths, periods and amplitudes -- it is the restatement
(tests/strack_ref.py) byte for byte, flow, status records and cycle records; chained behind the pitch track on the device
it equals the host path; the cap on the rejection loops; the program.  Every output row sits inside a guard band and what
lies past a row's length, its cycles or the pitch keeps its sentinel.  The smallest shapes that can go wrong."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_support as gs  # noqa: E402
import pitch_signals as ps  # noqa: E402
import strack_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voice_synth_amd", "bin")
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
S8 = 0x5A


@pytest.fixture(scope="module")
def eng():
    e = vs.Engine(0)
    yield e
    e.close()


def lane_of(args, seed, fs=None):
    lane = vs.lane_from_cli([a for a in args], ["-v", "a"], seed=seed)[0]
    if fs is not None:
        lane.fs = fs
    return lane


def without_rate(args):
    args = list(args)
    if "-r" in args:
        k = args.index("-r")
        del args[k:k + 2]
    return args


def run_dev(eng, lanes, ns, rows, period, amp=None, cycles_pitch=0, max_reject=256, pad=6, period_stride=4):
    """vs_strack_launch on device pointers: the flow inside a sentinel band at a pitch above n_samples, the status and
    cycle records in sentinel-filled memory.  Returns (flow [n][ns], stat [n], cycles [n][cycles_pitch] or None): what
    the launch did not write is still the sentinel (gpu_support checks the bands and the pitch padding)."""
    n = len(lanes)
    period = np.ascontiguousarray(period, dtype=np.int32)
    fp = period.shape[1]
    pitch = ns + pad
    out = gs.GuardedRows(n, ns, pitch)
    with eng.scope() as dev:
        out.on(dev)
        d_per = dev.put(period)
        d_amp = dev.put(np.ascontiguousarray(amp, dtype=np.int32)) if amp is not None else None
        d_stat = dev.filled(n * vs.STRACK_STAT_DTYPE.itemsize, S8, np.uint8)
        d_cyc = dev.filled(n * cycles_pitch * vs.STRACK_CYCLE_DTYPE.itemsize, S8, np.uint8) if cycles_pitch else None
        eng.source_track_dev(lanes, ns, rows, d_per, period_stride, fp, out.first(pitch), pitch, d_stat, amp_ptr=d_amp,
                             amp_stride=4 if amp is not None else 0, cycles_ptr=d_cyc, cycles_pitch=cycles_pitch,
                             max_reject=max_reject)
        eng.synchronize()
        flow = out.rows_back(pitch).copy()
        stat = dev.get(d_stat, (n,), vs.STRACK_STAT_DTYPE)
        cyc = dev.get(d_cyc, (n, cycles_pitch), vs.STRACK_CYCLE_DTYPE) if cycles_pitch else None
    return flow, stat, cyc


def expected(lanes, ns, rows, period, amp, cycles_pitch, max_reject=256):
    """the restatement's rows over the sentinel: (flow, stat, cycles, full logs)"""
    n = len(lanes)
    flow, stat, _, logs = sr.source_track(lanes, ns, rows, period, amp, max_reject,
                                          out=np.full((n, ns), gs.SENTINEL, dtype=np.int16))
    cyc = np.frombuffer(bytes([S8]) * (n * cycles_pitch * sr.CYCLE_DTYPE.itemsize), dtype=sr.CYCLE_DTYPE)
    cyc = cyc.reshape(n, cycles_pitch).copy()
    for i, log in enumerate(logs):
        k = min(len(log), cycles_pitch)
        cyc[i, :k] = log[:k]
    return flow, stat, cyc, logs


def same_records(got, want, what):
    assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, what
    g, w = got.view(np.uint8).reshape(got.shape + (-1,)), want.view(np.uint8).reshape(want.shape + (-1,))
    bad = np.argwhere((g != w).any(axis=-1))
    assert len(bad) == 0, (what, bad[:6], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 1. a constant track is vs_source ----

@pytest.mark.parametrize("ns", (4097, 6000))
def test_constant_track_is_vs_source(eng, ns):
    lanes, per = [], []
    for fs in (11025, 16000, 22050, 44100):
        for k, args in enumerate(sr.CONSTANT_LANES):
            for seed in range(16):
                lanes.append(lane_of(without_rate(args), 1000 * k + 77 * seed + fs, fs))
                per.append(sr.constant_period(lanes[-1]))
    n, cp = len(lanes), 400
    want, recs, ncyc = eng.source(lanes, ns, log_cycles=cp)
    assert ncyc.max() <= cp and ncyc.min() >= 5
    # frames that differ row by row: the track is constant, f(n) is not
    fp = 9
    period = np.repeat(np.array(per, dtype=np.int32)[:, None], fp, axis=1)
    rows = vs.strack_rows(n, 1 + np.arange(n) % fp, 1)
    rows["hop"] = np.array([1, 160, ns + 5, 37])[np.arange(n) % 4]
    rows["offset"] = np.array([0, 3000, -3000, INT32_MIN, 5])[np.arange(n) % 5]
    rows["length"] = ns
    flow, stat, cyc = run_dev(eng, lanes, ns, rows, period, cycles_pitch=cp)
    gs.same_rows(flow, want, "flow")
    assert np.array_equal(stat["n_cycles"], ncyc) and (stat["status"] == 0).all() and (stat["n_unvoiced"] == 0).all()
    assert (stat["n_resets"] == 0).all()
    for i in range(n):
        k = int(ncyc[i])
        assert np.array_equal(cyc["T"][i, :k], recs["T"][i, :k]), i
        for f in ("S", "x_pow", "w_pow"):
            assert np.array_equal(cyc[f][i, :k].view(np.uint32), recs[f][i, :k].view(np.uint32)), (i, f)
        assert (cyc[i, k:].view(np.uint8) == S8).all(), i
    # the draws: against the oracle's count, on the lanes of one seed
    from oracle import pyoracle
    for i in range(0, n, 16):
        assert int(stat["n_draws"][i]) == pyoracle.source_one(lanes[i], ns)[3], i


# ---- 2. drawn tracks against the restatement ----

TRACK_LANES = (
    [], ["-j", "3"], ["-s", "8"], ["-n", "15"], ["-j", "2", "-s", "6", "-n", "25"], ["-j", "10", "-s", "10", "-n", "10", "-z", "1"],
    ["-l", "0.2", "-z", "0.5", "-c", "0.9"], ["-a", "30000", "-s", "10", "-n", "30"], ["-c", "1", "-j", "10", "-n", "20"],
    ["-l", "0", "-n", "20", "-c", "0.3"], ["-k", "0.5", "-j", "1"], ["-j", "0.05", "-s", "0.05"],
)


def drawn_batch(n=96, ns=4000, fp=64):
    rng = np.random.default_rng(20260)
    lanes, rows = [], vs.strack_rows(n, 1, 1)
    period = np.zeros((n, fp), dtype=np.int32)
    amp = np.zeros((n, fp), dtype=np.int32)
    bad_p = np.array([0, -1, 1, INT32_MIN, INT32_MAX, 2049, 100000])
    bad_a = np.array([-1, 32767, INT32_MIN, INT32_MAX, 40000])
    for i in range(n):
        fs = (11025, 16000, 22050, 44100)[i % 4]
        lanes.append(lane_of(TRACK_LANES[i % len(TRACK_LANES)], 9000 + i, fs))
        pmin, pmax = [(32, 320), (2, 2048), (20, 400), (5, 60)][(i // 4) % 4]
        rows[i] = (int(rng.integers(1, fp + 1)), int(rng.choice([1, 3, 50, 160, 700, ns + 1, 100000, INT32_MAX])),
                   int(rng.choice([0, 0, 17, -3000, 3000, INT32_MIN])), int(rng.choice([ns, ns, ns - 1, 2500, 777, 1, 0])),
                   pmin, pmax)
        p = np.exp(rng.uniform(np.log(pmin), np.log(pmax + 1), fp)).astype(np.int64).clip(pmin, pmax)
        if i % 3 == 0:      # a contour instead of independent frames
            p = np.sort(p)[::-1] if i % 2 else np.sort(p)
        hole = rng.random(fp) < 0.2
        p[hole] = np.concatenate([bad_p, [pmin - 1, pmax + 1]])[rng.integers(0, len(bad_p) + 2, hole.sum())]
        period[i] = p
        a = rng.integers(0, 32767, fp)
        hole = rng.random(fp) < 0.15
        a[hole] = bad_a[rng.integers(0, len(bad_a), hole.sum())]
        amp[i] = a
    # the longest cos row and the longest cycle: pmax 2048 at 44100 Hz, cq 1, jitter 10 %
    lanes[3] = lane_of(["-c", "1", "-j", "10", "-n", "20"], 31, 44100)
    rows[3] = (4, 1500, 0, ns, 2, 2048)
    period[3, :4] = (2048, 2048, 2047, 2048)
    amp[3, :4] = (12000, 32766, 500, 12000)
    # a period of 2, and the whole row voiced
    lanes[5] = lane_of(["-j", "10", "-s", "5", "-n", "20"], 32, 16000)
    rows[5] = (2, 900, 0, 1800, 2, 2048)
    period[5, :2] = (2, 3)
    amp[5, :2] = (9000, 12000)
    return lanes, ns, rows, period, amp


@pytest.fixture(scope="module")
def drawn():
    lanes, ns, rows, period, amp = drawn_batch()
    cp = 40
    return dict(lanes=lanes, ns=ns, rows=rows, period=period, amp=amp, cp=cp,
                plain=expected(lanes, ns, rows, period, None, cp), with_amp=expected(lanes, ns, rows, period, amp, cp))


@pytest.mark.parametrize("which", ("plain", "with_amp"))
def test_drawn_tracks_are_the_restatements(eng, drawn, which):
    d = drawn
    amp = d["amp"] if which == "with_amp" else None
    wflow, wstat, wcyc, logs = d[which]
    flow, stat, cyc = run_dev(eng, d["lanes"], d["ns"], d["rows"], d["period"], amp, cycles_pitch=d["cp"])
    same_records(stat, wstat, "stat")
    gs.same_rows(flow, wflow, "flow")
    same_records(cyc, wcyc, "cycles")
    # the batch is what it claims to be: logs that are cut and logs that are not, rows without a cycle, both
    # kinds of stretch, a cycle longer than the longest period, a period of 2
    ncyc = wstat["n_cycles"]
    assert (ncyc > d["cp"]).any() and ((ncyc > 0) & (ncyc < d["cp"])).any() and (ncyc == 0).any()
    assert (wstat["n_unvoiced"] > 0).any() and (wstat["status"] & 2 == 0).all()
    assert max(int(l["T"].max()) for l in logs if len(l)) > 2048 and int(logs[5]["T"].min()) == 2
    # without a log the flow and the counts are the same
    flow2, stat2, _ = run_dev(eng, d["lanes"], d["ns"], d["rows"], d["period"], amp, pad=0)
    gs.same_rows(flow2, wflow, "flow without a log")
    same_records(stat2, wstat, "stat without a log")


def test_the_host_path_is_the_device_path(eng, drawn):
    d = drawn
    wflow, wstat, wcyc, _ = d["with_amp"]
    out = np.full((len(d["lanes"]), d["ns"]), gs.SENTINEL, dtype=np.int16)
    r = d["rows"]
    flow, stat, cyc = eng.source_track(d["lanes"], d["ns"], d["period"], r["hop"], r["offset"], r["n_frames"], r["length"],
                                       r["pmin"], r["pmax"], amp=d["amp"], log_cycles=d["cp"], out=out)
    gs.same_rows(flow, wflow, "flow")
    same_records(stat, wstat.astype(vs.STRACK_STAT_DTYPE), "stat")
    for i in range(len(d["lanes"])):
        k = min(int(wstat["n_cycles"][i]), d["cp"])
        assert cyc[i, :k].tobytes() == wcyc[i, :k].tobytes() and (cyc["start"][i, k:] == -1).all(), i


# ---- 3. chained on the device behind the pitch track ----

def test_chained_behind_the_pitch_track(eng):
    n, ns, fs = 64, 3000, 16000
    models, _ = vs.lanes_from_specs([(["-r", "16000", "-f", "%d" % (60 + k), "-j", "1"], ["-v", "a"], k) for k in range(n)])
    pcm = eng.source(models, ns)
    pcm[5] = 0                    # a row without a voiced frame
    pcm[6, 1200:] = 0             # a row that ends unvoiced
    row = vs.strack_row_from_pitch(fs, ns)
    fp = int(row["n_frames"])
    assert fp == 13
    lanes = [lane_of(TRACK_LANES[k % len(TRACK_LANES)] + ["-r", "16000"], 500 + k) for k in range(n)]
    out = gs.GuardedRows(n, ns, ns + 2)
    with eng.scope() as dev:
        out.on(dev)
        d_pcm = dev.put(pcm)
        d_fr = dev.put(np.zeros((n, fp), vs.PITCH_FRAME_DTYPE))
        d_stat = dev.room(n * vs.STRACK_STAT_DTYPE.itemsize)
        eng.pitch_dev(d_pcm, ns, n, ns, fs, fp, d_fr)
        lag_at = vs.PITCH_FRAME_DTYPE.fields["lag"][1]
        assert lag_at == 12 and vs.PITCH_FRAME_DTYPE.itemsize == 96
        eng.source_track_dev(lanes, ns, row, d_fr + lag_at, 96, fp, out.first(ns + 2), ns + 2, d_stat)
        eng.synchronize()
        flow = out.rows_back(ns + 2).copy()
        stat = dev.get(d_stat, (n,), vs.STRACK_STAT_DTYPE)
        frames = dev.get(d_fr, (n, fp), vs.PITCH_FRAME_DTYPE)
    lags = np.ascontiguousarray(frames["lag"])
    hflow, hstat = eng.source_track(lanes, ns, lags, int(row["hop"]), int(row["offset"]), pmin=int(row["pmin"]),
                                    pmax=int(row["pmax"]))
    gs.same_rows(flow, hflow, "flow")
    same_records(stat, hstat, "stat")
    assert stat["status"][5] == vs.VS_ST_NO_VOICED and (flow[5] == 0).all() and stat["n_unvoiced"][6] > 0
    assert (stat["n_cycles"][np.arange(n) != 5] > 0).all()
    # and the host path is the restatement
    wflow, wstat, _, _ = sr.source_track(lanes[:8], ns, [row] * 8, lags[:8])
    gs.same_rows(hflow[:8], wflow, "restatement")
    same_records(hstat[:8], wstat.astype(vs.STRACK_STAT_DTYPE), "restatement's stat")


# ---- 4. the cap on the rejection loops ----

def test_max_reject_resets_like_the_restatement(eng):
    ns = 3000
    lanes = [lane_of(["-j", "1000", "-s", str(s), "-r", "16000"], 40 + k) for k, s in enumerate((0, 0, 50, 100, 0, 7))]
    n = len(lanes)
    rows = vs.strack_rows(n, 3, 1000, 0, ns, 32, 320)
    period = np.tile(np.array([160, 80, 240], dtype=np.int32), (n, 1))
    for mr in (4, 1):
        flow, stat, cyc = run_dev(eng, lanes, ns, rows, period, cycles_pitch=80, max_reject=mr)
        wflow, wstat, wcyc, _ = expected(lanes, ns, rows, period, None, 80, max_reject=mr)
        same_records(stat, wstat, "stat")
        gs.same_rows(flow, wflow, "flow")
        same_records(cyc, wcyc, "cycles")
        assert (wstat["n_resets"] > 0).all()


# ---- refusals ----

def test_refusals(eng):
    lane = lane_of(["-r", "16000"], 1)
    per = np.full((1, 4), 100, dtype=np.int32)

    def rc(**kw):
        a = dict(hop=100, offset=0, n_frames=4, lengths=500, pmin=32, pmax=320, max_reject=256)
        a.update(kw)
        with pytest.raises(vs.VsError) as e:
            eng.source_track([lane], 500, per, a["hop"], a["offset"], a["n_frames"], a["lengths"], a["pmin"], a["pmax"],
                             max_reject=a["max_reject"])
        return e.value.code
    R = vs._ffi.VS_ERR_RANGE
    assert rc(n_frames=0) == R and rc(n_frames=5) == R and rc(hop=0) == R and rc(lengths=501) == R and rc(lengths=-1) == R
    assert rc(pmin=1) == R and rc(pmax=2049) == R and rc(pmin=321) == R and rc(max_reject=0) == R and rc(max_reject=65537) == R
    flow, stat = eng.source_track([lane], 500, per, 100, INT32_MIN, max_reject=65536)
    assert stat["n_cycles"][0] == 5
    lane.cq = 0.0
    assert rc() == vs._ffi.VS_ERR_UNSUPPORTED      # vs_lane_validate's answer


# ---- 5. the program ----

def _wav(path, fs, x):
    data = np.ascontiguousarray(x, dtype=np.int16).tobytes()
    h = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, 1, 1, fs, fs * 2, 2, 16, b"data",
                    len(data))
    open(path, "wb").write(h + data)


def _payload(path, header=44):
    return np.frombuffer(open(path, "rb").read()[header:], dtype=np.int16)


def _vsource(tmp_path, *args, seed="77"):
    env = dict(os.environ, VS_SEED=seed, VS_WAV_HEADER="44")
    return subprocess.run([os.path.join(BIN, "vsource")] + list(args), cwd=tmp_path, capture_output=True, text=True,
                          timeout=120, env=env)


def test_the_program(eng, tmp_path):
    """vsource -M, -M -A and -C: the file is the Engine's rows, the summary line its counts; a bad file gives 2"""
    fs = 16000
    x = ps.gaps()
    _wav(str(tmp_path / "model.wav"), fs, x)
    frames, nfr = eng.pitch(x[None], fs)
    fr = frames[0, :nfr[0]]
    row = vs.strack_row_from_pitch(fs, len(x))
    lags = np.ascontiguousarray(fr["lag"])[None]
    opts = ["-j", "1", "-s", "4", "-n", "25", "-a", "9000", "-c", "0.6"]
    lane = lane_of(opts + ["-r", "16000"], 77)
    r0 = fr["r0"].astype(np.float64)
    amps = np.floor(9000.0 * np.sqrt(r0 / float(fr["r0"].max())) + 0.5).astype(np.int32)[None]
    for extra, amp in (([], None), (["-A"], amps)):
        r = _vsource(tmp_path, "-o", "flow.wav", "-M", "model.wav", *extra, *opts)
        assert r.returncode == 0, r.stderr
        want, stat = eng.source_track([lane], len(x), lags, int(row["hop"]), int(row["offset"]), pmin=int(row["pmin"]),
                                      pmax=int(row["pmax"]), amp=amp)
        got = open(tmp_path / "flow.wav", "rb").read()
        assert got[:44] == open(tmp_path / "model.wav", "rb").read()[:44]
        assert np.array_equal(_payload(tmp_path / "flow.wav"), want[0])
        voiced = (lags[0] >= row["pmin"]) & (lags[0] <= row["pmax"])
        assert r.stdout.split() == ["flow.wav", str(nfr[0]), str(int(voiced.sum())), str(stat["n_cycles"][0]),
                                    str(stat["n_resets"][0]), str(stat["status"][0])]
        assert stat["n_cycles"][0] > 100 and stat["n_unvoiced"][0] > 8000
    # -C: three anchors over half a second at 22050 Hz (the reference's default rate), a hop of 5 ms
    r = _vsource(tmp_path, "-o", "glide.wav", "-C", "120,180.5,90", "-T", "5", "-d", "0.5", "-j", "2", seed="5")
    assert r.returncode == 0, r.stderr
    fs, f0s = 22050, (120.0, 180.5, 90.0)
    N = vs.num_samples(fs, 0.5)
    H = int(np.floor(0.005 * fs + 0.5))
    F = -(-N // H)
    per = []
    for f in range(F):
        c = min(f * H + H // 2, N)
        u = float(c) * 2.0 / float(N)
        k = min(int(u), 1)
        per.append(int(float(fs) / (f0s[k] + (u - k) * (f0s[k + 1] - f0s[k]))))
    want, stat = eng.source_track([lane_of(["-j", "2"], 5)], N, np.array(per, dtype=np.int32)[None], H, 0, pmin=fs // 500,
                                  pmax=-(-fs // 50))
    assert np.array_equal(_payload(tmp_path / "glide.wav"), want[0])
    assert r.stdout.split() == ["glide.wav", str(F), str(F), str(stat["n_cycles"][0]), "0", "0"]
    assert min(per) == int(22050 / 180.5) or min(per) == int(22050 / 180.5) + 1
    # refusals
    open(tmp_path / "bad.wav", "wb").write(b"RIFF")
    assert _vsource(tmp_path, "-o", "o.wav", "-M", "bad.wav").returncode == 2
    assert _vsource(tmp_path, "-o", "o.wav", "-M", "none.wav").returncode == 2
    _wav(str(tmp_path / "short.wav"), 16000, np.zeros(100, np.int16))
    assert _vsource(tmp_path, "-o", "o.wav", "-M", "short.wav").returncode == 2
    for bad in (["-o", "o.wav"], ["-o", "o.wav", "-C", "100"], ["-o", "o.wav", "-C", "100,200", "-f", "100"],
                ["-o", "o.wav", "-C", "100,200", "-g", "200"], ["-o", "o.wav", "-C", "100,200", "-A"],
                ["-o", "o.wav", "-C", "100,200", "-M", "model.wav"], ["-C", "100,200"]):
        assert _vsource(tmp_path, *bad).returncode == 1, bad
