"""The coefficient tracks on the device (vs_track / vs_track_launch, bin/vtrack) against their numpy restatement
(tests/track_ref.py), byte for byte in VS_ARITH_EXACT: hold mode with one set is vs_filter; hold and glide tracks with
per-row hops, offsets, set counts and lengths; unusable sets; the launch chained behind the LPC analysis on the device;
glides that end on the formants of their end tables; the FMA form within 1 LSB; the program; one full-size launch."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as tr  # noqa: E402
from test_track_ref import SPEECH_TOL_HZ, TRUTH_PAIRS, plateau_errors, truth_anchors  # noqa: E402

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(vs.__file__), "bin")
TABLES = "aiu1234567"
SEED = 20240607        # the generator of every drawn track below; tr.filter_track's state_max is checked where it is used
STATE_MAX = 1e12


def _lanes(index, n=None):
    specs, fs, dur, _ = configs.config_specs(index, n)
    lanes, d = vs.lanes_from_specs(specs)
    return lanes, vs.num_samples(fs, d)


_flows = {}


def _test_flows(engine):
    """config 2 in full, the first 512 rows of config 3 and of config 5: 2048 flows of 16000 samples"""
    if "all" not in _flows:
        parts = []
        for index, n in ((2, None), (3, 512), (5, 512)):
            lanes, ns = _lanes(index, n)
            parts.append(engine.source(lanes, ns))
        _flows["all"] = np.concatenate(parts)
    return _flows["all"]


def _table_reflections():
    return np.array([tr.reflection(vs.vowel_coefficients(v))[0] for v in TABLES])


def _blend_sets(rng, n, K, order):
    """[n][K][order+1]: random convex blends of two tables in the reflection domain (every |k_i| < 1: stable); order < 22
    keeps the first reflection coefficients, order > 22 appends small ones"""
    kt = _table_reflections()
    a, b = rng.integers(0, 10, (n, K)), rng.integers(0, 10, (n, K))
    w = rng.uniform(0, 1, (n, K, 1))
    k = w * kt[a] + (1.0 - w) * kt[b]
    if order <= 22:
        k = k[..., :order]
    else:
        k = np.concatenate([k, rng.uniform(-0.2, 0.2, (n, K, order - 22))], axis=-1)
    return tr.step_up(k)


def _drawn_rows(rng, n, K, ns):
    rows = np.zeros(n, dtype=tr.ROW_DTYPE)
    rows["n_sets"] = rng.integers(1, K + 1, n)
    rows["hop"] = rng.integers(1, max(2, 2 * ns // K), n)
    rows["offset"] = rng.integers(-3000, 3000, n)
    rows["length"] = np.where(rng.uniform(size=n) < 0.3, rng.integers(0, ns + 1, n), ns)
    rows["gain"] = rng.uniform(0.5, 4.0, n).astype(np.float32)
    rows["pre_emphasis"] = rng.choice([0.0, 1.0, 0.37, 0.9], n).astype(np.float32)
    # the corners: hop 1, hop > n_samples, offsets far outside the row on both sides, all sets, an empty row
    rows["hop"][0], rows["hop"][1] = 1, ns + 4000
    rows["offset"][2], rows["offset"][3], rows["offset"][4] = -5000, ns + 1000, -2147483648
    rows["hop"][4], rows["n_sets"][4] = 2147483647, K
    rows["n_sets"][:4] = K
    rows["length"][5], rows["length"][:5] = 0, ns
    return rows


def _device(engine, flow, coefs, rows, mode, gains=None, out=None):
    return engine.filter_track(flow, coefs, rows["hop"], rows["offset"], rows["n_sets"], rows["length"], rows["gain"],
                               rows["pre_emphasis"], mode, gains, out)


def _assert_same(got, want):
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:8]
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:8]


# 1 ---- hold mode with one set is vs_filter

@pytest.mark.parametrize("ns", [16000, 16001, 4097])
def test_hold_with_one_set_is_vs_filter(engine, ns):
    lanes = []
    for k, v in enumerate(TABLES):
        for r in range(64):
            lanes.append(vs.lane_from_cli(["-r", "16000", "-d", "2", "-j", "1", "-s", "5.76", "-n", "20"],
                                          ["-v", v, "-g", "%g" % (1 + 0.1 * r), "-p", ["1", "0", "0.37", "0.9"][r % 4]],
                                          100 * k + r)[0])
    flow = engine.source(lanes, ns)
    want = engine.filter(lanes, flow)
    coefs = np.array([vs.vowel_coefficients(v) for v in TABLES]).repeat(64, axis=0)[:, None, :]
    got, stat = engine.filter_track(flow, coefs, hop=160, gain=[l.gain for l in lanes],
                                    pre_emphasis=[l.pre_emphasis for l in lanes])
    assert np.array_equal(got, want) and not stat["status"].any() and not stat["n_unusable"].any()
    rng = np.random.default_rng(SEED)
    for order in (1, 12, 23, 40):
        A = np.array([configs.random_pole_set(order, rng) for _ in range(16)])
        custom = [vs.set_coefficients(lanes[r], A[r]) for r in range(16)]
        want = engine.filter(custom, flow[:16])
        got, stat = engine.filter_track(flow[:16], A[:, None, :], hop=7, offset=-3, gain=[l.gain for l in custom],
                                        pre_emphasis=[l.pre_emphasis for l in custom])
        assert np.array_equal(got, want), order
        assert np.abs(want.astype(np.int32)).max() > 100


def test_hold_with_one_set_is_vs_filter_on_config2_in_full(engine):
    lanes, ns = _lanes(2)
    flow = engine.source(lanes, ns)
    coefs = np.broadcast_to(vs.vowel_coefficients("a"), (len(lanes), 1, 23))
    got, stat = engine.filter_track(flow, coefs, hop=1, gain=lanes[0].gain, pre_emphasis=lanes[0].pre_emphasis)
    assert np.array_equal(got, engine.filter(lanes, flow)) and not stat["status"].any()


# 2 ---- hold tracks against the restatement

@pytest.mark.parametrize("K", [1, 2, 7, 100])
def test_hold_tracks_equal_the_restatement(engine, K):
    flow = _test_flows(engine)
    n, ns = flow.shape
    rng = np.random.default_rng(SEED + K)
    coefs = _blend_sets(rng, n, K, 22)
    rows = _drawn_rows(rng, n, K, ns)
    peak = []
    want = tr.filter_track(flow, coefs, rows, tr.HOLD, state_max=peak)
    assert peak[0] < STATE_MAX
    _assert_same(_device(engine, flow, coefs, rows, "hold"), want)
    assert not want[1]["status"].any() and not want[1]["n_unusable"].any()


# 3 ---- unusable sets, forward fill, untouched samples

@pytest.mark.parametrize("mode", ["hold", "glide"])
def test_unusable_sets_and_samples_past_the_length(engine, mode):
    flow = _test_flows(engine)[1000:1064]
    n, ns = flow.shape
    K = 9
    rng = np.random.default_rng(SEED + 3)
    coefs = _blend_sets(rng, n, K, 22)
    gains = rng.uniform(0.5, 2.0, (n, K))
    coefs[0, :3, 1:] = np.nan                    # at the start: E_0..E_2 are the first usable set
    coefs[1, 4, 7] = np.nan                      # in the middle
    coefs[2, K - 1, 1] = np.inf                  # at the end
    coefs[3, :, 22] = np.nan                     # no usable set at all
    coefs[4, 2:7, 3] = np.nan
    gains[5, 3] = np.nan                         # an unusable gain
    coefs[6, 0, 1:] = np.nan
    coefs[6, 5, 1:] = np.nan
    coefs[7, 2] = np.concatenate([[1.0], np.zeros(21), [1.25]])      # finite, |k_22| >= 1: unusable in glide mode only
    coefs[8, :, 1:] = 0.0
    coefs[8, :, 22] = np.where(np.arange(K) % 2, 1.0, -1.0)          # ... |k_22| = 1 in every set: VS_TRACK_NO_SET there
    rows = _drawn_rows(rng, n, K, ns)
    rows["n_sets"] = K
    rows["hop"][:16] = 1500
    rows["offset"][:16] = 100
    rows["length"][:16] = np.where(np.arange(16) % 2, ns, ns - 777)
    rows["n_sets"][9] = 3
    coefs[9, 3:, 5] = np.nan                     # beyond n_sets: not counted
    m = tr.HOLD if mode == "hold" else tr.GLIDE
    if mode == "hold":                           # row 8's poles lie on the unit circle there: it filters silence
        flow = flow.copy()
        flow[8] = 0
    sentinel = np.full((n, ns), 0x5A5A, dtype=np.int16)
    for g in (None, gains):
        want = tr.filter_track(flow, coefs, rows, m, g, out=sentinel)
        got = _device(engine, flow, coefs, rows, mode, g, out=sentinel)
        _assert_same(got, want)
        st = got[1]
        glide = mode == "glide"
        assert list(st["n_unusable"][:5]) == [3, 1, 1, K, 5] and st["n_unusable"][6] == 2 and st["n_unusable"][9] == 0
        assert st["n_unusable"][5] == (1 if g is not None else 0)
        assert st["n_unusable"][7] == (1 if glide else 0) and st["n_unusable"][8] == (K if glide else 0)
        assert st["status"][3] == vs.VS_TRACK_NO_SET and st["status"][8] == (vs.VS_TRACK_NO_SET if glide else 0)
        assert st["status"].sum() == (2 if glide else 1)
        assert not got[0][3, :rows["length"][3]].any()
        for r in range(n):
            assert (got[0][r, rows["length"][r]:] == 0x5A5A).all()


# 4 ---- glide tracks against the restatement

@pytest.mark.parametrize("order", [12, 22, 40])
@pytest.mark.parametrize("K", [1, 2, 11, 100])
def test_glide_tracks_equal_the_restatement(engine, order, K):
    flow = _test_flows(engine)
    n, ns = flow.shape
    rng = np.random.default_rng(SEED + 1000 * order + K)
    coefs = _blend_sets(rng, n, K, order)
    rows = _drawn_rows(rng, n, K, ns)
    for gains in (None, rng.uniform(0.25, 2.0, (n, K))):
        peak = []
        want = tr.filter_track(flow, coefs, rows, tr.GLIDE, gains, state_max=peak)
        assert peak[0] < STATE_MAX
        _assert_same(_device(engine, flow, coefs, rows, "glide", gains), want)
        assert not want[1]["status"].any() and not want[1]["n_unusable"].any()


# 5 ---- chained on the device behind the analysis

@pytest.mark.parametrize("mode", ["hold", "glide"])
def test_device_chained_copy_synthesis_equals_the_host_path(engine, mode):
    lanes, ns = _lanes(2)
    n, fs = len(lanes), 16000
    pitch = vs.row_pitch(ns)
    opts = dict(n_formants=0)
    nfr = vs.lpc_frames(fs, ns, **opts)
    row = vs.track_from_lpc(fs, ns, mode, **opts)
    with engine.scope() as dev:
        plan = dev.plan(lanes, ns)
        flow_d, pcm_d, out_d = (dev.room(n * pitch * 2) for _ in range(3))
        fr_d, cf_d, st_d = dev.room(n * nfr * 32), dev.room(n * nfr * 23 * 8), dev.room(n * 8)
        engine.dev_upload(out_d, np.zeros((n, pitch), dtype=np.int16))
        plan.launch(vs.VS_KIND_SOURCE, flow_d, pitch)
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        engine.lpc_dev(pcm_d, pitch, n, ns, fs, nfr, fr_d, None, cf_d, **opts)
        engine.filter_track_dev(mode, 22, flow_d, pitch, out_d, pitch, n, ns, row, cf_d, nfr, stat_ptr=st_d)
        assert plan.status() == 0
        flow = engine.dev_download(flow_d, (n, pitch))[:, :ns]
        pcm = engine.dev_download(pcm_d, (n, pitch))[:, :ns]
        out = engine.dev_download(out_d, (n, pitch))[:, :ns]
        st = engine.dev_download(st_d, (n,), vs.TRACK_STAT_DTYPE)
    coefs = engine.lpc(pcm, fs, coefs=True, **opts)["coefs"]
    assert coefs.shape == (n, nfr, 23) and row["n_sets"] == nfr
    want = engine.filter_track(flow, coefs, row["hop"], row["offset"], mode=mode)
    assert np.array_equal(out, want[0]) and np.array_equal(st, want[1])
    assert not st["status"].any() and np.abs(out.astype(np.int32)).max() > 1000


# 6 ---- truth: a glide ends on the formants of its end tables

def test_glides_end_on_the_formants_of_their_end_tables(engine):
    """the worst error with the restatement (tests/test_track_ref.py) is 136 Hz against SPEECH_TOL_HZ = 474 Hz"""
    lane = vs.lane_from_cli(["-r", "16000", "-d", "1", "-f", "110"], ["-v", "a"], 3)[0]
    flow = engine.source([lane], 16000)
    coefs = np.array([truth_anchors(a, b) for a, b in TRUTH_PAIRS])
    pcm, stat = engine.filter_track(np.repeat(flow, len(TRUTH_PAIRS), axis=0), coefs, hop=1600, gain=1.0,
                                    pre_emphasis=1.0, mode="glide")
    assert not stat["status"].any() and not stat["n_unusable"].any()
    assert np.abs(pcm.astype(np.int32)).max() < 32767
    res = engine.lpc(pcm, 16000, order=22, window_s=0.040, hop_s=0.010, n_formants=20)

    errs = []
    for r, (a, b) in enumerate(TRUTH_PAIRS):
        def frame(x, start, r=r):
            j = start // 160
            assert res["start"][r, j] == start and res["status"][r, j] == 0
            return res["formants"][r, j, :res["n_formants"][r, j], 0]
        errs += plateau_errors(pcm[r], a, b, frame)
    print("worst plateau formant error on the device %.1f Hz" % max(errs))
    assert len(errs) >= 12 and max(errs) <= SPEECH_TOL_HZ, max(errs)


# 7 ---- the FMA form

def test_fma_arithmetic_within_one_lsb_on_table_glides(engine):
    flow = _test_flows(engine)
    n, ns = flow.shape
    rng = np.random.default_rng(SEED + 7)
    tabs = np.array([vs.vowel_coefficients(v) for v in TABLES])
    worst = 0
    for K in (2, 11):
        coefs = tabs[rng.integers(0, 10, (n, K))]
        rows = _drawn_rows(rng, n, K, ns)
        exact = _device(engine, flow, coefs, rows, "glide")
        engine.set_arith(vs.VS_ARITH_FMA)
        try:
            fma = _device(engine, flow, coefs, rows, "glide")
        finally:
            engine.set_arith(vs.VS_ARITH_EXACT)
        assert np.array_equal(fma[1], exact[1])
        d = int(np.abs(fma[0].astype(np.int32) - exact[0].astype(np.int32)).max())
        print("K = %d: FMA differs from exact in %d samples, at most %d LSB" % (K, int((fma[0] != exact[0]).sum()), d))
        worst = max(worst, d)
    assert worst <= 1


# 8 ---- bin/vtrack

def _read(path):
    raw = open(path, "rb").read()
    return raw[:44], np.frombuffer(raw[44:], dtype=np.int16)


def test_vtrack_program(engine, tmp_path):
    env = dict(os.environ, VS_SEED="9", VS_WAV_HEADER="44")
    subprocess.run([os.path.join(BIN, "flowgen_shimmer"), "-o", "g.wav", "-r", "16000", "-d", "1", "-f", "110", "-j", "1"],
                   cwd=tmp_path, env=env, check=True, capture_output=True)
    subprocess.run([os.path.join(BIN, "vowel"), "-i", "g.wav", "-o", "model.wav", "-v", "i", "-p", "1"], cwd=tmp_path,
                   env=env, check=True, capture_output=True)
    head, flow = _read(tmp_path / "g.wav")
    _, model = _read(tmp_path / "model.wav")
    N = len(flow)
    r = subprocess.run([os.path.join(BIN, "vtrack"), "-i", "g.wav", "-o", "ai.wav", "-v", "a,i", "-g", "2", "-p", "1"],
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "ai.wav 2 0 0\n"
    coefs = np.array([vs.vowel_coefficients("a"), vs.vowel_coefficients("i")])[None]
    want, _ = engine.filter_track(flow[None], coefs, hop=N - 1, gain=2.0, pre_emphasis=1.0, mode="glide")
    got_head, got = _read(tmp_path / "ai.wav")
    assert got_head == head and np.array_equal(got, want[0])
    r = subprocess.run([os.path.join(BIN, "vtrack"), "-i", "g.wav", "-o", "aiu.wav", "-v", "a,i,u"], cwd=tmp_path, env=env,
                       capture_output=True, text=True)
    coefs = np.array([vs.vowel_coefficients(v) for v in "aiu"])[None]
    want, _ = engine.filter_track(flow[None], coefs, hop=(N - 1) // 2, mode="glide")
    assert r.returncode == 0 and np.array_equal(_read(tmp_path / "aiu.wav")[1], want[0])
    # -m: the frames of a recording
    for extra, mode in (([], "hold"), (["-G"], "glide")):
        opts = dict(order=18, hop_s=0.005, n_formants=0)
        r = subprocess.run([os.path.join(BIN, "vtrack"), "-i", "g.wav", "-o", "copy.wav", "-m", "model.wav", "-O", "18", "-t",
                            "5", "-p", "0.9"] + extra, cwd=tmp_path, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lp = engine.lpc(model[None], 16000, coefs=True, **opts)
        row = vs.track_from_lpc(16000, len(model), mode, **opts)
        want, st = engine.filter_track(flow[None], lp["coefs"], row["hop"], row["offset"], pre_emphasis=0.9, mode=mode)
        assert r.stdout == "copy.wav %d %d %d\n" % (row["n_sets"], st["n_unusable"][0], st["status"][0])
        assert np.array_equal(_read(tmp_path / "copy.wav")[1], want[0])
        assert np.abs(want.astype(np.int32)).max() > 1000
    # a model that is not PCM: named, exit status 2
    raw = bytearray(open(tmp_path / "model.wav", "rb").read())
    raw[20:22] = struct.pack("<H", 3)
    open(tmp_path / "tag3.wav", "wb").write(bytes(raw))
    r = subprocess.run([os.path.join(BIN, "vtrack"), "-i", "g.wav", "-o", "x.wav", "-m", "tag3.wav"], cwd=tmp_path, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "tag3.wav" in r.stderr and not os.path.exists(tmp_path / "x.wav")
    r = subprocess.run([os.path.join(BIN, "vtrack"), "-i", "g.wav", "-o", "x.wav", "-v", "a"], cwd=tmp_path, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 1


# 9 ---- one full-size launch

# the rows compared with the restatement (it is too slow for all 65536): 64 spread over the batch
FULL_ROWS = np.linspace(0, 65535, 64).astype(int)


def test_full_size_launch_on_config3(engine):
    lanes, ns = _lanes(3)
    flow = engine.source(lanes, ns)
    n = len(lanes)
    assert flow.shape == (65536, 16000)
    rng = np.random.default_rng(SEED + 9)
    pool = _blend_sets(rng, 4096, 1, 22)[:, 0]
    for mode, m, K, hop in (("hold", tr.HOLD, 100, 160), ("glide", tr.GLIDE, 11, 1600)):
        coefs = pool[rng.integers(0, len(pool), (n, K))]
        got, stat = engine.filter_track(flow, coefs, hop=hop, offset=40, gain=2.0, pre_emphasis=1.0, mode=mode)
        assert not stat["status"].any() and not stat["n_unusable"].any()
        rows = vs.track_rows(len(FULL_ROWS), K, hop, 40, ns, 2.0, 1.0)
        peak = []
        want, _ = tr.filter_track(flow[FULL_ROWS], coefs[FULL_ROWS], rows, m, state_max=peak)
        assert peak[0] < STATE_MAX
        assert np.array_equal(got[FULL_ROWS], want)
        del coefs, got
