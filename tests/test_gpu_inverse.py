"""The inverse filter on the device (vs_inverse / vs_inverse_launch, bin/vinverse) against its numpy restatement
(tests/inverse_ref.py), byte for byte, output and stat, in both arithmetics: drawn rows over orders, modes, hops, offsets,
lengths, de-emphases and scales; the hostile cases tests/test_inverse_ref.py builds (saturation past int32 with an exact
n_clipped, the integrator on a full-scale constant, unusable sets, taps that tell the arithmetics apart); pitches and
base alignments through the launch; the round trip behind vs_track within the header's derived bound; the chain
lpc -> inverse -> track -> measure on one stream; range errors; the program; launches back to back.

Shapes are small (70 rows x 2003 samples unless said otherwise): the restatement's loop over samples sets the cost.
Every test prints what it measured (pytest -s): profiles/inverse_hostile_signals.txt keeps those lines."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inverse_ref as ir  # noqa: E402
import test_inverse_ref as cases  # noqa: E402
from test_inverse_ref import SENTINEL  # noqa: E402
from gpu_support import INPUT_PAD, GuardedRows  # noqa: E402

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(vs.__file__), "bin")
R, N = 70, 2003                                 # a whole wavefront and a partial one; 83 groups of 24, one of 8, 3 samples
ORDERS = [1, 12, 22, 23, 40]
MODES = [ir.HOLD, ir.GLIDE]
MODE_NAME = {ir.HOLD: "hold", ir.GLIDE: "glide"}
ARITHS = {"exact": vs.VS_ARITH_EXACT, "fma": vs.VS_ARITH_FMA}
SEED = 20241018


class _arith:
    def __init__(self, engine, arith):
        self.engine, self.arith = engine, arith

    def __enter__(self):
        self.engine.set_arith(ARITHS[self.arith])

    def __exit__(self, *exc):
        self.engine.set_arith(vs.VS_ARITH_EXACT)


def _device(engine, pcm, coefs, rows, mode, out=None):
    return engine.inverse_filter(pcm, coefs, rows["hop"], rows["offset"], rows["n_sets"], rows["length"], rows["scale"],
                                 rows["de_emphasis"], MODE_NAME[mode], out)


def _ints(a):
    return [int(v) for v in a]


def _assert_same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:8], got[1][:4], want[1][:4])
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:8])


def _run_case(engine, c, arith):
    with _arith(engine, arith):
        got = _device(engine, c.pcm, c.coefs, c.rows, c.mode, c.out)
    _assert_same(got, c.want)
    return got


# 1 ---- drawn rows against the restatement

def _drawn_pcm(rng, n, ns):
    """noise at full scale, a tenth and a hundredth of it, row by row"""
    amp = np.array([1.0, 0.1, 0.01])[np.arange(n) % 3]
    return (rng.integers(-32768, 32768, (n, ns)) * amp[:, None]).astype(np.int16)


def _drawn_rows(rng, n, K, ns):
    """tests/test_gpu_track.py's _drawn_rows with the inverse's fields, and the short lengths"""
    rows = np.zeros(n, dtype=ir.ROW_DTYPE)
    rows["n_sets"] = rng.integers(1, K + 1, n)
    rows["hop"] = rng.integers(1, max(2, 2 * ns // K), n)
    rows["offset"] = rng.integers(-3000, 3000, n)
    rows["length"] = np.where(rng.uniform(size=n) < 0.3, rng.integers(0, ns + 1, n), ns)
    rows["scale"] = rng.uniform(0.1, 8.0, n).astype(np.float32)
    rows["de_emphasis"] = rng.choice([0.0, 1.0, 0.37, 0.9], n).astype(np.float32)
    # the corners: hop 1, hop > n_samples, offsets far outside the row on both sides, offset -2^31 with hop 2^31 - 1
    rows["hop"][0], rows["hop"][1] = 1, ns + 4000
    rows["offset"][2], rows["offset"][3], rows["offset"][4] = -5000, ns + 1000, -2147483648
    rows["hop"][4], rows["n_sets"][4] = 2147483647, K
    rows["n_sets"][:4] = K
    rows["length"][:5] = ns
    short = [0, 1, 7, 8, 9, 23, 24, 25, 47, 48, 49]
    rows["length"][5:5 + len(short)] = short
    rows["length"][[62, 63, 64, n - 1]] = ns                 # the ends of the whole wavefront and of the partial one
    return rows


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ORDERS)
def test_drawn_rows_equal_the_restatement(engine, order, mode, arith):
    K = 7
    rng = np.random.default_rng(SEED + 10 * order + mode)
    pcm = _drawn_pcm(rng, R, N)
    coefs = cases.table_like_sets(rng, R, K, order)
    rows = _drawn_rows(rng, R, K, N)
    c = cases.restated(pcm, coefs, rows, mode, arith=arith, out=np.full((R, N), SENTINEL, dtype=np.int16))
    got = _run_case(engine, c, arith)
    st = got[1]
    assert not st["status"].any() and not st["n_unusable"].any() and not st["reserved_"].any()
    assert {0.0, 0.37, 0.9, 1.0} == set(np.round(rows["de_emphasis"].astype(float), 2))
    for r in range(R):
        assert (got[0][r, rows["length"][r]:] == SENTINEL).all()
    clipped = st["n_clipped"].sum() / max(1, rows["length"].sum())
    print("order %2d %-5s %-5s: %d rows x %d samples equal the restatement; %.1f %% of the samples clipped; e*c in "
          "[%.3e, %.3e]" % (order, MODE_NAME[mode], arith, R, N, 100 * clipped, c.lo.min(), c.hi.max()))
    assert 0.01 < clipped < 0.9


# 2 ---- the hostile cases of the CPU file

@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("order", cases.HOSTILE_ORDERS)
def test_saturation_past_int32_with_an_exact_count(engine, order, arith):
    line = cases.check_saturation_conditions(order)
    got = _run_case(engine, cases.saturation_case(order, arith), arith)
    assert got[1]["n_clipped"].max() == cases.HOSTILE_N
    print(arith, line)


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [22, 40])
def test_integrator_on_constant_full_scale_rows(engine, order, mode, arith):
    c = cases.integrator_case(order, mode, arith)
    assert np.isfinite(c.lo).all() and np.isfinite(c.hi).all()
    got = _run_case(engine, c, arith)
    print("order %d %s %s: rho = 1 on constant -32768: e*c in [%.3e, %.3e], n_clipped %s" % (
        order, MODE_NAME[mode], arith, c.lo.min(), c.hi.max(), _ints(got[1]["n_clipped"])))


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", cases.HOSTILE_ORDERS)
def test_unusable_sets_forward_fill_and_rows_without_a_set(engine, order, mode, arith):
    c = cases.unusable_case(order, mode, arith)
    got = _run_case(engine, c, arith)
    st = got[1]
    assert st["status"][3] == vs.VS_INVERSE_NO_SET and st["status"][5] == vs.VS_INVERSE_NO_SET
    assert st["status"].sum() == (3 if mode == ir.GLIDE else 2)
    print("order %2d %-5s %-5s: n_unusable %s, status %s" % (order, MODE_NAME[mode], arith, _ints(st["n_unusable"]),
                                                             _ints(st["status"])))


@pytest.mark.parametrize("order", cases.CANCEL_ORDERS)
def test_each_arithmetic_runs_its_own_form(engine, order):
    e, f = cases.cancelling_case(order, "exact"), cases.cancelling_case(order, "fma")
    assert (e.want[0] != f.want[0]).mean() > 0.25
    _run_case(engine, e, "exact")
    _run_case(engine, f, "fma")
    engine.set_arith(vs.VS_ARITH_F32)                      # no single-precision form: the FMA form, as on the track path
    try:
        _assert_same(_device(engine, f.pcm, f.coefs, f.rows, f.mode), f.want)
    finally:
        engine.set_arith(vs.VS_ARITH_EXACT)
    print("order %d: the device follows each restatement where they differ in %.1f %% of the samples" % (
        order, 100 * (e.want[0] != f.want[0]).mean()))


# 3 ---- layouts through vs_inverse_launch

LAYOUTS = [(N, N), (N + 1, N), (N, N + 1), (N + 6, N + 3)]
BASES = [(0, 0), (2, 0), (0, 2), (2, 2)]        # bytes added to the (256-byte aligned) allocations of input and output


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [22, 40])
def test_pitches_and_alignments_through_the_launch(engine, order, mode):
    K = 4
    rng = np.random.default_rng(SEED + 400 + order)
    pcm = _drawn_pcm(rng, R, N)
    coefs = cases.table_like_sets(rng, R, K, order)
    rows = ir.rows_of(R, K, 300, rng.integers(-30, 30, R), rng.integers(0, N + 1, R), rng.uniform(0.1, 8.0, R),
                      rng.choice([0.0, 0.37, 0.9, 1.0], R))
    rows["length"][:6] = [N, 0, N - 1, 1, 8, N - 8]
    c = cases.restated(pcm, coefs, rows, mode, out=np.full((R, N), SENTINEL, dtype=np.int16))
    with engine.scope() as dev:
        cf_d, st_d = dev.put(coefs), dev.room(R * 16)
        out = GuardedRows(R, N, N + 6, 2, sentinel=SENTINEL).on(dev)
        in_d = dev.room(out.room * 2)
        for in_pitch, out_pitch in LAYOUTS:
            for in_off, out_off in BASES:
                what = (in_pitch, out_pitch, in_off, out_off)
                staged = np.full((R, in_pitch), INPUT_PAD, dtype=np.int16)      # the padding of the input is not silence
                staged[:, :N] = pcm
                engine.dev_upload(in_d + in_off, staged)
                out.fill()
                engine.dev_upload(st_d, np.full(R, -1, dtype=vs.INVERSE_STAT_DTYPE))
                engine.inverse_filter_dev(MODE_NAME[mode], order, in_d + in_off, in_pitch, out.first(out_pitch, out_off),
                                          out_pitch, R, N, rows, cf_d, K, stat_ptr=st_d)
                engine.synchronize()
                body = out.rows_back(out_pitch, out_off, what)          # guards and pitch padding untouched
                _assert_same((body, dev.get(st_d, (R,), vs.INVERSE_STAT_DTYPE)), c.want, what)
    print("order %d %s: %d layouts x %d base alignments equal the restatement, padding and guards untouched" % (
        order, MODE_NAME[mode], len(LAYOUTS), len(BASES)))


# 4 ---- the round trip on the device

def test_round_trip_behind_the_track_filter_stays_within_the_derived_bound(engine):
    flow = cases.round_trip_flows()
    coefs = cases.table_sets()
    mu, g, scale = cases._pair_arrays(40)
    pcm, tstat = engine.filter_track(flow, coefs, hop=1, gain=g, pre_emphasis=mu)
    assert np.abs(pcm.astype(np.int32)).max() < 32767 and not tstat["status"].any()
    got = engine.inverse_filter(pcm, coefs, hop=1, scale=scale, de_emphasis=mu)
    want = ir.inverse_filter(pcm, coefs, ir.rows_of(40, 1, 1, 0, cases.ROUND_N, scale, mu), ir.HOLD)
    _assert_same(got, want)
    err = np.abs(got[0].astype(np.int32) - flow.astype(np.int32)).max(axis=1)
    bound = cases.hold_bounds()
    for q in range(4):
        print("hold, mu %.2f g %.2f: largest |inverse - flow| %s LSB, derived bounds %s" % (
            cases.PAIRS[q][0], cases.PAIRS[q][1], _ints(err[q::4]), _ints(bound[q::4])))
    assert (err <= bound).all() and not got[1]["n_clipped"].any()
    # a -> i: 101 anchors at hop 160
    flow = flow[:4]
    A, B = vs.vowel_coefficients("a"), vs.vowel_coefficients("i")
    coefs = np.broadcast_to(vs.track_glide_sets(A, B, 101), (4, 101, 23))
    pcm, tstat = engine.filter_track(flow, coefs, hop=160, gain=g[:4], pre_emphasis=mu[:4], mode="glide")
    assert np.abs(pcm.astype(np.int32)).max() < 32767 and not tstat["n_unusable"].any()
    got = engine.inverse_filter(pcm, coefs, hop=160, scale=scale[:4], de_emphasis=mu[:4], mode="glide")
    want = ir.inverse_filter(pcm, coefs, ir.rows_of(4, 101, 160, 0, cases.ROUND_N, scale[:4], mu[:4]), ir.GLIDE)
    _assert_same(got, want)
    err = np.abs(got[0].astype(np.int32) - flow.astype(np.int32)).max(axis=1)
    bound = np.array([2 * max(ir.round_trip_bound(A, mu[r], scale[r], cases.ROUND_N),
                              ir.round_trip_bound(B, mu[r], scale[r], cases.ROUND_N)) for r in range(4)])
    print("glide a -> i: largest |inverse - flow| %s LSB, twice the larger end bound %s" % (_ints(err), _ints(bound)))
    assert (err <= bound).all()


# 5 ---- the chain on one stream

def test_chain_lpc_inverse_track_measure_on_one_stream(engine):
    specs, fs, dur, _ = configs.config_specs(3, 16)
    lanes, _ = vs.lanes_from_specs(specs)
    n, ns = len(lanes), 4000
    pcm = engine.synth(lanes, ns)
    opts = dict(n_formants=0)
    nfr = vs.lpc_frames(fs, ns, **opts)
    irow = vs.inverse_from_lpc(fs, ns, "hold", **opts)
    trow = vs.track_from_lpc(fs, ns, "hold", **opts)
    assert tuple(irow)[:4] == tuple(trow)[:4] and irow["n_sets"] == nfr
    irow["scale"], trow["gain"] = 0.25, 4.0      # a residual that stays inside int16; the track's gain undoes the scale
    with engine.scope() as dev:
        pcm_d = dev.put(pcm)
        res_d, syn_d = (dev.put(np.zeros((n, ns), dtype=np.int16)) for _ in range(2))
        fr_d, cf_d = dev.room(n * nfr * 32), dev.room(n * nfr * 23 * 8)
        ist_d, tst_d, ac_d = dev.room(n * 16), dev.room(n * 8), dev.room(n * 96)
        # four launches, no wait in between
        engine.lpc_dev(pcm_d, ns, n, ns, fs, nfr, fr_d, None, cf_d, **opts)
        engine.inverse_filter_dev("hold", 22, pcm_d, ns, res_d, ns, n, ns, irow, cf_d, nfr, stat_ptr=ist_d)
        engine.filter_track_dev("hold", 22, res_d, ns, syn_d, ns, n, ns, trow, cf_d, nfr, stat_ptr=tst_d)
        engine.measure_dev(res_d, ns, n, ns, fs, ac_d, polarity=-1)
        res = dev.get(res_d, (n, ns))
        syn = dev.get(syn_d, (n, ns))
        coefs = dev.get(cf_d, (n, nfr, 23), np.float64)
        ist = dev.get(ist_d, (n,), vs.INVERSE_STAT_DTYPE)
        tst = dev.get(tst_d, (n,), vs.TRACK_STAT_DTYPE)
        ac = dev.get(ac_d, (n,), vs.ACOUSTIC_DTYPE)
    host_coefs = engine.lpc(pcm, fs, coefs=True, **opts)["coefs"]
    assert np.array_equal(coefs, host_coefs, equal_nan=True)
    want_res = engine.inverse_filter(pcm, host_coefs, irow["hop"], irow["offset"], scale=0.25)
    assert np.array_equal(res, want_res[0]) and np.array_equal(ist, want_res[1])
    want_syn = engine.filter_track(res, host_coefs, trow["hop"], trow["offset"], gain=4.0)
    assert np.array_equal(syn, want_syn[0]) and np.array_equal(tst, want_syn[1])
    want_ac = engine.measure(res, fs, polarity=-1)
    assert ac.tobytes() == want_ac.tobytes()
    assert not ist["status"].any() and np.abs(res.astype(np.int32)).max() > 100
    d = np.abs(syn.astype(np.int32) - pcm.astype(np.int32))
    print("chain on one stream: %d rows x %d samples, %d frames; residual peak %d, n_clipped %d; resynthesis from the "
          "residual against the input: at most %d LSB (mean %.2f)" % (n, ns, nfr, np.abs(res.astype(np.int32)).max(),
                                                                     int(ist["n_clipped"].sum()), d.max(), d.mean()))


# 6 ---- range errors

def test_range_errors(engine):
    pcm = np.zeros((2, 100), dtype=np.int16)
    coefs = np.zeros((2, 3, 23))
    ok = dict(hop=10, scale=1.0, de_emphasis=0.5)
    engine.inverse_filter(pcm, coefs, **ok)
    for bad in (dict(de_emphasis=-0.01), dict(de_emphasis=1.01), dict(de_emphasis=np.nan), dict(scale=np.nan),
                dict(scale=np.inf), dict(hop=0), dict(n_sets=4), dict(n_sets=0), dict(lengths=101), dict(lengths=-1)):
        with pytest.raises(vs.VsError) as e:
            engine.inverse_filter(pcm, coefs, **dict(ok, **bad))
        assert e.value.code == vs._ffi.VS_ERR_RANGE, bad
    with pytest.raises(vs.VsError) as e:
        engine.inverse_filter(pcm, np.zeros((2, 3, 42)), **ok)
    assert e.value.code == vs._ffi.VS_ERR_RANGE
    with pytest.raises(vs.VsError) as e:
        engine.inverse_filter(pcm, coefs, mode=2, **ok)
    assert e.value.code == vs._ffi.VS_ERR_ARG
    engine.inverse_filter(pcm, coefs, **dict(ok, de_emphasis=[0.0, 1.0]))      # the ends of the range are inside


# 7 ---- bin/vinverse

def _read(path):
    raw = open(path, "rb").read()
    return raw[:44], np.frombuffer(raw[44:], dtype=np.int16)


def _run(tmp_path, env, prog, *args):
    return subprocess.run([os.path.join(BIN, prog)] + list(args), cwd=tmp_path, env=env, capture_output=True, text=True)


def test_vinverse_program(engine, tmp_path):
    env = dict(os.environ, VS_SEED="9", VS_WAV_HEADER="44")
    r = _run(tmp_path, env, "flowgen_shimmer", "-o", "g.wav", "-r", "16000", "-d", "0.5", "-f", "110", "-j", "1", "-s", "5")
    assert r.returncode == 0, r.stderr
    head, flow = _read(tmp_path / "g.wav")
    ns = len(flow)
    # vtrack -v a,i -p 0.9 then vinverse -v a,i -d 0.9 -s 1/g: the flow file again, within the derived bound
    r = _run(tmp_path, env, "vtrack", "-i", "g.wav", "-o", "ai.wav", "-v", "a,i", "-g", "0.1", "-p", "0.9")
    assert r.returncode == 0, r.stderr
    speech = _read(tmp_path / "ai.wav")[1]
    assert np.abs(speech.astype(np.int32)).max() < 32767
    r = _run(tmp_path, env, "vinverse", "-i", "ai.wav", "-o", "back.wav", "-v", "a,i", "-d", "0.9", "-s", "10")
    assert r.returncode == 0, r.stderr
    assert r.stdout == "back.wav 2 0 0 0\n"
    got_head, back = _read(tmp_path / "back.wav")
    A, B = vs.vowel_coefficients("a"), vs.vowel_coefficients("i")
    bound = 2 * max(ir.round_trip_bound(A, np.float32(0.9), 10.0, ns), ir.round_trip_bound(B, np.float32(0.9), 10.0, ns))
    err = int(np.abs(back.astype(np.int32) - flow.astype(np.int32)).max())
    print("vtrack -v a,i -g 0.1 -p 0.9 | vinverse -v a,i -d 0.9 -s 10: |back - flow| <= %d LSB (bound %.0f)" % (err, bound))
    assert got_head == head and err <= bound
    want, st = engine.inverse_filter(speech[None], np.array([A, B])[None], hop=ns - 1, scale=10.0, de_emphasis=0.9,
                                     mode="glide")
    assert np.array_equal(back, want[0])
    # one id: that table held, its taps untouched
    r = _run(tmp_path, env, "vinverse", "-i", "ai.wav", "-o", "a.wav", "-v", "a", "-d", "1", "-s", "0.5")
    want, st = engine.inverse_filter(speech[None], A[None, None], hop=1, scale=0.5, de_emphasis=1.0)
    assert r.returncode == 0 and r.stdout == "a.wav 1 0 %d 0\n" % st["n_clipped"][0]
    assert np.array_equal(_read(tmp_path / "a.wav")[1], want[0])
    # -m with the input as its own model: the LPC residual, as the Python chain gives it
    for extra, mode, pre in (([], "hold", 0), (["-G", "-P"], "glide", 1)):
        opts = dict(order=18, hop_s=0.005, n_formants=0, pre_emphasis=pre)
        r = _run(tmp_path, env, "vinverse", "-i", "ai.wav", "-o", "res.wav", "-m", "ai.wav", "-O", "18", "-t", "5", "-d",
                 "0.5", *extra)
        assert r.returncode == 0, r.stderr
        lp = engine.lpc(speech[None], 16000, coefs=True, **opts)
        row = vs.inverse_from_lpc(16000, ns, mode, **opts)
        want, st = engine.inverse_filter(speech[None], lp["coefs"], row["hop"], row["offset"], de_emphasis=0.5, mode=mode)
        assert r.stdout == "res.wav %d %d %d %d\n" % (row["n_sets"], st["n_unusable"][0], st["n_clipped"][0],
                                                      st["status"][0])
        assert np.array_equal(_read(tmp_path / "res.wav")[1], want[0])
        assert np.abs(want.astype(np.int32)).max() > 50
    # a file that is not PCM: named, exit status 2; usage: 1
    raw = bytearray(open(tmp_path / "ai.wav", "rb").read())
    raw[20:22] = struct.pack("<H", 3)
    open(tmp_path / "tag3.wav", "wb").write(bytes(raw))
    for args in (("-i", "tag3.wav", "-o", "x.wav", "-v", "a"), ("-i", "ai.wav", "-o", "x.wav", "-m", "tag3.wav"),
                 ("-i", "missing.wav", "-o", "x.wav", "-v", "a")):
        r = _run(tmp_path, env, "vinverse", *args)
        assert r.returncode == 2 and ("tag3.wav" in r.stderr or "missing.wav" in r.stderr)
        assert not os.path.exists(tmp_path / "x.wav")
    for args in (("-i", "ai.wav", "-o", "x.wav"), ("-i", "ai.wav", "-o", "x.wav", "-v", "a", "-m", "ai.wav"),
                 ("-i", "ai.wav", "-o", "x.wav", "-v", "a", "-d", "1.5"), ("-i", "ai.wav", "-o", "x.wav", "-v", "a,")):
        assert _run(tmp_path, env, "vinverse", *args).returncode == 1


# 8 ---- launches back to back

def test_two_launches_back_to_back_with_different_rows(engine):
    K, order = 5, 22
    rng = np.random.default_rng(SEED + 8)
    pcm = _drawn_pcm(rng, R, N)
    coefs = cases.table_like_sets(rng, R, K, order)
    rows = [_drawn_rows(np.random.default_rng(SEED + 80 + i), R, K, N) for i in range(2)]
    want = [ir.inverse_filter(pcm, coefs, rows[i], ir.HOLD) for i in range(2)]
    assert not np.array_equal(want[0][0], want[1][0])
    with engine.scope() as dev:
        in_d, cf_d = dev.put(pcm), dev.put(coefs)
        out_d = [dev.put(np.zeros((R, N), dtype=np.int16)) for _ in range(2)]
        st_d = [dev.room(R * 16) for _ in range(2)]
        for i in range(2):                       # no wait between the two
            engine.inverse_filter_dev("hold", order, in_d, N, out_d[i], N, R, N, rows[i], cf_d, K, stat_ptr=st_d[i])
        for i in range(2):
            _assert_same((dev.get(out_d[i], (R, N)), dev.get(st_d[i], (R,), vs.INVERSE_STAT_DTYPE)), want[i], i)
    print("two launches back to back: each equals its own restatement (%d and %d samples clipped)" % (
        want[0][1]["n_clipped"].sum(), want[1][1]["n_clipped"].sum()))
