"""The per-cycle log (vs_cycle_rec) and the cycle counts of every kernel that writes them, byte for byte against the
oracle (records viewed as uint32: -0.0 is not 0.0, a NaN equals only itself), every lane against its own
po.source_one(lane, n, pitch) -- which also holds the plan's row reordering -- next to the flow or PCM of the same launch:

  a. vs_source (the host path): zero-copy on a fresh context for 64 lanes and fewer, pooled otherwise; it clears the log;
  b. vs_plan_launch with a log and counts into canary-filled buffers: kinds SOURCE and SYNTH, the three contexts, pitches
     below, at and above the cycle counts; a launch writes records [0, min(ncyc, pitch)) of a row and nothing else;
  c. the pre-emphasis-1 instantiation with a log;   d. vowel -n's noise passes behind a launch with a log;
  e. the narrow build;   f. the wide plan (the source step writes flow, log and counts);
  g. the counts of the kernels that keep no log: the wave-specialised ones (two roles, three, the -n power kernel);
  h. bin/flowgen_shimmer, which prints the log line by line, against recorded runs of the compiled reference.

The batches, and what makes them worth launching, are built and asserted on the CPU in tests/test_cycle_log_ref.py.
Every test prints what it compared (pytest -s): profiles/cycle_log_sets.txt keeps those lines."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cycle_log_ref as ref  # noqa: E402
from test_cycle_log_ref import LOG_PITCH, PITCHES, PREFIXES, as_bytes, batch  # noqa: E402
from gpu_support import SENTINEL  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY16 = SENTINEL
CANARY32 = 0x5A5A5A5A
ARITHS = (vs.VS_ARITH_EXACT, vs.VS_ARITH_FMA, vs.VS_ARITH_F32)
ARITH_NAME = {vs.VS_ARITH_EXACT: "EXACT", vs.VS_ARITH_FMA: "FMA", vs.VS_ARITH_F32: "F32"}
KIND_NAME = {vs.VS_KIND_SOURCE: "SOURCE", vs.VS_KIND_SYNTH: "SYNTH"}
BIN = os.path.join(os.path.dirname(vs.__file__), "bin")


@functools.lru_cache(maxsize=None)
def _pcm(name):
    b = batch(name)
    pcm = po.synth(b.lanes, b.n)
    pcm.setflags(write=False)
    return pcm


def _expected_log(want_recs, want_ncyc, pitch, rows, fill):
    """[rows][pitch][4] uint32: records [0, min(ncyc, pitch)) of every lane, `fill` everywhere else (rows may be one more
    than the lanes: the row behind the batch)"""
    exp = np.full((rows, pitch, 4), fill, dtype="<u4")
    nl = len(want_ncyc)
    live = np.arange(pitch)[None, :] < np.minimum(want_ncyc, pitch)[:, None]
    exp[:nl][live] = as_bytes(want_recs)[live]
    return exp, int(live.sum())


def _same_log(got, exp, what):
    """got, exp: [rows][pitch][4] uint32.  Says how many lanes differ, and where the first ones do."""
    bad = (got != exp).any(axis=2)
    assert not bad.any(), ("%d rows differ" % bad.any(axis=1).sum(), what, np.argwhere(bad)[:6],
                           got[bad][:3], exp[bad][:3])


def _want(lanes, n, pitch):
    """(records [lanes][pitch], ncyc) of lanes that belong to no batch"""
    recs, ncyc, _ = ref.oracle_log(lanes, n, pitch)
    return recs, ncyc


def _canary_launch(eng, plan, nl, n, kind, pitch=0, counts=True):
    """one launch into canary-filled buffers of one row more than the batch: (out [nl + 1][n] int16, log
    [nl + 1][pitch][4] uint32 or None, ncyc [nl + 1] int32 or None)"""
    with eng.scope() as dev:
        out_d = dev.filled((nl + 1) * n, CANARY16, np.int16)
        log_d = dev.filled((nl + 1) * pitch * 4, CANARY32, "<u4") if pitch else None
        cnt_d = dev.filled(nl + 1, CANARY32, np.int32) if counts else None
        plan.launch(kind, out_d, log_ptr=log_d, log_pitch=pitch, ncyc_ptr=cnt_d)
        eng.synchronize()
        assert plan.status() == 0
        out = dev.get(out_d, (nl + 1, n))
        log = dev.get(log_d, (nl + 1, pitch, 4), np.dtype("<u4")) if pitch else None
        cnt = dev.get(cnt_d, (nl + 1,), np.int32) if counts else None
    assert (out[nl] == CANARY16).all()
    return out, log, cnt


def _held(out, log, cnt, want_out, want_recs, want_ncyc, pitch, what):
    """a launch against the oracle: the rows, the log (canaries wherever a launch must not write) and the counts; returns
    the records compared"""
    nl = len(want_ncyc)
    assert np.array_equal(cnt[:nl], want_ncyc), (what, np.flatnonzero(cnt[:nl] != want_ncyc)[:8])
    assert cnt[nl] == CANARY32, what
    exp, nrec = _expected_log(want_recs, want_ncyc, pitch, nl + 1, CANARY32)
    _same_log(log, exp, what)
    if want_out is not None:
        bad = (out[:nl] != want_out).any(axis=1)
        assert not bad.any(), ("%d rows of samples differ" % bad.sum(), what, np.flatnonzero(bad)[:8])
    return nrec


# a ---- the host path

def _vs_source(eng, lanes, n, pitch):
    """vs_source into canary-filled host arrays of one row more than the batch"""
    arr = vs._as_lane_array(lanes)
    nl = len(arr)
    flow = np.full((nl + 1, n), CANARY16, dtype=np.int16)
    recs = np.full((nl + 1, pitch, 4), CANARY32, dtype="<u4")
    cnt = np.full(nl + 1, CANARY32, dtype=np.int32)
    vs.check(eng._lib.vs_source(eng._ctx, arr, nl, n, flow.ctypes.data, recs.ctypes.data, pitch, cnt.ctypes.data), "vs_source")
    return flow, recs, cnt


@pytest.mark.parametrize("name", sorted(ref.BATCHES))
def test_vs_source_log_and_counts(name):
    """a fresh context: the prefixes of 64 lanes and fewer run without a copy (the log lives in pinned host memory the
    kernel writes over PCIe, cleared by the CPU), then the larger ones through the pool (cleared on the stream), then the
    small ones again on the context that has copied by now.  Records [0, min(ncyc, pitch)) are the oracle's, the rest of
    the row is zero, the count is the full one; the row behind the batch is the caller's"""
    b = batch(name)
    with vs.Engine(0) as eng:
        total = 0
        order = [(k, "zero-copy") for k in PREFIXES if k <= 64] + [(k, "pooled") for k in PREFIXES if k > 64] + [
            (len(b.lanes), "pooled"), (64, "pooled"), (1, "pooled")]
        for k, path in order:
            for pitch in PITCHES:
                want_recs, want_ncyc = b.want(pitch)
                flow, recs, cnt = _vs_source(eng, b.lanes[:k], b.n, pitch)
                what = (name, k, pitch, path)
                assert np.array_equal(flow[:k], b.flow[:k]) and (flow[k] == CANARY16).all(), what
                assert np.array_equal(cnt[:k], want_ncyc[:k]) and cnt[k] == CANARY32, what
                exp, nrec = _expected_log(want_recs[:k], want_ncyc[:k], pitch, k + 1, 0)
                exp[k] = CANARY32
                _same_log(recs, exp, what)
                total += nrec
            if path == "zero-copy" and k == 64:
                # Engine.source, the call the other tests make, gives the same
                f2, r2, c2 = eng.source(b.lanes[:k], b.n, log_cycles=LOG_PITCH)
                assert np.array_equal(f2, b.flow[:k]) and np.array_equal(c2, b.ncyc[:k])
                assert np.array_equal(as_bytes(r2), as_bytes(b.recs[:k]))
        print("vs_source, %s: %d calls (lanes %s; pitches %s; without a copy, pooled, pooled again), %d records and %d "
              "counts equal the oracle, zeros behind them" % (name, len(order) * len(PITCHES), [k for k, _ in order],
                                                             list(PITCHES), total, sum(k for k, _ in order) * len(PITCHES)))
        print("  " + ref.describe(b))


# b ---- vs_plan_launch with a log and counts

@pytest.mark.parametrize("kind", [vs.VS_KIND_SOURCE, vs.VS_KIND_SYNTH])
@pytest.mark.parametrize("name", sorted(ref.BATCHES))
def test_plan_launch_log_in_every_context(name, kind):
    """the whole batch at five pitches in the three contexts, the prefixes at two pitches: one-wave kernel
    <ARITH, KIND, LOG = true, false> for each (the source kind always runs the exact one).  The log does not depend on
    the context; the fused kind's PCM is the oracle's in EXACT and, in FMA and F32, what the same context's one-wave
    kernel gives without a log"""
    b = batch(name)
    nl = len(b.lanes)
    mid = int(b.ncyc[nl // 2])
    pitches = (1, 7, mid, LOG_PITCH, 333)
    logs = {}
    for arith in ARITHS:
        with vs.Engine(0, arith=arith) as eng:
            want_out = b.flow if kind == vs.VS_KIND_SOURCE else _pcm(name)
            if kind == vs.VS_KIND_SYNTH and arith != vs.VS_ARITH_EXACT:
                eng.set_tuning(kernel=vs.VS_KERNEL_SINGLE)
                with eng.plan(b.lanes, b.n) as plain:
                    pname = plain.kernel_name(kind)
                    assert pname.startswith("vs_synth_kernel<%d, 0, false, " % vs.VS_ARITH_FMA), pname
                    want_out = _canary_launch(eng, plain, nl, b.n, kind, counts=False)[0][:nl]
                eng.set_tuning()
            total = 0
            with eng.plan(b.lanes, b.n) as plan:
                for pitch in pitches:
                    want_recs, want_ncyc = b.want(pitch)
                    out, log, cnt = _canary_launch(eng, plan, nl, b.n, kind, pitch)
                    total += _held(out, log, cnt, want_out, want_recs, want_ncyc, pitch, (name, KIND_NAME[kind], ARITH_NAME[arith], pitch))
                    logs.setdefault(pitch, log)
                    assert np.array_equal(log, logs[pitch]), (pitch, ARITH_NAME[arith])     # the same bytes in all three contexts
            # partial wavefronts: rows and slots behind the batch are the caller's
            shapes = 0
            for k in PREFIXES:
                with eng.plan(b.lanes[:k], b.n) as plan:
                    for pitch in (7, LOG_PITCH):
                        want_recs, want_ncyc = b.want(pitch)
                        out, log, cnt = _canary_launch(eng, plan, k, b.n, kind, pitch)
                        # (FMA, F32: a lane's PCM does not depend on the batch it is launched in)
                        total += _held(out, log, cnt, want_out[:k], want_recs[:k], want_ncyc[:k], pitch,
                                       (name, KIND_NAME[kind], ARITH_NAME[arith], k, pitch))
                        shapes += 1
            print("vs_plan_launch with a log, %s, %s, VS_ARITH_%s: %d lanes at pitches %s and the prefixes %s at 7 and %d: "
                  "%d records (nothing behind them in canary-filled rows), the counts and the %s equal %s" % (
                      name, KIND_NAME[kind], ARITH_NAME[arith], nl, list(pitches), list(PREFIXES), LOG_PITCH, total,
                      "flow" if kind == vs.VS_KIND_SOURCE else "PCM",
                      "the oracle" if kind == vs.VS_KIND_SOURCE or arith == vs.VS_ARITH_EXACT else "the oracle (log, counts) and the one-wave kernel without a log (PCM)"))


# c ---- the pre-emphasis-1 instantiation

def test_log_with_the_pre_emphasis_1_instantiation():
    import test_synth_hostile_ref as hostile
    c = hostile.hcase("h22p1")
    ns, nl = hostile.NS, hostile.BATCH
    assert all(l.pre_emphasis == 1.0 for l in c.lanes)
    want_pcm, f = c.want("exact")
    seen = hostile.compared(f, ns)                     # a row is promised up to the first state that is not finite
    with vs.Engine(0) as eng:
        eng.set_tuning(kernel=vs.VS_KERNEL_SINGLE)
        with eng.plan(c.lanes, ns) as plan:
            assert plan.kernel_name(vs.VS_KIND_SYNTH) == "vs_synth_kernel<0, 0, false, true>"
            total = 0
            for pitch in (3, 40):
                want_recs, want_ncyc = _want(c.lanes, ns, pitch)
                out, log, cnt = _canary_launch(eng, plan, nl, ns, vs.VS_KIND_SYNTH, pitch)
                total += _held(out, log, cnt, None, want_recs, want_ncyc, pitch, ("h22p1", pitch))
                bad = (out[:nl] != want_pcm) & seen
                assert not bad.any(), np.argwhere(bad)[:8]
            assert want_ncyc.max() < 40 and want_ncyc.min() > 3
        print("vs_synth_kernel<0, 0, true, true> (h22p1 of tests/test_synth_hostile_ref.py, %d lanes x %d samples, pitches 3 and 40): "
              "%d records, the counts and %d samples of PCM equal the oracle" % (nl, ns, total, int(seen.sum())))


# d ---- vowel -n behind a launch with a log

def test_output_noise_passes_behind_a_launch_with_a_log(engine):
    b = batch("CORNER")
    nl = len(b.lanes)
    lanes = (vs.Lane * nl)()
    for i, l in enumerate(b.lanes):
        C.memmove(C.byref(lanes[i]), C.byref(l), C.sizeof(vs.Lane))
        if i % 2 == 0:
            lanes[i].out_snr = 100.0                     # vowel -n 20
    assert sum(1 for l in lanes if l.out_snr > 0) >= nl // 2 and len({l.fs for l in lanes}) > 1     # frames of several lengths
    want_pcm = po.synth(lanes, b.n)
    assert (want_pcm[::2] != _pcm("CORNER")[::2]).any(axis=1).sum() > nl // 8        # the noise is in the samples
    with engine.plan(lanes, b.n) as plan:
        name = plan.kernel_name(vs.VS_KIND_SYNTH)
        assert name.endswith("vs_out_noise_kernel"), name
        total = 0
        for pitch in (7, LOG_PITCH):
            want_recs, want_ncyc = b.want(pitch)
            out, log, cnt = _canary_launch(engine, plan, nl, b.n, vs.VS_KIND_SYNTH, pitch)
            total += _held(out, log, cnt, want_pcm, want_recs, want_ncyc, pitch, ("CORNER + vowel -n", pitch))
    print("SYNTH with a log and vowel -n on every other lane (CORNER, %d lanes, pitches 7 and %d): %d records, the counts "
          "and the PCM equal the oracle" % (nl, LOG_PITCH, total))


# e ---- the narrow build

def test_log_of_the_narrow_build(engine):
    fa = ["-r", "48000", "-d", "0.6", "-f", "50", "-g", "52", "-j", "5", "-s", "10", "-n", "15"]
    lanes = [vs.lane_from_cli(fa, ["-v", "aiu1234567"[seed % 10], "-g", "2"], 300 + seed)[0] for seed in range(21)]
    n = 8000
    flow, pcm = po.source(lanes, n), po.synth(lanes, n)
    with engine.plan(lanes, n) as plan:
        assert "narrow build" in plan.kernel_name(vs.VS_KIND_SYNTH) and "narrow build" in plan.kernel_name(vs.VS_KIND_SOURCE)
        total = 0
        for pitch in (4, 16):
            want_recs, want_ncyc = _want(lanes, n, pitch)
            for kind, want_out in ((vs.VS_KIND_SOURCE, flow), (vs.VS_KIND_SYNTH, pcm)):
                out, log, cnt = _canary_launch(engine, plan, len(lanes), n, kind, pitch)
                total += _held(out, log, cnt, want_out, want_recs, want_ncyc, pitch, ("narrow", KIND_NAME[kind], pitch))
        assert want_ncyc.min() > 4 and want_ncyc.max() < 16 and bool(((want_recs["w_pow"] > 0) & (want_recs["S"] != 0)).any())
    print("the narrow build (16 utterances per wavefront; 21 lanes at 48 kHz, F0 50 Hz, %d samples; SOURCE and SYNTH at pitches "
          "4 and 16): %d records, the counts, the flow and the PCM equal the oracle" % (n, total))


# f ---- the wide plan

def test_log_of_the_wide_plan(engine):
    orders = [1, 2, 5, 21, 22, 23, 24, 30, 31, 39, 40]
    lanes, fs, dur = configs.wide_order_lanes([orders[i % len(orders)] for i in range(70)])
    assert all((l.flags & vs.VS_FLAG_SHIMMER) and (l.flags & vs.VS_FLAG_NOISE) and l.shimmer != 0.0 for l in lanes)
    n = 5000
    pcm = po.synth(lanes, n)
    with engine.plan(lanes, n) as plan:
        name = plan.kernel_name(vs.VS_KIND_SYNTH)
        assert name.startswith("vs_synth_kernel<0, 1, false, false> + ") and name.split(" + ")[-1].startswith("vs_filter_wide_kernel<"), name
        total = 0
        for pitch in (7, 60):
            want_recs, want_ncyc = _want(lanes, n, pitch)
            out, log, cnt = _canary_launch(engine, plan, 70, n, vs.VS_KIND_SYNTH, pitch)
            total += _held(out, log, cnt, pcm, want_recs, want_ncyc, pitch, ("wide", pitch))
        assert want_ncyc.min() > 7 and want_ncyc.max() < 60
    print("the wide plan (%s; 70 lanes x %d samples, pitches 7 and 60): %d records and the counts from the source step, and "
          "the PCM, equal the oracle" % (name, n, total))


# g ---- the counts of the kernels that keep no log

WS_TUNINGS = {"auto": dict(kernel=vs.VS_KERNEL_AUTO), "single": dict(kernel=vs.VS_KERNEL_SINGLE),
              "ws2": dict(kernel=vs.VS_KERNEL_WS, ws_roles=2), "ws3": dict(kernel=vs.VS_KERNEL_WS, ws_roles=3)}


def _fused_name(plan, tuning, lanes):
    """the first kernel of the fused launch is the family the tuning asks for"""
    name = plan.kernel_name(vs.VS_KIND_SYNTH)
    first = name.split(" + ")[0]
    pre1 = "true" if all(l.pre_emphasis == 1.0 for l in lanes) else "false"
    if tuning == "single":
        assert first == "vs_synth_kernel<0, 0, false, %s>" % pre1, name
    elif tuning == "auto":
        assert first in ["vs_synth_ws%s_kernel<0, %s, %d>" % (p, pre1, r) for p in ("", "_pow") for r in (2, 3)], name
    else:
        assert first in ["vs_synth_ws%s_kernel<0, %s, %s>" % (p, pre1, tuning[2]) for p in ("", "_pow")], name
    return first


@pytest.mark.parametrize("tuning", sorted(WS_TUNINGS))
def test_counts_of_a_launch_without_a_log(tuning):
    b = batch("FUZZ")
    pcm = _pcm("FUZZ")
    with vs.Engine(0) as eng:
        eng.set_tuning(**WS_TUNINGS[tuning])
        names = []
        for k in (len(b.lanes), 1, 63, 65, 130):
            with eng.plan(b.lanes[:k], b.n) as plan:
                names.append(_fused_name(plan, tuning, b.lanes[:k]))
                out, _, cnt = _canary_launch(eng, plan, k, b.n, vs.VS_KIND_SYNTH)
            assert np.array_equal(cnt[:k], b.ncyc[:k]), (tuning, k, np.flatnonzero(cnt[:k] != b.ncyc[:k])[:8])
            assert cnt[k] == CANARY32
            assert np.array_equal(out[:k], pcm[:k]), (tuning, k)
        # one frame length and vowel -n on every lane: the filter wavefronts take the frame powers along
        specs, fs, dur, _ = configs.config_specs(3, 130, out_noise_db=20)
        lanes, d = vs.lanes_from_specs(specs)
        n = 6000
        if tuning != "single":
            with eng.plan(lanes, n) as plan:
                first = _fused_name(plan, tuning, lanes)
                assert first.startswith("vs_synth_ws_pow_kernel<0, "), first
                names.append(first)
                out, _, cnt = _canary_launch(eng, plan, 130, n, vs.VS_KIND_SYNTH)
            want_ncyc = _want(lanes, n, 1)[1]
            assert np.array_equal(cnt[:130], want_ncyc) and cnt[130] == CANARY32
            assert np.array_equal(out[:130], po.synth(lanes, n))
        print("counts without a log, tuning %s: FUZZ whole and the prefixes 1, 63, 65, 130%s: %s -- the counts and the PCM "
              "equal the oracle, the element behind them is the caller's" % (
                  tuning, "" if tuning == "single" else ", and 130 lanes of config 3 with vowel -n 20", sorted(set(names))))


# h ---- the program that prints the log

@functools.lru_cache(maxsize=None)
def _program_lines():
    """12 of the recorded command lines of tests/test_cycle_log_ref.py: four whose log prints -nan lines, four with inf
    lines, four that draw their noise in the general order (T4 > 0)"""
    runs, _ = ref.reference_log_runs()
    runs = [r for r in runs if r[4]["rc"] == 0 and r[4]["done"]]
    nan = [i for i, r in enumerate(runs) if b"SNRdb =  -nan\n" in r[5]][:4]
    inf = [i for i, r in enumerate(runs) if b"SNRdb =   inf\n" in r[5] and i not in nan][:4]
    t4 = [i for i, r in enumerate(runs) if r[8] and i not in nan and i not in inf][:4]
    assert len(nan) == 4 and len(inf) == 4 and len(t4) == 4
    return [runs[i] for i in nan + inf + t4]


@pytest.mark.parametrize("index", range(12))
def test_flowgen_shimmer_prints_the_log_as_the_reference_does(tmp_path, index):
    fa, seed, lane, n, rec, text, flow, nd, t4 = _program_lines()[index]
    g = rec["files"]["g.wav"]
    for header in (44, 72):
        env = dict(os.environ, VS_SEED=str(seed), VS_WAV_HEADER=str(header))
        r = subprocess.run([os.path.join(BIN, "flowgen_shimmer"), "-o", "g.wav"] + list(fa), cwd=tmp_path, env=env,
                           capture_output=True, timeout=120)
        raw = open(tmp_path / "g.wav", "rb").read()
        assert r.returncode == rec["rc"], r.stderr
        assert po.digest(r.stdout) == rec["stdout_sha256"], (fa, seed, header)
        assert len(raw) == header + 2 * g["n"] and po.digest(raw[header:]) == g["payload_sha256"], (fa, seed, header)
        if header == 72:
            assert raw[:72].hex() == g["header"]
    kind = "-nan lines" if index < 4 else ("inf lines" if index < 8 else "T4 > 0")
    print("flowgen_shimmer %s (VS_SEED %d; %s): stdout (%d bytes), payload and return code equal the recorded reference "
          "run with both header sizes" % (" ".join(fa), seed, kind, len(text)))
