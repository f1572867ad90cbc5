"""PSOLA with a time map on the device (csrc/vs_psola_ts.hip) against the restatement (tests/psola_ts_ref.py), byte for
byte: the output rows, the status records and the synthesis records.  Drawn hostile rows (the marks, runs and targets of
the PSOLA tests' rows) with drawn maps of 2 to 5 anchors, frozen pieces and every kind of invalid map; output lengths around
the overlap-add kernel's tile, shorter and longer than the input; output rows at several pitches and odd bases; dense
marks that take several stagings; the identity map against vs_psola_launch; the whole chain behind the source track; the
host-buffer call; the program.  Every output sits inside a guard band and what a launch must not write keeps its
sentinel."""
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_support as gs  # noqa: E402
import guided_ref as gr  # noqa: E402
import pitch_signals as ps  # noqa: E402
import psola_ref as pp  # noqa: E402
import psola_ts_ref as pt  # noqa: E402
import strack_ref as sr  # noqa: E402
import test_gpu_psola as base  # noqa: E402  (its drawn rows, its record comparisons, its WAV helpers)

pytestmark = pytest.mark.gpu
S8 = base.S8
TILE = 2048                  # VS_PS_TILE
NS, NO = 3000, 6100          # the widths of the input and of the output rows
MAP_PITCH = 6

sentinel_records, same_records = base.sentinel_records, base.same_records


@pytest.fixture(scope="module")
def eng():
    e = vs.Engine(0)
    yield e
    e.close()


def run_dev(eng, b, pitch, offset_bytes, segs=True, gain=True, in_pitch=None):
    """vs_psola_ts_launch of the batch b on device pointers: the output rows in GuardedRows at that pitch and base, the
    PCM staged at in_pitch between padding that is not silence, the status and synthesis records in sentinel-filled
    memory"""
    n, ns = b["x"].shape
    no = b["no"]
    in_pitch = ns if in_pitch is None else in_pitch
    out = gs.GuardedRows(n, no, pitch, offset_bytes)
    sp = b["sp"]
    with eng.scope() as dev:
        out.on(dev)
        d_x = dev.put(gs.staged_input(b["x"], in_pitch)) + 2 * gs.GUARD
        d_mk, d_rec = dev.put(b["marks"]), dev.put(b["rec"])
        d_sg = dev.put(b["segs"]) if segs else None
        d_st, d_T, d_cnt = dev.put(b["start"]), dev.put(b["T"]), dev.put(b["count"])
        d_g = dev.put(b["gain"]) if gain else None
        d_an, d_w = dev.put(b["anchors"]), dev.put(b["n_anchors"])
        d_stat = dev.filled(n * vs.PSOLA_STAT_DTYPE.itemsize, S8, np.uint8)
        d_sy = dev.filled(n * sp * vs.PSOLA_MARK_DTYPE.itemsize, S8, np.uint8)
        eng.psola_ts_dev(d_x, in_pitch, n, ns, d_mk, b["marks"].shape[1], d_rec, d_st, 4, d_T, 4, d_cnt, 4,
                         b["start"].shape[1], d_an, d_w, b["anchors"].shape[1], out.first(pitch, offset_bytes), pitch, no,
                         d_stat, d_sy, sp, segs_ptr=d_sg, seg_pitch=b["segs"].shape[1] if segs else 0, gain_ptr=d_g,
                         gain_stride=4 if gain else 0, lengths=b["lengths"], out_lengths=b["out_lengths"], pmin=b["pmin"],
                         pmax=b["pmax"], unvoiced_period=b["U"])
        eng.synchronize()
        y = out.rows_back(pitch, offset_bytes, (pitch, offset_bytes)).copy()
        stat = dev.get(d_stat, (n,), vs.PSOLA_STAT_DTYPE)
        sy = dev.get(d_sy, (n, sp), vs.PSOLA_MARK_DTYPE)
    return y, stat, sy


def expected(b, segs=True, gain=True):
    n = len(b["x"])
    return pt.psola_ts(b["x"], b["lengths"], b["no"], b["out_lengths"], b["marks"], b["rec"], b["segs"] if segs else None,
                       b["start"], b["T"], b["gain"] if gain else None, b["count"], b["anchors"], b["n_anchors"], b["pmin"],
                       b["pmax"], b["U"], b["sp"], out=np.full((n, b["no"]), gs.SENTINEL, dtype=np.int16),
                       synth=sentinel_records((n, b["sp"]), pt.MARK_DTYPE))


def same(got, want, what=""):
    y, st, sy = got
    wy, wst, wsy = want
    same_records(st, wst.astype(vs.PSOLA_STAT_DTYPE), what + " stat")
    same_records(sy, wsy.astype(vs.PSOLA_MARK_DTYPE), what + " synth")
    gs.same_rows(y, wy, what + " y")


# ---- the batch: 68 rows of at most 3000 samples, output rows of at most 6100 ----

FLAWS = ("one anchor", "more than the pitch", "u_0", "v_0", "u_last", "v_last", "u repeats", "v falls")


def drawn_map(rng, length, len_out, flaw=None):
    """(anchors [MAP_PITCH], W): 2 to 5 anchors from (0, 0) to (len_out, length), one piece in three frozen; flaw: one of
    FLAWS"""
    W = min(int(rng.integers(2, 6)), len_out + 1)
    an = np.zeros(MAP_PITCH, dtype=pt.ANCHOR_DTYPE)
    an["u"], an["v"] = rng.integers(-5, 7000, MAP_PITCH), rng.integers(-5, 4000, MAP_PITCH)   # (what lies past W)
    if W < 2:
        an[0], an[1] = (0, 0), (len_out, length)              # len_out = 0: u cannot increase
        return an, 2
    u = [0] + sorted(int(q) for q in rng.choice(np.arange(1, len_out), W - 2, replace=False)) + [len_out]
    v = [0] + sorted(int(q) for q in rng.integers(0, length + 1, W - 2)) + [length]
    for j in range(1, W):
        if rng.random() < 0.33 and j < W - 1:
            v[j] = v[j - 1]                                   # a frozen piece
    if rng.random() < 0.2 and W > 2:
        v[W - 2] = length                                     # frozen at the end: Minv(len) is len_out all the same
    if flaw == "one anchor":
        W = 1
    elif flaw == "more than the pitch":
        W = MAP_PITCH + 1
    elif flaw == "u_0":
        u[0] = -1
    elif flaw == "v_0":
        v[0] = -1
    elif flaw == "u_last":
        u[-1] += int(rng.choice([-1, 1]))
    elif flaw == "v_last":
        v[-1] += int(rng.choice([-1, 1]))
    elif flaw == "u repeats":
        u = u[:1] + u
        v = v[:1] + v
        W += 1
    elif flaw == "v falls":
        u, v, W = [0, max(1, len_out // 2), max(2, len_out)], [0, length, length - 1], 3
        if len_out < 2:
            u = [0, 1, 1]
    k = min(len(u), MAP_PITCH)
    an["u"][:k], an["v"][:k] = u[:k], v[:k]
    return an, W


def make_batch():
    rng = np.random.default_rng(20262)
    n, mp, sgp, tp = 68, 160, 5, 200
    b = dict(x=np.zeros((n, NS), np.int16), lengths=np.zeros(n, np.int32), marks=np.full((n, mp), -1, np.int32),
             rec=np.zeros(n, vs.GUIDED_REC_DTYPE), segs=np.zeros((n, sgp), vs.GUIDED_SEG_DTYPE),
             start=np.zeros((n, tp), np.int32), T=np.zeros((n, tp), np.int32), gain=np.zeros((n, tp), np.int32),
             count=np.zeros(n, np.int32), pmin=32, pmax=320, sp=64, U=80, no=NO,
             out_lengths=np.zeros(n, np.int32), anchors=np.zeros((n, MAP_PITCH), pt.ANCHOR_DTYPE),
             n_anchors=np.zeros(n, np.int32))
    # the three signals of the definition's consequences, cut to the batch's width, with the restatement's guided marks:
    # twice as long, half as long, three anchors, the identity
    train = ps.train([123] * 100, lambda p: int(0.6 * p), lambda c: 8000.0)[0]
    g = ps.gaps()                # cut to 10 cycles, 400 zeros, 400 samples of the noise, 8 cycles
    gaps = np.concatenate([g[:1230], g[7380:7780], g[11380:11780], g[-970:]])
    signals = [(ps.glide()[0][:NS], 2 * NS), (gaps, 2 * NS), (train[:NS], NS // 2), (train[:TILE + 1], NO),
               (gaps, NS), (gaps, 2001)]
    T140 = rng.integers(119, 128, tp)
    for i, (s, len_out) in enumerate(signals):
        out, mk, rec, sg, _ = gr.track_and_guided(s[None], 16000, marks=mp, segs=sgp)
        b["x"][i, :len(s)] = s
        b["lengths"][i] = len(s)
        b["marks"][i], b["rec"][i], b["segs"][i] = mk[0], tuple(rec[0]), sg[0]
        b["T"][i] = T140
        b["start"][i] = np.cumsum(T140) - T140
        b["gain"][i] = rng.integers(int(0.85 * pp.Q), int(1.15 * pp.Q) + 1, tp)
        b["count"][i] = tp if i != 1 else 0
        b["out_lengths"][i] = len_out
        b["anchors"][i, 1] = (len_out, len(s))
        b["n_anchors"][i] = 2
    b["anchors"][5, :3] = [(0, 0), (1500, 1500), (2001, NS)]  # the first half as it is, the second three times as fast
    b["n_anchors"][5] = 3
    assert (b["rec"]["n_marks"][:6] < mp).all() and (b["rec"]["n_segments"][:6] >= 1).all()
    fixed_out = [0, 1, 2, TILE - 1, TILE, TILE + 1, NO, NO - 1]
    for i in range(len(signals), n):
        x, length, marks, nseg, nm, segs, start, T, gain, count = base.drawn_row(rng, i, NS, mp, sgp, tp)
        length = min(length, NS)
        b["x"][i], b["lengths"][i] = x, length
        b["marks"][i, :len(marks)] = marks
        b["rec"][i] = (nseg, nm, 0, 0)
        b["segs"]["first_mark_index"][i], b["segs"]["n_marks"][i] = [s[0] for s in segs], [s[1] for s in segs]
        b["start"][i], b["T"][i], b["gain"][i], b["count"][i] = start, T, gain, count
        j = i - len(signals)
        len_out = fixed_out[j] if j < len(fixed_out) else int(rng.integers(1, NO + 1))
        if j >= len(fixed_out) and rng.random() < 0.3:
            len_out = max(1, length // int(rng.integers(2, 40)))      # heavy compression: stretches without marks
        flaw = FLAWS[j - 20] if 20 <= j < 20 + len(FLAWS) else None
        b["out_lengths"][i] = len_out
        b["anchors"][i], b["n_anchors"][i] = drawn_map(rng, length, len_out, flaw)
    return b


@pytest.fixture(scope="module")
def batch():
    b = make_batch()
    return dict(b=b, full=expected(b), no_segs=expected(b, segs=False), no_gain=expected(b, gain=False))


def test_the_batch_is_what_it_claims(batch):
    """no GPU work: the restatement's answers cover the status bits, voiced and unvoiced marks, flips, clamps, the
    output lengths around the tile, maps of every count, frozen pieces, boundaries behind stretches without marks"""
    b = batch["b"]
    y, st, sy = batch["full"]
    s = st["status"]
    for bit in (pt.BAD_RUN, pt.OVERFLOW, pt.NO_RUN, pt.BAD_MAP):
        assert (s & bit).any(), bit
    assert (s == 0).any() and ((s & pt.BAD_MAP) != 0).sum() >= len(FLAWS) + 1 and len(b["x"]) > 64
    assert (st["n_runs_done"] > 1).any() and (st["n_clipped"] > 0).any() and (st["n_governed"] > 0).any()
    assert st["n_synth"].max() > b["sp"] - 15
    lo, ln = b["out_lengths"], b["lengths"]
    for want in (0, 1, 2, TILE - 1, TILE, TILE + 1, NO):
        assert (lo == want).any(), want
    ok = (s & (pt.BAD_MAP | pt.OVERFLOW)) == 0
    assert (ok & (lo < ln)).any() and (ok & (lo > ln)).any() and (lo > 2 * TILE).any() and (ln == 0).any()
    for W in (2, 3, 4, 5):
        assert (ok & (b["n_anchors"] == W)).any(), W
    frozen = [i for i in np.flatnonzero(ok) if (np.diff(b["anchors"]["v"][i, :b["n_anchors"][i]]) == 0).any()]
    assert len(frozen) >= 3
    codes = [sy["cycle"][i, :st["n_synth"][i]] for i in range(len(st))]
    assert sum((c == pt.UNVOICED_FLIP).sum() for c in codes) > 50 and sum((c == pt.UNVOICED).sum() for c in codes) > 200
    assert sum((c >= 0).sum() for c in codes) > 200 and sum((c == -1).sum() for c in codes) > 200
    for i in np.flatnonzero(ok & (ln > 0)):
        k = st["n_synth"][i]
        t = sy["t"][i, :k]
        assert t[0] == 0 and t[-1] == lo[i] and (np.diff(t) > 0).all() and np.diff(t).max() <= 3 * pt.MAX_LAG // 2, i
        assert sy["cycle"][i, k - 1] == pt.RUN_END and (y[i, lo[i]:] == gs.SENTINEL).all()
    # rows in which a stretch has no marks: fewer unvoiced-or-voiced changes in the records than stretches in the chain
    skipped = 0
    for i in np.flatnonzero(ok & (ln > 0)):
        runs = pp.runs_of(b["rec"]["n_segments"][i], b["rec"]["n_marks"][i], b["segs"][i], b["marks"].shape[1])
        chain, _, _ = pt.stretches(int(ln[i]), b["marks"][i], runs, b["U"])
        mp = pt.map_of(b["anchors"][i], b["n_anchors"][i], int(ln[i]), int(lo[i]))
        skipped += sum(pt.Minv(mp, c[1][-1]) <= pt.Minv(mp, c[1][0]) for c in chain)
    assert skipped >= 5


@pytest.mark.parametrize("pitch,offset_bytes", ((NO, 0), (NO + 3, 2), (NO + 8, 6), (NO + 1, 14)))
def test_device_is_the_restatement(eng, batch, pitch, offset_bytes):
    same(run_dev(eng, batch["b"], pitch, offset_bytes, in_pitch=NS + (offset_bytes // 2)), batch["full"])


def test_without_segment_records_and_without_gains(eng, batch):
    for key, kw in (("no_segs", dict(segs=False)), ("no_gain", dict(gain=False))):
        same(run_dev(eng, batch["b"], NO + 5, 4, **kw), batch[key], key)


def test_the_host_path_is_the_device_path(eng, batch):
    b = batch["b"]
    n = len(b["x"])
    got = eng.psola_ts(b["x"], 16000, b["marks"], b["rec"], b["start"], b["T"], b["anchors"], b["n_anchors"], NO,
                       out_lengths=b["out_lengths"], count=b["count"], segs=b["segs"], gain=b["gain"], lengths=b["lengths"],
                       synth=b["sp"], pmin=b["pmin"], pmax=b["pmax"], unvoiced_period=b["U"],
                       out=np.full((n, NO), gs.SENTINEL, np.int16),
                       synth_fill=sentinel_records((n, b["sp"]), vs.PSOLA_MARK_DTYPE))
    same(got, batch["full"])


def test_the_identity_map_is_psola_on_the_device(eng, batch):
    """every row's own length and two anchors: y and n_clipped of vs_psola_launch on the same rows, for this target and
    two unvoiced periods"""
    b = dict(batch["b"])
    n = len(b["x"])
    b["no"], b["out_lengths"], b["sp"] = NS, b["lengths"].copy(), 400
    b["anchors"], b["n_anchors"] = vs.psola_two_anchors(b["lengths"], b["lengths"], MAP_PITCH)
    wy, wst, _ = base.run_dev(eng, b, NS + 2, 2)
    for U in (80, 37):
        b["U"] = U
        y, st, _ = run_dev(eng, b, NS + 2, 2)
        rows = np.flatnonzero(b["lengths"] > 0)               # (a row of length 0 has no valid map)
        assert (st["status"][rows] & (pt.BAD_MAP | pt.OVERFLOW) == 0).all() and (wst["status"] & pp.OVERFLOW == 0).all()
        gs.same_rows(y[rows], wy[rows], "y")
        assert np.array_equal(st["n_clipped"][rows], wst["n_clipped"][rows]) and (wst["n_clipped"] > 0).any()
        assert (y[b["lengths"] == 0] == gs.SENTINEL).all()
    assert (wst["n_governed"] > 0).any() and len(rows) > n - 6


def test_dense_marks_take_several_stagings(eng):
    """U = 2 on rows without runs, and marks 1 to 3 samples apart: more than VS_PS_STAGE synthesis marks in one tile, and
    more than one round of the section"""
    rng = np.random.default_rng(8)
    n, ns, no, mp, tp, sp = 4, 1500, 2600, 900, 4, 2700
    b = dict(x=rng.integers(-20000, 20001, (n, ns)).astype(np.int16), lengths=np.array([ns, ns - 1, 1200, 900], np.int32),
             marks=np.full((n, mp), -1, np.int32), rec=np.zeros(n, vs.GUIDED_REC_DTYPE),
             segs=np.zeros((n, 1), vs.GUIDED_SEG_DTYPE), start=np.zeros((n, tp), np.int32), T=np.ones((n, tp), np.int32),
             gain=np.zeros((n, tp), np.int32), count=np.zeros(n, np.int32), pmin=2, pmax=2048, sp=sp, U=2, no=no,
             out_lengths=np.array([no, 2049, 2500, 700], np.int32))
    for i in (1, 3):                                          # rows 0 and 2 have no run: unvoiced marks 2 samples apart
        m = 3 + np.concatenate([[0], np.cumsum(rng.integers(1, 4, mp - 1))])
        m = m[m < b["lengths"][i]]
        b["marks"][i, :len(m)] = m
        b["rec"][i] = (1, len(m), 0, 0)
    b["anchors"], b["n_anchors"] = vs.psola_two_anchors(b["lengths"], b["out_lengths"], 3)
    b["anchors"][2, :3] = [(0, 0), (2000, 300), (2500, 1200)]
    b["n_anchors"][2] = 3
    want = expected(b, segs=False, gain=False)
    wst = want[1]
    assert wst["n_synth"].min() > 300 and wst["n_synth"].max() > 1200 and (wst["status"] & ~(pt.NO_RUN | pt.BAD_RUN) == 0).all()
    same(run_dev(eng, b, no + 6, 10, segs=False, gain=False), want)


def test_both_instantiations_of_the_shared_core_on_the_same_rows(eng):
    """The two overlap-add kernels are one core (csrc/vs_psola_dev.h) with a switch; here both run on the same three rows
    of 2300 samples, a little more than a tile -- a run in the middle, two runs with a gap, no run -- and each is held
    to its own restatement: PSOLA copies x in front of a run, behind it, in the gap and in the row without a run (the
    run-end bit), the time map with the identity map fills the same places with unvoiced grains.  The launches are not
    compared with each other (test_the_identity_map_is_psola_on_the_device does that where they must agree); the
    restatements say where they may differ.  With the identity map the unvoiced marks fall on their analysis marks, so
    no grain is flipped, and every row has records, so no sample is silence: those two branches are the batch's
    (test_the_batch_is_what_it_claims counts its flips, its rows with a bad map have no record and come back as zeros)."""
    rng = np.random.default_rng(77)
    n, ns, mp, sgp, tp, sp, pitch, off = 3, 2300, 24, 2, 24, 96, 2303, 2
    b = dict(x=rng.integers(-12000, 12001, (n, ns)).astype(np.int16), lengths=np.full(n, ns, np.int32),
             marks=np.full((n, mp), -1, np.int32), rec=np.zeros(n, vs.GUIDED_REC_DTYPE),
             segs=np.zeros((n, sgp), vs.GUIDED_SEG_DTYPE), start=np.zeros((n, tp), np.int32),
             T=np.zeros((n, tp), np.int32), gain=np.zeros((n, tp), np.int32), count=np.full(n, tp, np.int32), pmin=32,
             pmax=320, sp=sp, U=80, no=ns, out_lengths=np.full(n, ns, np.int32))
    runs = ([np.arange(700, 1501, 100)], [np.arange(200, 801, 120), np.arange(1400, 2101, 100)], [])
    for i, row in enumerate(runs):
        at = 0
        for q, m in enumerate(row):
            b["marks"][i, at:at + len(m)] = m
            b["segs"]["first_mark_index"][i, q], b["segs"]["n_marks"][i, q] = at, len(m)
            at += len(m)
        b["rec"][i] = (len(row), at, 0, 0)
    T = rng.integers(95, 111, tp)
    b["T"][:], b["start"][:] = T, np.cumsum(T) - T
    b["gain"][:] = rng.integers(int(0.9 * pp.Q), int(1.1 * pp.Q) + 1, tp)
    b["anchors"], b["n_anchors"] = vs.psola_two_anchors(b["lengths"], b["out_lengths"], MAP_PITCH)
    want_ps, want_ts = base.expected(b), expected(b)
    (py, pst, psy), (ty, tst, tsy) = want_ps, want_ts
    # what the restatements hold: the runs done, run ends in PSOLA's records, unvoiced marks in the time map's, PSOLA's
    # copy regions, and the time map's rows ending in one last record
    assert list(pst["n_runs_done"]) == [1, 2, 0] and list(tst["n_runs_done"]) == [1, 2, 0]
    assert pst["status"][2] == pp.NO_RUN and tst["status"][2] == pt.NO_RUN and (pst["status"][:2] == 0).all()
    assert [(psy["cycle"][i, :pst["n_synth"][i]] == pp.RUN_END).sum() for i in range(n)] == [1, 2, 0]
    assert all((tsy["cycle"][i, :tst["n_synth"][i]] == pt.UNVOICED).sum() >= 8 for i in range(n))
    assert all((tsy["cycle"][i, :tst["n_synth"][i]] == pt.RUN_END).sum() == 1 for i in range(n))
    assert (pst["n_governed"][:2] > 3).all() and (tst["n_governed"][:2] > 3).all()
    x = b["x"]
    assert np.array_equal(py[0, :700], x[0, :700]) and np.array_equal(py[0, 1500:], x[0, 1500:])
    assert np.array_equal(py[1, 800:1400], x[1, 800:1400]) and np.array_equal(py[2], x[2])
    # where the two may differ: somewhere in row 1's gap, or nowhere
    assert (py[1, 800:1400] != ty[1, 800:1400]).any() or np.array_equal(py, ty)
    same(base.run_dev(eng, b, pitch, off), want_ps, "psola")
    same(run_dev(eng, b, pitch, off), want_ts, "psola_ts")


# ---- the whole chain on the device: pitch -> guided -> source track -> psola_ts, the target read in place ----

def test_chained_behind_the_source_track(eng):
    fs, ns, n, no = 16000, 3000, 4, 4500
    train = ps.train([123] * 100, lambda p: int(0.6 * p), lambda c: 8000.0)[0]
    x = np.stack([train[:ns], ps.glide()[0][:ns], ps.gaps()[5000:5000 + ns], np.zeros(ns, np.int16)])
    lanes = [vs.lane_from_cli(["-j", j, "-r", "16000"], ["-v", "a"], seed=700 + k)[0] for k, j in enumerate(("2", "0.5", "3", "2"))]
    # the target is in output time: the source track runs over the output's length, on the lags of the output's frames
    row = vs.strack_row_from_pitch(fs, no)
    rin = vs.strack_row_from_pitch(fs, ns)
    fp_in, mp, sgp, cp, sp = int(rin["n_frames"]), 140, 4, 150, 260
    an, w = vs.psola_two_anchors([ns] * n, [no] * n)
    out = gs.GuardedRows(n, no, no + 3, 2)
    with eng.scope() as dev:
        out.on(dev)
        d_x = dev.put(x)
        d_fr = dev.put(np.zeros((n, fp_in), vs.PITCH_FRAME_DTYPE))
        d_meas = dev.room(n * vs.ACOUSTIC_DTYPE.itemsize)
        d_mk = dev.filled(n * mp, -1, np.int32)
        d_rec = dev.room(n * vs.GUIDED_REC_DTYPE.itemsize)
        d_sg = dev.put(np.zeros((n, sgp), vs.GUIDED_SEG_DTYPE))
        d_flow = dev.room(n * no * 2)
        d_sst = dev.room(n * vs.STRACK_STAT_DTYPE.itemsize)
        d_cyc = dev.filled(n * cp * vs.STRACK_CYCLE_DTYPE.itemsize, S8, np.uint8)
        d_stat = dev.filled(n * vs.PSOLA_STAT_DTYPE.itemsize, S8, np.uint8)
        d_sy = dev.filled(n * sp * vs.PSOLA_MARK_DTYPE.itemsize, S8, np.uint8)
        d_an, d_w = dev.put(an), dev.put(w)
        eng.pitch_dev(d_x, ns, n, ns, fs, fp_in, d_fr)
        eng.measure_guided_dev(d_x, ns, n, ns, fs, d_fr, fp_in, d_meas, d_rec, d_mk, mp, d_sg, sgp)
        # a contour for the output: the input's frames, each held for 3/2 of its hop (the hop of a row in output time)
        lag_at = vs.PITCH_FRAME_DTYPE.fields["lag"][1]
        srow = row.copy()
        srow["n_frames"], srow["hop"], srow["offset"] = fp_in, int(rin["hop"]) * 3 // 2, int(rin["offset"]) * 3 // 2
        eng.source_track_dev(lanes, no, srow, d_fr + lag_at, vs.PITCH_FRAME_DTYPE.itemsize, fp_in, d_flow, no, d_sst,
                             cycles_ptr=d_cyc, cycles_pitch=cp)
        eng.psola_ts_dev(d_x, ns, n, ns, d_mk, mp, d_rec, d_cyc, 32, d_cyc + 4, 32, d_sst + 4, 24, cp, d_an, d_w, 2,
                         out.first(no + 3, 2), no + 3, no, d_stat, d_sy, sp, segs_ptr=d_sg, seg_pitch=sgp,
                         pmin=int(row["pmin"]), pmax=int(row["pmax"]))
        eng.synchronize()
        y = out.rows_back(no + 3, 2).copy()
        stat = dev.get(d_stat, (n,), vs.PSOLA_STAT_DTYPE)
        sy = dev.get(d_sy, (n, sp), vs.PSOLA_MARK_DTYPE)
    # the chain of restatements
    _, mk, rec, sg, frames = gr.track_and_guided(x, fs, marks=mp, segs=sgp)
    lags = np.ascontiguousarray(frames["lag"][:, :fp_in])
    _, wsst, _, logs = sr.source_track(lanes, no, [srow] * n, lags)
    start, T = np.zeros((n, cp), np.int32), np.zeros((n, cp), np.int32)
    for i, log in enumerate(logs):
        k = min(len(log), cp)
        start[i, :k], T[i, :k] = log["start"][:k], log["T"][:k]
    want = pt.psola_ts(x, [ns] * n, no, [no] * n, mk, rec, sg, start, T, None, wsst["n_cycles"], an, w, int(row["pmin"]),
                       int(row["pmax"]), 80, sp, out=np.full((n, no), gs.SENTINEL, np.int16),
                       synth=sentinel_records((n, sp), pt.MARK_DTYPE))
    same((y, stat, sy), want)
    wst = want[1]
    assert (wst["n_governed"][:3] > 10).all() and wst["status"][3] == pt.NO_RUN and (y[3] == 0).all()
    assert (wst["status"][:3] == 0).all() and (wsst["n_cycles"][:3] >= 15).all()


def test_refusals(eng):
    x = np.zeros((1, 500), np.int16)
    mk = np.array([[100, 200, 300]], np.int32)
    rec = np.zeros(1, vs.GUIDED_REC_DTYPE)
    one = np.array([[100]], np.int32)
    an, w = vs.psola_two_anchors([500], [700])

    def rc(**kw):
        a = dict(lengths=None, synth=8, pmin=32, pmax=320, out_samples=700)
        a.update(kw)
        with pytest.raises(vs.VsError) as e:
            eng.psola_ts(x, 16000, mk, rec, one, one, an, w, **a)
        return e.value.code
    R, A = vs._ffi.VS_ERR_RANGE, vs._ffi.VS_ERR_ARG
    assert rc(pmin=1) == R and rc(pmax=2049) == R and rc(lengths=501) == R and rc(out_lengths=701) == R
    assert rc(out_lengths=-1) == R and rc(unvoiced_period=1) == R and rc(unvoiced_period=1366) == R
    assert rc(synth=1) == A
    with eng.scope() as dev:
        p, q = dev.room(4096), dev.room(4096)
        for bad in (dict(start_stride=2), dict(out_pitch=699), dict(synth_pitch=1), dict(map_pitch=1), dict(out=p),
                    dict(out=p + 998), dict(segs_ptr=p, seg_pitch=0)):
            a = dict(start_stride=4, out_pitch=700, synth_pitch=8, map_pitch=2, out=q)
            a.update(bad)
            with pytest.raises(vs.VsError) as e:
                eng.psola_ts_dev(p, 500, 1, 500, p, 3, p, p, a["start_stride"], p, 4, p, 4, 1, p, p, a["map_pitch"], a["out"],
                                 a["out_pitch"], 700, p, p, a["synth_pitch"], segs_ptr=a.get("segs_ptr"),
                                 seg_pitch=a.get("seg_pitch", 0))
            assert e.value.code == A, bad


# ---- the program ----

def test_the_program(eng, tmp_path):
    """-d 1: the bytes and the line of a call without -d; -d 2 and -d 0.5 -x 1.25: the restatement chain (track, guided
    marks, periods put into output time, staircase over the output, PSOLA with the two-anchor map) and a header of the
    output's length; the refusals"""
    fs = 16000
    x = np.concatenate([ps.gaps()[:7380 + 2000], ps.glide()[0][:5000]])
    N = len(x)
    base._wav(str(tmp_path / "in.wav"), fs, x)
    for k, opts in enumerate((["-x", "1.25"], ["-j", "2", "-S", "5"])):
        plain = base._vpsola(tmp_path, "-i", "in.wav", "-o", "a%d.wav" % k, *opts)
        one = base._vpsola(tmp_path, "-i", "in.wav", "-o", "b%d.wav" % k, "-d", "1", "-u", "3", *opts)
        assert plain.returncode == 0 and one.returncode == 0, (plain.stderr, one.stderr)
        assert open(tmp_path / ("a%d.wav" % k), "rb").read() == open(tmp_path / ("b%d.wav" % k), "rb").read()
        assert plain.stdout.split()[1:] == one.stdout.split()[1:] and int(plain.stdout.split()[4]) > 50
    row = vs.strack_row_from_pitch(fs, N)
    tmin, tmax, F, hop, offset = (int(row[k]) for k in ("pmin", "pmax", "n_frames", "hop", "offset"))
    mp, sgp = N // tmin + 2, F
    _, mk, rec, sg, frames = gr.track_and_guided(x[None], fs, marks=mp, segs=sgp)
    lags = frames["lag"][0, :F].astype(np.int64)
    voiced = (lags >= tmin) & (lags <= tmax)
    base_f0 = gr.track_and_guided(x[None], fs)[0]["f0_hz"][0]
    for name, args, num, den, xf in (("long.wav", ["-d", "2"], 2, 1, None), ("short.wav", ["-d", "0.5", "-x", "1.25"], 1, 2, 1.25)):
        r = base._vpsola(tmp_path, "-i", "in.wav", "-o", name, *args)
        assert r.returncode == 0, r.stderr
        No = (2 * N * num + den) // (2 * den)
        orow = vs.strack_row_from_pitch(fs, No)
        Fo, cap = int(orow["n_frames"]), max(N, No) // tmin + 2
        st_, T_, J = np.zeros((1, cap), np.int32), np.zeros((1, cap), np.int32), 0
        if xf:
            period = np.where(voiced, np.floor(lags / xf + 0.5), 0).astype(np.int64)
            g = np.minimum(int(orow["offset"]) + np.arange(Fo) * int(orow["hop"]), No - 1)
            at = g * N // No
            operiod = period[np.where(at < offset, 0, np.minimum((at - offset) // hop, F - 1))]
            start, T = pp.staircase(operiod, int(orow["hop"]), int(orow["offset"]), Fo, No, tmin, tmax, cap)
            J = len(start)
            st_[0, :J], T_[0, :J] = start, T
        an, w = vs.psola_two_anchors([N], [No])
        wy, wst, _ = pt.psola_ts(x[None], [N], No, [No], mk, rec, sg, st_, T_, None, [J], an, w, tmin, tmax, 80,
                                 No // min(tmin, 41) + 2 * sgp + 4)
        raw = open(tmp_path / name, "rb").read()
        assert len(raw) == 44 + 2 * No and int.from_bytes(raw[40:44], "little") == 2 * No
        assert int.from_bytes(raw[4:8], "little") == 36 + 2 * No and raw[8:40] == open(tmp_path / "in.wav", "rb").read()[8:40]
        assert np.array_equal(base._payload(tmp_path / name), wy[0])
        assert r.stdout.split() == [name] + [str(int(wst[f][0])) for f in ("n_runs", "n_runs_done", "n_synth", "n_governed",
                                                                           "n_clipped", "status")]
        assert wst["status"][0] == 0 and (wst["n_governed"][0] > 40) == bool(xf)
        f0 = gr.track_and_guided(wy, fs)[0]["f0_hz"][0]                      # (the file's two voices weigh in by their frames)
        assert 0.95 < f0 / base_f0 / (xf or 1.0) < 1.05
    # refusals
    for bad in (["-d", "0"], ["-d", "-2"], ["-d", "nan"], ["-d"], ["-u", "0"], ["-q", "2"]):
        assert base._vpsola(tmp_path, "-i", "in.wav", "-o", "o.wav", *bad).returncode == 1, bad
    assert base._vpsola(tmp_path, "-i", "in.wav", "-o", "o.wav", "-d", "2", "-u", "200").returncode == 1    # U = 3200
    assert base._vpsola(tmp_path, "-i", "in.wav", "-o", "o.wav", "-d", "0.00001").returncode == 2          # no output sample
