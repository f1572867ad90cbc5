"""numpy restatement of the guided marks defined in include/voice_synth.h ("guided marks").

Test infrastructure only: the product never imports it.  Written from the header, one function per step (A voiced, B
runs, C samples, D the walk, E the summary); everything that places a mark is an integer, so the integer fields, marks,
counts and segment records of the device must equal these bit for bit, and the doubles (but for the two that go through
log10) must be equal as well.
"""
import math

import numpy as np

import acoustic_ref as ar
import pitch_ref as pr

MG_ALL = 0
MG_LONGEST = 1
MG_MAX_EDGE = 16

REC_DTYPE = np.dtype([(n, "<i4") for n in ("n_segments", "n_marks", "n_frames_walked", "reserved_")])
SEG_DTYPE = np.dtype([(n, "<i4") for n in ("first_frame", "n_frames", "first_mark_index", "n_marks")])

DEFAULTS = dict(f0_min=50.0, f0_max=500.0, polarity=1, segments=MG_ALL, edge_frames=1, min_frames=3, hop_s=0.010)
NAN = float("nan")


def opts(**kw):
    """the options as a dict; ValueError where the library refuses them"""
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError(k)
        o[k] = v
    if o["polarity"] not in (1, -1) or o["segments"] not in (MG_ALL, MG_LONGEST):
        raise ValueError("polarity / segments")
    if not (math.isfinite(o["hop_s"]) and o["hop_s"] >= 0):
        raise ValueError("hop_s")
    if not 0 <= int(o["edge_frames"]) <= MG_MAX_EDGE or int(o["min_frames"]) < 1:
        raise ValueError("edge_frames / min_frames")
    return o


def plan(fs, length, o):
    """(tmin, tmax, H, n_frames, C) of a row"""
    tmin, tmax = ar.lag_bounds(fs, o["f0_min"], o["f0_max"])
    H = pr.hop(fs, o["hop_s"])
    return tmin, tmax, H, pr.frame_count(length, tmax, H), tmax + tmax // 2


def voiced(lags, tmin, tmax):
    """A: tmin <= lag <= tmax, and nothing else"""
    lags = np.asarray(lags, dtype=np.int64)
    return (lags >= tmin) & (lags <= tmax)


def runs(v, edge_frames, min_frames, segments):
    """B: the walked runs [(fa, fb)] in order"""
    F = len(v)
    out = []
    f = 0
    while f < F:
        if not v[f]:
            f += 1
            continue
        fa = f
        while f + 1 < F and v[f + 1]:
            f += 1
        fb = f
        f += 1
        if fa > 0:
            fa += edge_frames
        if fb < F - 1:
            fb -= edge_frames
        if fb - fa + 1 >= min_frames:
            out.append((fa, fb))
    if segments == MG_LONGEST and out:
        best = out[0]
        for r in out[1:]:
            if r[1] - r[0] > best[1] - best[0]:   # ties to the first
                best = r
        out = [best]
    return out


def frame_of(n, C, H, n_frames):
    """C: f(n)"""
    return 0 if n <= C else min(n_frames - 1, (n - C + H // 2) // H)


def run_samples(fa, fb, C, H, n_frames, length):
    """C: [a, b) of the run [fa, fb]"""
    a = 0 if fa == 0 else C + fa * H - H // 2
    b = length if fb == n_frames - 1 else min(length, C + (fb + 1) * H - H // 2)
    return a, b


def walk_run(y, lags, a, b, tmin, tmax, C, H, n_frames, fa, events=None):
    """D: the marks and amplitudes of one run (y int64); events (a list) receives "empty" for every empty window and
    "again" for every window that begins at or before the end of the window before it (the device walks that stretch a
    second time)"""
    m = [a + int(np.argmax(y[a:min(a + int(lags[fa]), b)]))]
    amps = []
    T = None
    seen = min(a + int(lags[fa]), b) - 1          # the last sample looked at
    while True:
        P = int(lags[frame_of(m[-1], C, H, n_frames)])
        lo1, hi1, d = max(tmin, (2 * P + 2) // 3), min(tmax, (3 * P) // 2), (P + 3) // 4
        lo, hi = lo1, hi1
        if T is not None:
            lo2, hi2 = max(lo1, T - d), min(hi1, T + d)
            if lo2 <= hi2:
                lo, hi = lo2, hi2
            elif events is not None:
                events.append("empty")
        if m[-1] + hi >= b:
            return m, amps
        w0, w1 = m[-1] + lo, m[-1] + hi
        if events is not None and w0 <= seen:
            events.append("again")
        seen = w1
        k = w0 + int(np.argmax(y[w0:w1 + 1]))
        amps.append(int(y[k]) - int(y[m[-1]:k].min()))
        T = k - m[-1]
        m.append(k)


def summary(fs, per_run):
    """E but for hnr_db: the vs_acoustic fields of [(marks, amps)] per run, as a dict; K, N2, N3, N5 are included"""
    rec = {f: NAN for f in ar.FIELDS}
    Ts = [[m[i + 1] - m[i] for i in range(len(m) - 1)] for m, _ in per_run]
    As = [list(a) for _, a in per_run]
    K = sum(len(t) for t in Ts)
    N2 = sum(max(0, len(t) - 1) for t in Ts)
    N3 = sum(max(0, len(t) - 2) for t in Ts)
    N5 = sum(max(0, len(t) - 4) for t in Ts)
    rec.update(n_periods=K, N2=N2, N3=N3, N5=N5, status=(ar.AC_FEW_PERIODS if K < 2 else 0))

    def sums(seqs):
        s2 = sum(abs(v[i + 1] - v[i]) for v in seqs for i in range(len(v) - 1))
        s3 = sum(abs(3 * v[i] - (v[i - 1] + v[i] + v[i + 1])) for v in seqs for i in range(1, len(v) - 1))
        s5 = sum(abs(5 * v[i] - sum(v[i - 2:i + 3])) for v in seqs for i in range(2, len(v) - 2))
        return s2, s3, s5

    if K >= 1:
        Tm = float(sum(sum(t) for t in Ts)) / float(K)
        rec["f0_hz"] = float(fs) / Tm
        s2, s3, s5 = sums(Ts)
        if N2:
            rec["jitter_local"] = (float(s2) / float(N2)) / Tm
            rec["jitter_abs_s"] = (float(s2) / float(N2)) / float(fs)
        if N3:
            rec["jitter_rap"] = (float(s3) / (3.0 * float(N3))) / Tm
        if N5:
            rec["jitter_ppq5"] = (float(s5) / (5.0 * float(N5))) / Tm
        if min(min(a) for a in As if a) <= 0:
            rec["status"] |= ar.AC_ZERO_AMPLITUDE
        else:
            Am = float(sum(sum(a) for a in As)) / float(K)
            s2, s3, s5 = sums(As)
            if N2:
                rec["shimmer_local"] = (float(s2) / float(N2)) / Am
                sdb = 0.0
                for a in As:                      # in mark order
                    for i in range(len(a) - 1):
                        sdb += abs(20.0 * math.log10(float(a[i + 1]) / float(a[i])))
                rec["shimmer_db"] = sdb / float(N2)
            if N3:
                rec["shimmer_apq3"] = (float(s3) / (3.0 * float(N3))) / Am
            if N5:
                rec["shimmer_apq5"] = (float(s5) / (5.0 * float(N5))) / Am
    return rec


def hnr(qs):
    """E: hnr_db from the q of the walked frames"""
    Q = sum(min(max(int(q), 0), 32768) for q in qs)
    rho = float(Q) / (32768.0 * float(len(qs)))
    rho = min(max(rho, 1e-10), 1.0 - 1e-10)
    return 10.0 * math.log10(rho / (1.0 - rho))


def guided_row(x, fs, frames, events=None, **kw):
    """one row: x int16 [len], frames the row's pitch records (at least n_frames of them; the fields lag and q are read).
    Returns dict(rec=the vs_acoustic fields, marks=[...] of all runs, guided=(n_segments, n_marks, n_frames_walked),
    segs=[(first_frame, n_frames, first_mark_index, n_marks)], runs=[(marks, amps)])"""
    o = opts(**kw)
    x = np.asarray(x, dtype=np.int64)
    y = x * int(o["polarity"])
    tmin, tmax, H, F, C = plan(fs, len(x), o)
    rec = {f: NAN for f in ar.FIELDS}
    rec.update(p0=0, n_periods=0, first_mark=-1, status=0)
    empty = dict(rec=rec, marks=[], guided=(0, 0, 0), segs=[], runs=[])
    if F == 0:
        rec["status"] = ar.AC_TOO_SHORT
        return empty
    lags = np.asarray(frames["lag"][:F], dtype=np.int64)
    qs = np.asarray(frames["q"][:F], dtype=np.int64)
    rr = runs(voiced(lags, tmin, tmax), int(o["edge_frames"]), int(o["min_frames"]), o["segments"])
    if not rr:
        rec["status"] = ar.AC_UNVOICED
        return empty
    per_run, segs, marks = [], [], []
    for fa, fb in rr:
        a, b = run_samples(fa, fb, C, H, F, len(x))
        m, amps = walk_run(y, lags, a, b, tmin, tmax, C, H, F, fa, events)
        segs.append((fa, fb - fa + 1, len(marks), len(m)))
        marks += m
        per_run.append((m, amps))
    s = summary(fs, per_run)
    for k in rec:
        if k in s:
            rec[k] = s[k]
    nF = sum(fb - fa + 1 for fa, fb in rr)
    rec["hnr_db"] = hnr([qs[f] for fa, fb in rr for f in range(fa, fb + 1)])
    rec["first_mark"] = marks[0]
    rec["p0"] = int(lags[frame_of(marks[0], C, H, F)])
    return dict(rec=rec, marks=marks, guided=(len(rr), len(marks), nF), segs=segs, runs=per_run)


def guided(pcm, fs, frames, lengths=None, marks=0, segs=0, marks_fill=None, segs_fill=None, **kw):
    """rows of pcm (int16 [n][samples]); fs scalar or per row; frames [n][frames_pitch] pitch records.  Returns (records
    ar.DTYPE [n], marks int32 [n][marks] or None (-1, or marks_fill, where nothing is written), rec REC_DTYPE [n], segs
    SEG_DTYPE [n][segs] or None (zero, or segs_fill, where nothing is written))"""
    pcm = np.asarray(pcm)
    n = pcm.shape[0]
    fs = np.broadcast_to(np.asarray(fs, dtype=np.int64), (n,))
    out = np.zeros(n, dtype=ar.DTYPE)
    grec = np.zeros(n, dtype=REC_DTYPE)
    mk = None
    if marks:
        mk = np.full((n, marks), -1, dtype=np.int32) if marks_fill is None else np.array(marks_fill, np.int32).reshape(n, marks)
    sg = None
    if segs:
        sg = np.zeros((n, segs), SEG_DTYPE) if segs_fill is None else np.array(segs_fill, SEG_DTYPE).reshape(n, segs)
    for i in range(n):
        L = pcm.shape[1] if lengths is None else int(lengths[i])
        r = guided_row(pcm[i, :L], int(fs[i]), frames[i], **kw)
        for k, v in r["rec"].items():
            out[i][k] = v
        grec[i] = r["guided"] + (0,)
        if marks:
            m = r["marks"][:marks]
            mk[i, :len(m)] = m
        if segs:
            for k, s in enumerate(r["segs"][:segs]):
                sg[i, k] = s
    return out, mk, grec, sg


def track_and_guided(pcm, fs, lengths=None, pitch=None, **kw):
    """what vs_guided computes: pitch_ref's track with the guided options' f0_min, f0_max and hop_s, then guided()"""
    o = opts(**{k: v for k, v in kw.items() if k in DEFAULTS})
    pk = dict(pitch or {}, f0_min=o["f0_min"], f0_max=o["f0_max"], hop_s=o["hop_s"])
    frames, nfr = pr.track(pcm, fs, lengths, **pk)
    return guided(pcm, fs, frames, lengths, **kw) + (frames,)


COLUMNS = ar.COLUMNS + ("segments", "voiced_frames")


def format_line(name, rec, grec):
    """one line of `acoustic -T`: the line of `acoustic` and behind it n_segments and n_frames_walked"""
    return "%s %d %d" % (ar.format_line(name, rec), int(grec["n_segments"]), int(grec["n_frames_walked"]))


# ---- the chains that take guided marks where they took vs_measure's (VS_MG_LONGEST: one contiguous train) ----

def measure_longest(pcm, fs, f0_min=50.0, f0_max=500.0, polarity=1, marks_pitch=None, lengths=None):
    """pitch_ref's track at its defaults but the range, then guided() with VS_MG_LONGEST: (meas, marks, rec, frames)"""
    pcm = np.asarray(pcm)
    mp = pcm.shape[1] // 2 + 2 if marks_pitch is None else marks_pitch
    out, mk, rec, _, frames = track_and_guided(pcm, fs, lengths, marks=mp, f0_min=f0_min, f0_max=f0_max, polarity=polarity,
                                               segments=MG_LONGEST)
    return out, mk, rec, frames


def measure_and_glottal(pcm, fs, level_open=26, level_mid=128, polarity=1, f0_min=50.0, f0_max=500.0, cycles_pitch=0):
    """glottal_ref.measure_and_glottal with guided marks: (meas, marks, records[, cycles], frames last)"""
    import glottal_ref as gl
    meas, mk, _, frames = measure_longest(pcm, fs, f0_min, f0_max, polarity)
    res = gl.glottal(pcm, meas, mk, level_open, level_mid, polarity, cycles_pitch)
    return (meas, mk) + (tuple(res) if cycles_pitch else (res,)) + (frames,)


def closed_phase(pcm, fs, de_emphasis=0.0, scale=1.0, f0_min=50.0, f0_max=500.0, polarity=1, first_de_emphasis=0.99,
                 level_open=26, level_mid=128, **kw):
    """cplpc_ref.closed_phase (one set per row: window_s == 0) with guided marks in the first pass.  Returns its dict and
    frames, the residual's pitch track"""
    import cplpc_ref as cp
    import iaif_ref as ia
    import inverse_ref as ir
    import lpc_ref as lr
    pcm = np.asarray(pcm, dtype=np.int16)
    n, ns = pcm.shape
    p = cp.opts(**kw)["order"]
    ikw = dict(glottal_order=min(4, p), order=p)
    sets1 = ia.analyse(pcm, fs, **ikw)
    L, H, starts = lr.frame_plan(int(fs), ns, ia.lpc_opts(ia.opts(**ikw)))
    n_sets, hop, offset, _ = ir.from_lpc(L, H, 0, len(starts), ns, ir.HOLD)[:4]
    residual, inv_stat = ir.inverse_filter(pcm, sets1["coefs"], ir.rows_of(n, n_sets, hop, offset, ns, scale,
                                                                           first_de_emphasis), ir.HOLD)
    mp = ns // 2 + 2
    meas, mk, rec, cyc, frames = measure_and_glottal(residual, fs, level_open, level_mid, polarity, f0_min, f0_max, mp)
    sets = cp.analyse(pcm, fs, rec, cyc, **kw)
    assert cp.opts(**kw)["window_s"] == 0
    flow, stat = ir.inverse_filter(pcm, sets["coefs"], ir.rows_of(n, 1, 1, 0, ns, scale, de_emphasis), ir.HOLD)
    return dict(residual=residual, inv_stat=inv_stat, meas=meas, marks=mk, glottal=rec, cycles=cyc, iaif=sets1, flow=flow,
                flow_stat=stat, sets=sets, frames=frames)
