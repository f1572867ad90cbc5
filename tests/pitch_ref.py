"""numpy restatement of the pitch track defined in include/voice_synth.h ("pitch track").

Test infrastructure only: the product never imports it.  Written from the header, step by step; every quantity is an
integer, so the device's records must equal these byte for byte.
"""
import math

import numpy as np

import acoustic_ref as ar

PT_MAX_CAND = 7
PT_SILENT = 0x1
PT_UNVOICED = 0x2
PT_NO_CANDIDATE = 0x4
PT_MAX_COST = 1 << 20

FRAME_DTYPE = np.dtype([("r0", "<i8"), ("start", "<i4"), ("lag", "<i4"), ("q", "<i4"), ("status", "<i4"),
                        ("n_cand", "<i4"), ("reserved_", "<i4"), ("cand_lag", "<i4", (PT_MAX_CAND,)),
                        ("cand_q", "<i4", (PT_MAX_CAND,)), ("back", "u1", (PT_MAX_CAND + 1,))])
assert FRAME_DTYPE.itemsize == 96

DEFAULTS = dict(f0_min=50.0, f0_max=500.0, voicing_q=14746, octave_q=328, jump_q=11469, vuv_q=4588, silence_rms=16,
                hop_s=0.010)


def opts(**kw):
    """the options as a dict; ValueError where the library answers VS_ERR_ARG"""
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise TypeError(k)
        o[k] = v
    for k in ("voicing_q", "octave_q", "jump_q", "vuv_q"):
        if not 0 <= int(o[k]) <= PT_MAX_COST:
            raise ValueError(k)
    if not 0 <= int(o["silence_rms"]) <= 32767 or not (math.isfinite(o["hop_s"]) and o["hop_s"] >= 0):
        raise ValueError("silence_rms / hop_s")
    return o


def log2_table(n=ar.AC_MAX_LAG + 1):
    """Lg[0..n): 0, then floor(256*log2(t) + 0.5)"""
    t = np.arange(1, n, dtype=np.float64)
    return np.concatenate([[0], np.floor(256.0 * np.log2(t) + 0.5)]).astype(np.int32)[:n]


def log2_margin(n=ar.AC_MAX_LAG + 1):
    """the smallest distance of 256*log2(t), t in [1, n), to a rounding tie (a half-integer)"""
    v = 256.0 * np.log2(np.arange(1, n, dtype=np.float64))
    return float(np.abs(v - np.floor(v) - 0.5).min())


def hop(fs, hop_s):
    H = math.floor(float(hop_s) * float(fs) + 0.5)
    if H < 1 or H > 0x7FFFFFFF:
        raise ValueError("hop of %r samples" % H)   # (the library: VS_ERR_RANGE)
    return int(H)


def frame_count(length, tmax, H):
    return 1 + (length - (3 * tmax + 2)) // H if length >= 3 * tmax + 2 else 0


def frame_q(y, s, tmin, tmax):
    """(r0, q) of the frame at s: q[t - (tmin - 1)] for t in [tmin - 1, tmax + 1] (y int64)"""
    W = 2 * tmax
    tlo = tmin - 1
    a = y[s:s + W]
    seg = y[s:s + W + tmax + 1]                                   # the frame reads y[s .. s + W + tmax]
    r = np.correlate(seg[tlo:], a, "valid")[:tmax + 3 - tmin]     # r[i] = sum_k a[k] * seg[tlo + i + k]
    c = np.concatenate([[0], np.cumsum(seg * seg)])
    t = np.arange(tlo, tmax + 2)
    e = c[t + W] - c[t]
    r0 = int(c[W])
    den = r0 + e
    ok = (r > 0) & (den > 0)
    q = np.where(ok, (np.where(ok, r, 0) << 16) // np.where(ok, den, 1), 0)
    return r0, q.astype(np.int64)


def frame_candidates(y, s, tmin, tmax, silence_rms):
    """(r0, status bits, [(t, q)] in ascending t) of one frame"""
    W = 2 * tmax
    r0, q = frame_q(y, s, tmin, tmax)
    if r0 < W * int(silence_rms) ** 2:
        return r0, PT_SILENT, []
    i = np.arange(1, len(q) - 1)
    loc = i[(q[i] > 0) & (q[i] > q[i - 1]) & (q[i] >= q[i + 1])]
    best = sorted(((-int(q[k]), int(k) + tmin - 1) for k in loc))[:PT_MAX_CAND]
    cands = sorted((t, -nq) for nq, t in best)
    return r0, (0 if cands else PT_NO_CANDIDATE), cands


def greedy(cands):
    """the lag of the best candidate of a frame by (q descending, t ascending); 0 without one"""
    return min(cands, key=lambda c: (-c[1], c[0]))[0] if cands else 0


def viterbi(frames, tmax, o, lg):
    """frames: [[(t, q)] per frame].  Returns (states, back): the chosen state and the back[8] of every frame"""
    F = len(frames)
    back = np.zeros((F, PT_MAX_CAND + 1), dtype=np.uint8)
    if F == 0:
        return [], back

    def local(c):
        return [int(o["voicing_q"])] + [q + ((int(o["octave_q"]) * int(lg[tmax] - lg[t])) >> 8) for t, q in c]

    def trans(ti, tj):
        if ti == 0 and tj == 0:
            return 0
        if ti == 0 or tj == 0:
            return int(o["vuv_q"])
        return (int(o["jump_q"]) * abs(int(lg[ti]) - int(lg[tj]))) >> 8

    delta = local(frames[0])
    for f in range(1, F):
        lp, lc = [0] + [t for t, _ in frames[f - 1]], [0] + [t for t, _ in frames[f]]
        D = local(frames[f])
        nd = []
        for j, tj in enumerate(lc):
            v = [delta[i] - trans(ti, tj) for i, ti in enumerate(lp)]
            bi = v.index(max(v))              # ties to the smallest i
            back[f, j] = bi
            nd.append(D[j] + v[bi])
        delta = nd
    states = [0] * F
    states[F - 1] = delta.index(max(delta))  # ties to the smallest j
    for f in range(F - 1, 0, -1):
        states[f - 1] = int(back[f, states[f]])
    return states, back


def track_row(x, fs, **kw):
    """the records (FRAME_DTYPE [n_frames]) of one row"""
    o = opts(**kw)
    tmin, tmax = ar.lag_bounds(fs, o["f0_min"], o["f0_max"])
    H = hop(fs, o["hop_s"])
    y = np.asarray(x, dtype=np.int64)
    F = frame_count(len(y), tmax, H)
    rec = np.zeros(F, dtype=FRAME_DTYPE)
    lg = log2_table()
    frames = []
    for f in range(F):
        r0, st, cands = frame_candidates(y, f * H, tmin, tmax, o["silence_rms"])
        rec[f]["r0"], rec[f]["start"], rec[f]["status"], rec[f]["n_cand"] = r0, f * H, st, len(cands)
        for k, (t, q) in enumerate(cands):
            rec[f]["cand_lag"][k], rec[f]["cand_q"][k] = t, q
        frames.append(cands)
    states, back = viterbi(frames, tmax, o, lg)
    for f, s in enumerate(states):
        rec[f]["back"] = back[f]
        if s == 0:
            rec[f]["lag"], rec[f]["q"] = 0, int(o["voicing_q"])
            rec[f]["status"] |= PT_UNVOICED
        else:
            rec[f]["lag"], rec[f]["q"] = frames[f][s - 1]
    return rec


def track(pcm, fs, lengths=None, frames_pitch=None, fill=None, **kw):
    """rows of pcm (int16 [n][samples]); fs scalar or per row.  Returns (records [n][frames_pitch], n_frames [n]); the
    records past a row's frames are those of `fill` ([n][frames_pitch]) or zero"""
    pcm = np.asarray(pcm)
    n = pcm.shape[0]
    fs = np.broadcast_to(np.asarray(fs, dtype=np.int64), (n,))
    rows = [track_row(pcm[i, :pcm.shape[1] if lengths is None else int(lengths[i])], int(fs[i]), **kw) for i in range(n)]
    nfr = np.array([len(r) for r in rows], dtype=np.int32)
    fp = max(1, int(nfr.max())) if frames_pitch is None else int(frames_pitch)
    out = np.zeros((n, fp), dtype=FRAME_DTYPE) if fill is None else np.array(fill, dtype=FRAME_DTYPE).reshape(n, fp).copy()
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, nfr


COLUMNS = ("file", "frames", "voiced", "segments", "F0_mean_Hz", "F0_min_Hz", "F0_max_Hz", "status")


def summary(rec, fs):
    """what `pitch` prints of a row's records: frames, voiced, segments (maximal runs of voiced frames), mean / min / max
    of fs / lag over the voiced frames (NaN without one), status = the OR of the frames' bits"""
    lag = rec["lag"].astype(np.int64)
    v = lag > 0
    seg = int(np.count_nonzero(v[1:] & ~v[:-1]) + (1 if len(v) and v[0] else 0))
    f0 = float(fs) / lag[v].astype(np.float64)
    acc = 0.0
    for v1 in f0.tolist():                     # summed in order of the frames
        acc += v1
    mean = acc / len(f0) if len(f0) else float("nan")
    st = 0
    for s in rec["status"].tolist():
        st |= int(s)
    return dict(frames=len(rec), voiced=int(v.sum()), segments=seg, f0_mean=mean, f0_min=float(f0.min()) if len(f0) else
                float("nan"), f0_max=float(f0.max()) if len(f0) else float("nan"), status=st)


def format_line(name, rec, fs):
    s = summary(rec, fs)

    def g(v):
        return "nan" if math.isnan(v) else "%.3f" % v
    return "%s %d %d %d %s %s %s %d" % (name, s["frames"], s["voiced"], s["segments"], g(s["f0_mean"]), g(s["f0_min"]),
                                        g(s["f0_max"]), s["status"])


def format_frame(name, r):
    """one line of `pitch -l`"""
    head = "# frame %s: %d %d %d %d %d" % (name, int(r["start"]), int(r["lag"]), int(r["q"]), int(r["status"]),
                                          int(r["n_cand"]))
    return head + "".join(" %d:%d" % (int(t), int(q)) for t, q in zip(r["cand_lag"][:r["n_cand"]], r["cand_q"][:r["n_cand"]]))
