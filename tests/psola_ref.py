"""PSOLA as include/voice_synth.h defines it ("PSOLA", stages A-D), restated with numpy and Python integers only: the
runs of a row, which of them are usable, the synthesis marks of a usable run, the two grains of every sample, the
records.  Nothing here is shared with the library; the device and this file agree byte for byte."""
import numpy as np

Q = 32768
MAX_LAG = 2048               # VS_AC_MAX_LAG
BAD_RUN, OVERFLOW, NO_RUN = 0x1, 0x2, 0x4
RUN_END = -2                 # VS_PS_RUN_END: the cycle field of a run's last synthesis mark
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1

MARK_DTYPE = np.dtype([(n, "<i4") for n in ("t", "k", "cycle", "gain")])
STAT_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_runs", "n_runs_done", "n_synth", "n_governed", "n_clipped")])


def runs_of(n_segments, n_marks, segs, marks_pitch):
    """the runs of a row as (first, m) pairs.  segs: the row's vs_guided_seg records (any array with first_mark_index and
    n_marks, its length is seg_pitch) or None: one run of the row's n_marks marks, capped at marks_pitch"""
    if segs is None:
        return [(0, min(int(n_marks), int(marks_pitch)))]
    n = max(0, min(int(n_segments), len(segs)))
    return [(int(segs["first_mark_index"][k]), int(segs["n_marks"][k])) for k in range(n)]


def usable(a, first, m, length, prev_end):
    """a: the row's mark array (its length is marks_pitch)"""
    if m < 2 or first < 0 or first + m > len(a):
        return False
    r = [int(v) for v in a[first:first + m]]
    if r[0] < 0 or r[-1] >= length or r[0] <= prev_end:
        return False
    return all(0 < r[j + 1] - r[j] <= MAX_LAG for j in range(m - 1))


def pr(r, k):
    return r[k + 1] - r[k] if k < len(r) - 1 else r[k] - r[k - 1]


def pl(r, k):
    return r[k] - r[k - 1] if k > 0 else r[1] - r[0]


def gain_of(gain, c):
    return Q if gain is None else int(gain[c])


def seek(start, J, t):
    """the largest c with start[c''] <= t for all c'' <= c; -1 without one"""
    c = -1
    while c + 1 < J and int(start[c + 1]) <= t:
        c += 1
    return c


def synth_marks(r, start, T, gain, J, pmin, pmax):
    """stage A on one usable run (r: its marks): a list of (t, k, cycle or -1 or RUN_END, gain)"""
    m, E = len(r), r[-1]
    out = []
    t, k, prev = r[0], 0, -1
    while True:
        c = -1
        if prev >= 0 and prev + 1 < J and int(start[prev + 1]) == int(start[prev]) + int(T[prev]):
            c = prev + 1
        else:
            c = seek(start, J, t)
            if c >= 0 and not t < int(start[c]) + int(T[c]):
                c = -1
        if c >= 0 and not (pmin <= int(T[c]) <= pmax and 0 <= gain_of(gain, c) <= 65535):
            c = -1
        Ti = int(T[c]) if c >= 0 else pr(r, k)
        g = gain_of(gain, c) if c >= 0 else Q
        out.append((t, k, c, g if out else Q))
        prev = c
        if E - t <= Ti + Ti // 2:
            out.append((E, m - 1, RUN_END, Q))
            return out
        t += Ti
        k = k + int(np.argmin(np.abs(np.asarray(r[k:], dtype=np.int64) - t)))


def plan_row(length, a, runs, start, T, gain, J, pmin, pmax, synth_pitch):
    """stages A and D of one row: (records [(t, k in the row, cycle, gain)], the run [(first, m)] of every record, stat
    without n_clipped)"""
    recs, owner = [], []
    status = n_done = n_gov = 0
    prev_end = -1
    J = max(0, int(J))
    over = False
    for first, m in runs:
        if over:
            continue
        if not usable(a, first, m, length, prev_end):
            status |= BAD_RUN
            continue
        r = [int(v) for v in a[first:first + m]]
        sm = synth_marks(r, start, T, gain, J, pmin, pmax)
        if len(recs) + len(sm) > synth_pitch:
            status |= OVERFLOW
            over = True
            continue
        prev_end = r[-1]
        n_done += 1
        n_gov += sum(1 for s in sm if s[2] >= 0)
        recs += [(t, first + k, c, g) for t, k, c, g in sm]
        owner += [(first, m)] * len(sm)
    if n_done == 0:
        status |= NO_RUN
    return recs, owner, dict(status=status, n_runs=len(runs), n_runs_done=n_done, n_synth=len(recs), n_governed=n_gov)


def ola_row(x, length, a, recs, owner, y):
    """stage B: y[0..length) from x[0..length); returns n_clipped"""
    xs = np.zeros(length, dtype=np.int64)
    xs[:] = x[:length]
    y[:length] = x[:length]
    clipped = 0

    def rd(idx):
        ok = (idx >= 0) & (idx < length)
        v = np.zeros(len(idx), dtype=np.int64)
        v[ok] = xs[idx[ok]]
        return v

    for j in range(len(recs) - 1):
        t0, k0, c0, g0 = recs[j]
        t1, k1, _, g1 = recs[j + 1]
        if c0 == RUN_END:
            continue
        first, m = owner[j]
        r = [int(v) for v in a[first:first + m]]
        G = t1 - t0
        d = np.arange(G, dtype=np.int64)
        e = G - d
        A, B = r[k0 - first], r[k1 - first]
        L, L2 = min(G, pr(r, k0 - first)), min(G, pl(r, k1 - first))
        wl = np.where(d < L, Q - (d * Q) // L, 0)
        wr = np.where(e < L2, ((L2 - e) * Q) // L2, 0)
        v = (rd(A + d) * wl * g0 + rd(B - e) * wr * g1 + (1 << 29)) >> 30
        clipped += int(((v < -32768) | (v > 32767)).sum())
        y[t0:t1] = np.clip(v, -32768, 32767)
    return clipped


def psola(x, lengths, marks, rec, segs, start, T, gain, count, pmin, pmax, synth_pitch, out=None, synth=None):
    """the whole call.  x int16 [n][ns]; lengths [n]; marks int32 [n][marks_pitch]; rec: records with n_segments and
    n_marks; segs: records [n][seg_pitch] or None; start, T, gain (or None) int32 [n][target_pitch]; count [n].
    out and synth: what the outputs hold before the call (default: zeros).  Returns (y, stat, synth)."""
    x = np.asarray(x, dtype=np.int16)
    n, ns = x.shape
    y = np.zeros((n, ns), dtype=np.int16) if out is None else np.array(out, dtype=np.int16)
    sy = np.zeros((n, synth_pitch), dtype=MARK_DTYPE) if synth is None else np.array(synth, dtype=MARK_DTYPE)
    stat = np.zeros(n, dtype=STAT_DTYPE)
    tp = np.asarray(start).shape[1]
    for i in range(n):
        length = int(lengths[i])
        J = min(max(0, int(count[i])), tp)
        runs = runs_of(rec["n_segments"][i], rec["n_marks"][i], None if segs is None else segs[i], marks.shape[1])
        recs, owner, st = plan_row(length, marks[i], runs, start[i], T[i], None if gain is None else gain[i], J, pmin, pmax,
                                   synth_pitch)
        for f, v in st.items():
            stat[f][i] = v
        for j, rcd in enumerate(recs):
            sy[i, j] = rcd
        stat["n_clipped"][i] = ola_row(x[i], length, marks[i], recs, owner, y[i])
    return y, stat, sy


def staircase(period, hop, offset, n_frames, length, pmin, pmax, cap):
    """the target of a period track without jitter: the walk of the source track (include/voice_synth.h, "source track",
    stages 1 and 2) with T = P -- cycles where the frame of g is voiced, a jump to the next voiced frame where it is
    not.  Returns (start, T) of at most cap cycles."""
    def frame(g):
        return 0 if g < offset else min((g - offset) // hop, n_frames - 1)

    def voiced(f):
        return pmin <= int(period[f]) <= pmax
    start, T = [], []
    g = 0
    while g < length and len(start) < cap:
        f = frame(g)
        if voiced(f):
            start.append(g)
            T.append(int(period[f]))
            g += int(period[f])
        else:
            f2 = next((q for q in range(f + 1, n_frames) if voiced(q)), None)
            g = length if f2 is None else min(length, offset + f2 * hop)
    return np.array(start, dtype=np.int32), np.array(T, dtype=np.int32)
