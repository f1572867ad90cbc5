"""PSOLA with a time map as include/voice_synth.h defines it ("PSOLA with a time map", steps 1-5), restated with numpy and
Python integers only: the map and its inverse, the chain of voiced and unvoiced stretches, the synthesis marks of a
stretch, the two grains of every sample, the records.  What the section takes over from "PSOLA" (the runs of a row, which
of them are usable, PR and PL, the prefix scan of the target) comes from that section's restatement, tests/psola_ref.py.
Nothing here is shared with the library; the device and this file agree byte for byte."""
import numpy as np

import psola_ref as pp

Q = pp.Q
MAX_LAG = pp.MAX_LAG
BAD_RUN, OVERFLOW, NO_RUN, BAD_MAP = pp.BAD_RUN, pp.OVERFLOW, pp.NO_RUN, 0x8
RUN_END = pp.RUN_END
UNVOICED, UNVOICED_FLIP = -3, -4     # VS_PS_UNVOICED, VS_PS_UNVOICED_FLIP: the cycle field of an unvoiced stretch's marks
U_MAX = 2 * MAX_LAG // 3

MARK_DTYPE, STAT_DTYPE = pp.MARK_DTYPE, pp.STAT_DTYPE
ANCHOR_DTYPE = np.dtype([("u", "<i4"), ("v", "<i4")])


# ---- the map

def map_of(anchors, W, length, len_out):
    """(u, v) as lists of Python integers when the row's map is valid, else None.  anchors: the row's ANCHOR_DTYPE
    records, map_pitch of them"""
    W = int(W)
    if not 2 <= W <= len(anchors):
        return None
    u = [int(anchors["u"][j]) for j in range(W)]
    v = [int(anchors["v"][j]) for j in range(W)]
    if u[0] != 0 or v[0] != 0 or u[-1] != len_out or v[-1] != length:
        return None
    if any(u[j + 1] <= u[j] for j in range(W - 1)) or any(v[j + 1] < v[j] for j in range(W - 1)):
        return None
    return u, v


def M(mp, n):
    """for 0 <= n < len_out"""
    u, v = mp
    j = max(q for q in range(len(u) - 1) if u[q] <= n)
    return v[j] + ((n - u[j]) * (v[j + 1] - v[j])) // (u[j + 1] - u[j])


def Minv(mp, p):
    """the smallest n in [0, len_out] with M(n) >= p; M(len_out) counts as reached; Minv(0) = 0, Minv(len) = len_out"""
    u, v = mp
    if p <= 0:
        return 0
    if p >= v[-1]:
        return u[-1]
    lo, hi = 0, u[-1]
    while lo < hi:                   # (M does not decrease)
        mid = (lo + hi) // 2
        if M(mp, mid) >= p:
            hi = mid
        else:
            lo = mid + 1
    return lo


def two_anchors(length, len_out, map_pitch=2):
    a = np.zeros(map_pitch, dtype=ANCHOR_DTYPE)
    a[1] = (len_out, length)
    return a


# ---- step 1: the stretches

def unvoiced_marks(g0, g1, U):
    p = [g0]
    while g1 - p[-1] > U + U // 2:
        p.append(p[-1] + U)
    return p + [g1]


def stretches(length, a, runs, U):
    """[(voiced, the stretch's marks, first)] that cover [0, length], and (status, the number of usable runs)"""
    out, status, done, prev_end, g0 = [], 0, 0, -1, 0
    for first, m in runs:
        if not pp.usable(a, first, m, length, prev_end):
            status |= BAD_RUN
            continue
        r = [int(x) for x in a[first:first + m]]
        if r[0] > g0:
            out.append((False, unvoiced_marks(g0, r[0], U), 0))
        out.append((True, r, first))
        prev_end = g0 = r[-1]
        done += 1
    if length > g0:
        out.append((False, unvoiced_marks(g0, length, U), 0))
    return out, status, done


# ---- step 2: the synthesis marks of one stretch

def stretch_marks(voiced, b, ts, te, mp, start, T, gain, J, pmin, pmax):
    """[(t, k in the stretch, cycle field, gain)]; the last one is the stretch's end (its cycle field is None)"""
    m, out = len(b), []
    t, k, prev, kprev, flip = ts, 0, -1, -1, 0
    while True:
        c = -1
        if voiced:
            if prev >= 0 and prev + 1 < J and int(start[prev + 1]) == int(start[prev]) + int(T[prev]):
                c = prev + 1
            else:
                c = pp.seek(start, J, t)
                if c >= 0 and not t < int(start[c]) + int(T[c]):
                    c = -1
            if c >= 0 and not (pmin <= int(T[c]) <= pmax and 0 <= pp.gain_of(gain, c) <= 65535):
                c = -1
        Ti = int(T[c]) if c >= 0 else pp.pr(b, k)
        g = pp.gain_of(gain, c) if c >= 0 else Q
        code = c
        if not voiced:
            flip = 1 - flip if out and k == kprev else 0
            code = UNVOICED_FLIP if flip else UNVOICED
        out.append((t, k, code, g if out else Q))
        prev, kprev = c, k
        if te - t <= Ti + Ti // 2:
            out.append((te, m - 1, None, Q))
            return out
        t += Ti
        k = k + int(np.argmin(np.abs(np.asarray(b[k:], dtype=np.int64) - M(mp, t))))


def plan_row(length, len_out, a, runs, mp, U, start, T, gain, J, pmin, pmax, synth_pitch):
    """steps 1, 2 and 5 of a row with a valid map: (records, stat without n_clipped).  A record is a dict: t, k, cycle,
    gain as they are stored; al, pr: the mark and the period of its left grain; ar, pl: of its right grain; flip"""
    chain, status, done = stretches(length, a, runs, U)
    J = max(0, int(J))
    recs, gov, end = [], 0, None
    for voiced, b, first in chain:
        ts, te = Minv(mp, b[0]), Minv(mp, b[-1])
        if te <= ts:
            continue
        sm = stretch_marks(voiced, b, ts, te, mp, start, T, gain, J, pmin, pmax)
        for i, (t, k, code, g) in enumerate(sm[:-1]):
            r = dict(t=t, k=first + k, cycle=code, gain=g, al=b[k], pr=pp.pr(b, k), ar=b[k], pl=pp.pl(b, k),
                     flip=code == UNVOICED_FLIP)
            if i == 0 and end is not None:       # the boundary: the right grain is the end of the stretch before
                r["ar"], r["pl"] = end["ar"], end["pl"]
            recs.append(r)
            gov += code is not None and code >= 0
        m = len(b)
        end = dict(t=te, k=first + m - 1, cycle=RUN_END, gain=Q, al=b[-1], pr=pp.pr(b, m - 1), ar=b[-1], pl=pp.pl(b, m - 1),
                   flip=False)
    if end is not None:
        recs.append(end)
    if done == 0:
        status |= NO_RUN
    if len(recs) > synth_pitch:
        recs, gov, status = [], 0, status | OVERFLOW
    return recs, dict(status=status, n_runs=len(runs), n_runs_done=done, n_synth=len(recs), n_governed=gov)


# ---- step 3: the samples

def ola_row(x, length, len_out, recs, y):
    xs = np.zeros(length, dtype=np.int64)
    xs[:] = x[:length]
    y[:len_out] = 0
    clipped = 0

    def rd(idx):
        ok = (idx >= 0) & (idx < length)
        v = np.zeros(len(idx), dtype=np.int64)
        v[ok] = xs[idx[ok]]
        return v

    for j in range(len(recs) - 1):
        r0, r1 = recs[j], recs[j + 1]
        t0, t1 = r0["t"], r1["t"]
        G = t1 - t0
        d = np.arange(G, dtype=np.int64)
        e = G - d
        A, B = r0["al"], r1["ar"]
        L, L2 = min(G, r0["pr"]), min(G, r1["pl"])
        wl = np.where(d < L, Q - (d * Q) // L, 0)
        wr = np.where(e < L2, ((L2 - e) * Q) // L2, 0)
        xa = rd(A - d if r0["flip"] else A + d)
        xb = rd(B + e if r1["flip"] else B - e)
        v = (xa * wl * r0["gain"] + xb * wr * r1["gain"] + (1 << 29)) >> 30
        clipped += int(((v < -32768) | (v > 32767)).sum())
        y[t0:t1] = np.clip(v, -32768, 32767)
    return clipped


def psola_ts(x, lengths, out_samples, out_lengths, marks, rec, segs, start, T, gain, count, anchors, n_anchors, pmin, pmax, U,
             synth_pitch, out=None, synth=None):
    """the whole call.  As psola_ref.psola(), and: out_samples; out_lengths [n]; anchors ANCHOR_DTYPE [n][map_pitch];
    n_anchors [n]; U the unvoiced period.  Returns (y [n][out_samples], stat, synth)."""
    assert 2 <= U <= U_MAX
    x = np.asarray(x, dtype=np.int16)
    n = x.shape[0]
    y = np.zeros((n, out_samples), dtype=np.int16) if out is None else np.array(out, dtype=np.int16)
    sy = np.zeros((n, synth_pitch), dtype=MARK_DTYPE) if synth is None else np.array(synth, dtype=MARK_DTYPE)
    stat = np.zeros(n, dtype=STAT_DTYPE)
    tp = np.asarray(start).shape[1]
    for i in range(n):
        length, len_out = int(lengths[i]), int(out_lengths[i])
        assert 0 <= len_out <= out_samples
        runs = pp.runs_of(rec["n_segments"][i], rec["n_marks"][i], None if segs is None else segs[i], marks.shape[1])
        mp = map_of(anchors[i], n_anchors[i], length, len_out)
        if mp is None:
            y[i, :len_out] = 0
            stat[i] = (BAD_MAP | NO_RUN, len(runs), 0, 0, 0, 0)
            continue
        J = min(max(0, int(count[i])), tp)
        recs, st = plan_row(length, len_out, marks[i], runs, mp, U, start[i], T[i], None if gain is None else gain[i], J,
                            pmin, pmax, synth_pitch)
        for f, v in st.items():
            stat[f][i] = v
        for j, r in enumerate(recs):
            sy[i, j] = (r["t"], r["k"], r["cycle"], r["gain"])
        stat["n_clipped"][i] = ola_row(x[i], length, len_out, recs, y[i])
    return y, stat, sy
