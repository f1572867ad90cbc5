"""numpy restatement of the glottal parameters defined in include/voice_synth.h ("Glottal parameters").

Test infrastructure only: the product never imports it.  Every step follows the header's text in the same order: the
cycle records are integers, every quotient is one IEEE division of two exactly representable doubles and the row means
are summed in the order of the cycles, so the device must equal all of it bit for bit.
"""
import math

import numpy as np

import acoustic_ref as ar

GL_NO_CYCLES = 0x1
GL_BAD_MARKS = 0x2
GL_REJECTED = 0x4
GL_ALL_REJECTED = 0x8
GLC_ZERO_AMPLITUDE = 0x1
GLC_NO_CLOSURE = 0x2

NAN = float("nan")

FIELDS = ("oq", "clq", "sq", "qoq", "naq")
OPTS_DTYPE = np.dtype([("level_open", "<i4"), ("level_mid", "<i4"), ("polarity", "<i4"), ("reserved_", "<i4")])
REC_DTYPE = np.dtype([(f, "<f8") for f in FIELDS] + [("n_cycles", "<i4"), ("n_rejected", "<i4"), ("status", "<i4"),
                                                      ("reserved_", "<i4")])
CYCLE_FIELDS = ("peak", "period", "trough", "amp", "open", "close", "open_mid", "close_mid", "gci", "decl", "status",
                "reserved_")
CYCLE_DTYPE = np.dtype([(f, "<i4") for f in CYCLE_FIELDS])


def check_levels(level_open, level_mid, polarity):
    """ValueError where the library returns an error"""
    if not (0 <= level_open <= 255 and level_open <= level_mid <= 255):
        raise ValueError("levels %d, %d out of range" % (level_open, level_mid))
    if polarity not in (1, -1):
        raise ValueError("polarity %d" % polarity)


def _empty(status):
    rec = {f: NAN for f in FIELDS}
    rec.update(n_cycles=0, n_rejected=0, status=status, reserved_=0)
    return rec


def _crossings(y, lo, mc, mn, b, a, q):
    """(open_q, close_q) of one cycle; close_q None when nothing in (mc, mn) is not above q"""
    below = 256 * (y[lo:mc] - b) <= q * a           # lo never is above: the list is not empty
    opn = lo + int(np.flatnonzero(below)[-1]) + 1
    after = np.flatnonzero(256 * (y[mc + 1:mn] - b) <= q * a)
    return opn, (mc + 1 + int(after[0]) if len(after) else None)


def cycle(y, mp, mc, mn, level_open, level_mid):
    """the cycle record (a dict of python ints) of the peak mc between the marks mp and mn; y int64"""
    lo = mp + int(np.argmin(y[mp:mc]))
    b = int(y[lo])
    a = int(y[mc]) - b
    c = dict(peak=mc, period=mn - mc, trough=lo, amp=a, open=-1, close=-1, open_mid=-1, close_mid=-1, gci=-1, decl=0,
             status=0, reserved_=0)
    if a <= 0:
        c["status"] = GLC_ZERO_AMPLITUDE
        return c
    open_o, close_o = _crossings(y, lo, mc, mn, b, a, level_open)
    if close_o is None:
        c["status"] = GLC_NO_CLOSURE
        return c
    open_h, close_h = _crossings(y, lo, mc, mn, b, a, level_mid)
    diff = y[mc:close_o] - y[mc + 1:close_o + 1]
    c.update(open=open_o, close=close_o, open_mid=open_h, close_mid=close_h, gci=mc + int(np.argmax(diff)) + 1,
             decl=int(diff.max()))
    return c


def quotients(c):
    """(OQ, ClQ, SQ, QOQ, NAQ) of an accepted cycle record"""
    T = float(c["period"])
    return (float(c["close"] - c["open"]) / T, float(c["close"] - c["peak"]) / T,
            float(c["peak"] - c["open"]) / float(c["close"] - c["peak"]), float(c["close_mid"] - c["open_mid"]) / T,
            float(c["amp"]) / (float(c["decl"]) * T))


def glottal_row(x, n_periods, ac_status, marks, level_open=26, level_mid=128, polarity=1):
    """(record as a dict, list of all the cycle records) of one row: x int16 [n_samples], the measurement's n_periods and
    status, marks = the row of the marks array (its length is marks_pitch)"""
    check_levels(level_open, level_mid, polarity)
    n = len(x)
    K = int(n_periods)
    marks_pitch = len(marks)
    if int(ac_status) & (ar.AC_TOO_SHORT | ar.AC_UNVOICED):
        return _empty(GL_NO_CYCLES), []
    if K < 0:
        return _empty(GL_BAD_MARKS), []
    M = min(K + 1, marks_pitch)
    if M < 3:
        return _empty(GL_NO_CYCLES), []
    m = [int(v) for v in marks[:M]]
    if m[0] < 0 or m[-1] >= n or any(m[j] >= m[j + 1] for j in range(M - 1)):
        return _empty(GL_BAD_MARKS), []
    y = np.asarray(x, dtype=np.int64) * int(polarity)
    cycles = [cycle(y, m[c - 1], m[c], m[c + 1], level_open, level_mid) for c in range(1, M - 1)]
    s = [0.0] * 5
    nacc = 0
    for c in cycles:
        if c["status"]:
            continue
        nacc += 1
        for i, v in enumerate(quotients(c)):
            s[i] = s[i] + v
    rec = _empty(0)
    rec["n_cycles"], rec["n_rejected"] = nacc, len(cycles) - nacc
    if rec["n_rejected"]:
        rec["status"] |= GL_REJECTED
    if nacc == 0:
        rec["status"] |= GL_ALL_REJECTED
    else:
        for f, v in zip(FIELDS, s):
            rec[f] = v / float(nacc)
    return rec, cycles


def glottal(pcm, meas, marks, level_open=26, level_mid=128, polarity=1, cycles_pitch=0, cycles_fill=None):
    """rows of pcm (int16 [n][samples]) with the measurement's records (acoustic_ref.DTYPE or the library's) and marks
    (int32 [n][marks_pitch]).  Returns the records (REC_DTYPE) and, with cycles_pitch > 0, the cycle records
    [n][cycles_pitch] (CYCLE_DTYPE): slots the definition leaves untouched keep cycles_fill (one record for all, or
    the array as it was before the call; default: all bytes 0xFF)."""
    pcm = np.asarray(pcm)
    n = pcm.shape[0]
    out = np.zeros(n, dtype=REC_DTYPE)
    cyc = None
    if cycles_pitch:
        fill = np.frombuffer(b"\xff" * CYCLE_DTYPE.itemsize, dtype=CYCLE_DTYPE)[0] if cycles_fill is None else cycles_fill
        cyc = np.broadcast_to(np.asarray(fill, dtype=CYCLE_DTYPE), (n, cycles_pitch)).copy()
    for i in range(n):
        rec, cl = glottal_row(pcm[i], meas["n_periods"][i], meas["status"][i], marks[i], level_open, level_mid, polarity)
        for k, v in rec.items():
            out[i][k] = v
        for j, c in enumerate(cl[:cycles_pitch]):
            for k, v in c.items():
                cyc[i, j][k] = v
    return (out, cyc) if cycles_pitch else out


def measure_and_glottal(pcm, fs, level_open=26, level_mid=128, polarity=1, f0_min=50.0, f0_max=500.0, lengths=None,
                        marks_pitch=None, cycles_pitch=0):
    """the chain of vs_glottal() on the restatements: acoustic_ref.measure (marks -1 past the last), then glottal().
    Returns (meas, marks, records[, cycles])."""
    pcm = np.asarray(pcm)
    if marks_pitch is None:
        marks_pitch = pcm.shape[1] // 2 + 2
    meas, marks = ar.measure(pcm, fs, f0_min, f0_max, polarity, lengths, marks_pitch)
    res = glottal(pcm, meas, marks, level_open, level_mid, polarity, cycles_pitch)
    return (meas, marks) + (res if cycles_pitch else (res,))


COLUMNS = ("file", "OQ", "ClQ", "SQ", "QOQ", "NAQ", "cycles", "rejected", "status")


def format_line(name, rec):
    """one line of the `glottal` program for a record (the C program prints with these printf formats)"""
    def g(v):
        return "nan" if math.isnan(v) else "%.4f" % v
    return "%s %s %s %s %s %s %d %d %d" % (name, g(rec["oq"]), g(rec["clq"]), g(rec["sq"]), g(rec["qoq"]), g(rec["naq"]),
                                           int(rec["n_cycles"]), int(rec["n_rejected"]), int(rec["status"]))


def format_cycle_line(c):
    """one line of `glottal -c` for a cycle record"""
    return "# cycle " + " ".join("%d" % int(c[f]) for f in CYCLE_FIELDS)
