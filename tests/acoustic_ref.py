"""numpy restatement of the acoustic measurement defined in include/voice_synth.h ("Acoustic measurement").

Test infrastructure only: the product never imports it.  Every step follows the header's text in the same order, so
that the integer fields and the marks of the device must equal these bit for bit, and the double fields (but for the
two that go through log10) must be equal as well.
"""
import math

import numpy as np

AC_TOO_SHORT = 0x1
AC_UNVOICED = 0x2
AC_FEW_PERIODS = 0x4
AC_ZERO_AMPLITUDE = 0x8
AC_MAX_LAG = 2048

NAN = float("nan")

FIELDS = ("f0_hz", "jitter_local", "jitter_abs_s", "jitter_rap", "jitter_ppq5",
          "shimmer_local", "shimmer_db", "shimmer_apq3", "shimmer_apq5", "hnr_db")
DTYPE = np.dtype([(f, "<f8") for f in FIELDS] + [("p0", "<i4"), ("n_periods", "<i4"), ("first_mark", "<i4"),
                                                   ("status", "<i4")])


def lag_bounds(fs, f0_min=50.0, f0_max=500.0):
    """(tmin, tmax) as the host computes them; ValueError where the library returns an error"""
    f0_min = float(np.float32(f0_min))
    f0_max = float(np.float32(f0_max))
    if not (f0_min > 0 and f0_max > 0) or fs <= 0:
        raise ValueError("bad rate or F0 bounds")
    tmin = int(math.floor(float(fs) / f0_max))
    tmax = int(math.ceil(float(fs) / f0_min))
    if tmin < 2 or tmin >= tmax or tmax > AC_MAX_LAG:   # (the library: VS_ERR_RANGE)
        raise ValueError("lag bounds %d..%d out of range" % (tmin, tmax))
    return tmin, tmax


def period_estimate(x, tmin, tmax):
    """stage A: (status bits, P0, hnr_db) of one row (x int64)"""
    n = len(x)
    if n < 3 * tmax + 2:
        return AC_TOO_SHORT, 0, NAN
    W = 2 * tmax
    s = (n - W - tmax - 1) // 2
    a = x[s:s + W]
    r = {t: int(np.dot(a, x[s + t:s + t + W])) for t in range(tmin - 1, tmax + 2)}
    r0 = int(np.dot(a, a))
    rmax = max(r[t] for t in range(tmin, tmax + 1))
    if rmax <= 0:
        return AC_UNVOICED, 0, NAN
    p0 = None
    for t in range(tmin, tmax + 1):
        if r[t] > r[t - 1] and r[t] >= r[t + 1] and 10 * r[t] >= 9 * rmax:
            p0 = t
            break
    if p0 is None:
        p0 = next(t for t in range(tmin, tmax + 1) if r[t] == rmax)
    b = x[s + p0:s + p0 + W]
    e = int(np.dot(b, b))
    rho = float(r[p0]) / math.sqrt(float(r0) * float(e))   # (rmax > 0: neither r0 nor e is 0)
    rho = min(max(rho, 1e-10), 1.0 - 1e-10)
    return 0, p0, 10.0 * math.log10(rho / (1.0 - rho))


def cycle_marks(y, p0, tmin, tmax):
    """stage B: marks m_0..m_K and amplitudes a_1..a_K of one row (y = polarity * x, int64)"""
    n = len(y)
    m = [int(np.argmax(y[:tmax]))]
    lo1, hi1 = max(tmin, (2 * p0 + 2) // 3), min(tmax, (3 * p0) // 2)
    lo, hi = lo1, hi1
    d = (p0 + 3) // 4
    amps = []
    while m[-1] + hi < n:
        w0, w1 = m[-1] + lo, m[-1] + hi
        k = w0 + int(np.argmax(y[w0:w1 + 1]))
        amps.append(int(y[k]) - int(y[m[-1]:k].min()))
        T = k - m[-1]
        m.append(k)
        lo, hi = max(lo1, T - d), min(hi1, T + d)
    return m, amps


def _perturbation(v, mean):
    """(local, rap/apq3, ppq5/apq5) of the sequence v (python ints), each NaN when v is too short"""
    K = len(v)
    loc = rap = ppq = NAN
    if K >= 2:
        loc = (float(sum(abs(v[i + 1] - v[i]) for i in range(K - 1))) / float(K - 1)) / mean
    if K >= 3:
        s3 = sum(abs(3 * v[i] - (v[i - 1] + v[i] + v[i + 1])) for i in range(1, K - 1))
        rap = (float(s3) / (3.0 * float(K - 2))) / mean
    if K >= 5:
        s5 = sum(abs(5 * v[i] - sum(v[i - 2:i + 3])) for i in range(2, K - 2))
        ppq = (float(s5) / (5.0 * float(K - 4))) / mean
    return loc, rap, ppq


def measure_row(x, fs, f0_min=50.0, f0_max=500.0, polarity=1, marks_pitch=0):
    """(record as a dict, marks list truncated to marks_pitch) of one row"""
    tmin, tmax = lag_bounds(fs, f0_min, f0_max)
    x = np.asarray(x, dtype=np.int64)
    y = x * int(polarity)
    rec = {f: NAN for f in FIELDS}
    rec.update(p0=0, n_periods=0, first_mark=-1, status=0)
    st, p0, hnr = period_estimate(y, tmin, tmax)
    rec["status"] = st
    if st:
        return rec, []
    rec["p0"] = p0
    rec["hnr_db"] = hnr
    m, amps = cycle_marks(y, p0, tmin, tmax)
    T = [m[i + 1] - m[i] for i in range(len(m) - 1)]
    K = len(T)
    rec["n_periods"] = K
    rec["first_mark"] = m[0]
    if K < 2:
        rec["status"] |= AC_FEW_PERIODS
    if K >= 1:
        Tm = float(sum(T)) / float(K)
        rec["f0_hz"] = float(fs) / Tm
        loc, rap, ppq = _perturbation(T, Tm)
        rec["jitter_local"], rec["jitter_rap"], rec["jitter_ppq5"] = loc, rap, ppq
        if K >= 2:
            rec["jitter_abs_s"] = (float(sum(abs(T[i + 1] - T[i]) for i in range(K - 1))) / float(K - 1)) / float(fs)
        if min(amps) <= 0:
            rec["status"] |= AC_ZERO_AMPLITUDE
        else:
            Am = float(sum(amps)) / float(K)
            loc, apq3, apq5 = _perturbation(amps, Am)
            rec["shimmer_local"], rec["shimmer_apq3"], rec["shimmer_apq5"] = loc, apq3, apq5
            if K >= 2:
                sdb = 0.0
                for i in range(K - 1):
                    sdb += abs(20.0 * math.log10(float(amps[i + 1]) / float(amps[i])))
                rec["shimmer_db"] = sdb / float(K - 1)
    return rec, (m[:marks_pitch] if marks_pitch else [])


def measure(pcm, fs, f0_min=50.0, f0_max=500.0, polarity=1, lengths=None, marks=0):
    """rows of pcm (int16 [n][samples]); fs scalar or per row.  Returns the structured array (DTYPE) and, when marks > 0,
    an int32 [n][marks] array of the marks (-1 past the last)."""
    pcm = np.asarray(pcm)
    n = pcm.shape[0]
    fs = np.broadcast_to(np.asarray(fs, dtype=np.int64), (n,))
    out = np.zeros(n, dtype=DTYPE)
    mk = np.full((n, marks), -1, dtype=np.int32) if marks else None
    for i in range(n):
        L = pcm.shape[1] if lengths is None else int(lengths[i])
        rec, m = measure_row(pcm[i, :L], int(fs[i]), f0_min, f0_max, polarity, marks)
        for k, v in rec.items():
            out[i][k] = v
        if marks:
            mk[i, :len(m)] = m
    return (out, mk) if marks else out


COLUMNS = ("file", "F0_Hz", "jitter_%", "jitter_abs_us", "RAP_%", "PPQ5_%", "shimmer_%", "shimmer_dB", "APQ3_%",
           "APQ5_%", "HNR_dB", "periods", "status")


def format_line(name, rec):
    """one line of the `acoustic` program for a record (the C program prints with these printf formats)"""
    def g(v, scale, fmt):
        return "nan" if math.isnan(v) else fmt % (v * scale)
    return "%s %s %s %s %s %s %s %s %s %s %s %d %d" % (
        name, g(rec["f0_hz"], 1.0, "%.3f"), g(rec["jitter_local"], 100.0, "%.4f"), g(rec["jitter_abs_s"], 1e6, "%.3f"),
        g(rec["jitter_rap"], 100.0, "%.4f"), g(rec["jitter_ppq5"], 100.0, "%.4f"), g(rec["shimmer_local"], 100.0, "%.4f"),
        g(rec["shimmer_db"], 1.0, "%.4f"), g(rec["shimmer_apq3"], 100.0, "%.4f"), g(rec["shimmer_apq5"], 100.0, "%.4f"),
        g(rec["hnr_db"], 1.0, "%.3f"), int(rec["n_periods"]), int(rec["status"]))
