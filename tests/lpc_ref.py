"""numpy restatement of the LPC analysis (include/voice_synth.h, "LPC analysis"): the tests hold the device to it.

The autocorrelation is an int64 dot product (exact), Levinson-Durbin runs on Python floats in the order the header
writes, and the formants come from numpy.roots.  r0, err, start, status and the coefficients are what the device must
give bit for bit; the formants are within the header's VS_LPC_FORMANT_TOL_HZ of numpy.roots."""
import math

import numpy as np

MAX_WINDOW = 16384
SILENT, UNSTABLE, NO_ROOTS = 0x1, 0x2, 0x4
HAMMING, RECTANGULAR = 0, 1


def opts(order=22, window=HAMMING, window_s=0.025, hop_s=0.010, pre_emphasis=0, n_formants=5, f_lo=50.0):
    if isinstance(window, str):
        window = {"hamming": HAMMING, "rectangular": RECTANGULAR}[window]
    return dict(order=order, window=window, window_s=window_s, hop_s=hop_s, pre_emphasis=pre_emphasis,
                n_formants=n_formants, f_lo=f_lo)


def frame_plan(fs, length, o):
    """(L, H, starts) of a row, or None where the library refuses the row (VS_ERR_RANGE)"""
    L = int(math.floor(float(o["window_s"]) * fs + 0.5))
    H = int(math.floor(float(o["hop_s"]) * fs + 0.5))
    pre = o["pre_emphasis"]
    if not (o["order"] < L <= MAX_WINDOW):
        return None
    if o["hop_s"] > 0:
        if H < 1:
            return None
        n = 1 + (length - pre - L) // H if length >= pre + L else 0
        return L, H, [pre + j * H for j in range(n)]
    return L, 0, ([pre + (length - pre - L) // 2] if length >= pre + L else [])


def window(L, kind=HAMMING):
    if kind == RECTANGULAR:
        return np.full(L, 256, dtype=np.int64)
    return np.array([int(math.floor(256.0 * (0.54 - 0.46 * math.cos(2.0 * math.pi * n / (L - 1))) + 0.5))
                     for n in range(L)], dtype=np.int64)


def autocorr(x, s, L, order, w, pre):
    """exact r(0..order) as Python ints of the frame starting at s"""
    x = np.asarray(x, dtype=np.int64)
    d = x[s:s + L] - x[s - 1:s + L - 1] if pre else x[s:s + L]
    v = w * d
    return [int(np.dot(v[:L - k], v[k:])) for k in range(order + 1)]


def levinson(r, order):
    """(A[0..order], err, status) in the header's order of operations (NaN taps and err on failure)"""
    rf = [float(t) for t in r]
    a = [0.0] * (order + 1)
    if rf[0] == 0.0:
        return [1.0] + [math.nan] * order, math.nan, SILENT
    e = rf[0]
    for i in range(1, order + 1):
        acc = rf[i]
        for j in range(1, i):
            acc = acc + a[j] * rf[i - j]
        k = -acc / e
        if not abs(k) < 1.0:
            return [1.0] + [math.nan] * order, math.nan, UNSTABLE
        na = a[:]
        for j in range(1, i):
            na[j] = a[j] + k * a[i - j]
        na[i] = k
        a = na
        e = e * (1.0 - k * k)
        if not e > 0.0:
            return [1.0] + [math.nan] * order, math.nan, UNSTABLE
    a[0] = 1.0
    return a, e, 0


def formants_of(A, fs, n, f_lo=50.0):
    """(f, bw) pairs of the roots of A with Im z > 0 and f_lo <= f <= fs/2 - f_lo, ascending f, the first n"""
    z = np.roots(np.asarray(A, dtype=np.float64))
    z = z[z.imag > 0]
    f = fs * np.arctan2(z.imag, z.real) / (2 * np.pi)
    bw = -fs * np.log(np.abs(z)) / np.pi
    keep = (f >= f_lo) & (f <= fs / 2 - f_lo)
    f, bw = f[keep], bw[keep]
    o = np.argsort(f, kind="stable")
    return [(float(f[i]), float(bw[i])) for i in o[:n]]


def analyse_row(x, fs, length=None, coefs=False, **kw):
    """one row: a list of frame dicts (r0, err, start, status, A, formants)"""
    o = opts(**kw)
    length = len(x) if length is None else length
    plan = frame_plan(fs, length, o)
    if plan is None:
        raise ValueError("row refused")
    L, H, starts = plan
    w = window(L, o["window"])
    out = []
    for s in starts:
        r = autocorr(x, s, L, o["order"], w, o["pre_emphasis"])
        A, e, st = levinson(r, o["order"])
        fm = formants_of(A, fs, o["n_formants"], o["f_lo"]) if st == 0 and o["n_formants"] > 0 else []
        out.append(dict(r0=float(r[0]), r=r, err=e, start=s, status=st, A=A, formants=fm))
    return out


def levinson_batch(r, order):
    """levinson() on every row of r (float64 [frames][order+1]) at once: the same operations, elementwise, so the same
    doubles.  (A [frames][order+1], err, status)"""
    m = r.shape[0]
    a = np.zeros((m, order + 1))
    st = np.where(r[:, 0] == 0.0, SILENT, 0).astype(np.int32)
    e = r[:, 0].copy()
    with np.errstate(all="ignore"):
        for i in range(1, order + 1):
            acc = r[:, i].copy()
            for j in range(1, i):
                acc = acc + a[:, j] * r[:, i - j]
            k = -acc / e
            st[(st == 0) & ~(np.abs(k) < 1.0)] = UNSTABLE
            na = a.copy()
            for j in range(1, i):
                na[:, j] = a[:, j] + k * a[:, i - j]
            na[:, i] = k
            a = na
            e = e * (1.0 - k * k)
            st[(st == 0) & ~(e > 0.0)] = UNSTABLE
    a[:, 0] = 1.0
    a[st != 0, 1:] = np.nan
    e[st != 0] = np.nan
    return a, e, st


def analyse(pcm, fs, lengths=None, **kw):
    """rows of pcm like Engine.lpc(..., coefs=True), without the formants: r0, err, start, status, n_frames and coefs
    over [rows][frames] (the same fill past a row's frames)"""
    pcm = np.asarray(pcm)
    n = pcm.shape[0]
    fs = np.broadcast_to(np.asarray(fs), (n,))
    lengths = np.broadcast_to(np.asarray(pcm.shape[1] if lengths is None else lengths), (n,))
    o = opts(**kw)
    p, pre = o["order"], o["pre_emphasis"]
    plans = []
    for i in range(n):
        plan = frame_plan(int(fs[i]), int(lengths[i]), o)
        if plan is None:
            raise ValueError("row %d refused" % i)
        plans.append(plan)
    nfr = np.array([len(pl[2]) for pl in plans], np.int32)
    fp = max(1, int(nfr.max()))
    res = dict(r0=np.full((n, fp), np.nan), err=np.full((n, fp), np.nan), start=np.full((n, fp), -1, np.int32),
               status=np.full((n, fp), -1, np.int32), n_frames=nfr, coefs=np.full((n, fp, p + 1), np.nan))
    frames = [(i, j, s, plans[i][0]) for i in range(n) for j, s in enumerate(plans[i][2])]
    x64 = pcm.astype(np.int64)
    for L in sorted({f[3] for f in frames}):
        sel = [f for f in frames if f[3] == L]
        w = window(L, o["window"])
        for c in range(0, len(sel), 4096):
            part = sel[c:c + 4096]
            rows = np.array([f[0] for f in part])
            idx = np.array([f[2] for f in part])[:, None] + np.arange(L)[None, :]
            d = x64[rows[:, None], idx]
            if pre:
                d = d - x64[rows[:, None], idx - 1]
            v = d * w[None, :]
            r = np.stack([(v[:, :L - k] * v[:, k:]).sum(axis=1) for k in range(p + 1)], axis=1)
            A, e, st = levinson_batch(r.astype(np.float64), p)
            jj = np.array([f[1] for f in part])
            res["r0"][rows, jj] = r[:, 0].astype(np.float64)
            res["err"][rows, jj] = e
            res["start"][rows, jj] = idx[:, 0]
            res["status"][rows, jj] = st
            res["coefs"][rows, jj] = A
    return res


def impulse_response(A, n=4096, peak=30000.0):
    """h of 1/A(z) for n samples, scaled to the given peak and rounded to int16"""
    A = np.asarray(A, dtype=np.float64)
    p = len(A) - 1
    h = np.zeros(n)
    for t in range(n):
        acc = 1.0 if t == 0 else 0.0
        for j in range(1, min(p, t) + 1):
            acc -= A[j] * h[t - j]
        h[t] = acc
    return np.round(h * (peak / np.abs(h).max())).astype(np.int16)


def table_formants(A, fs, f_lo=50.0, n=20):
    return formants_of(A, fs, n, f_lo)
