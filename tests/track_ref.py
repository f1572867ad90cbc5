"""numpy restatement of the coefficient tracks (include/voice_synth.h, "coefficient tracks"): the tests hold the device
and the library's host helpers to it.

Vectorised over rows (and sets), a Python loop over samples; every product, sum and quotient is one numpy operation on
doubles, i.e. rounded on its own, in the header's order.  What it returns is what the device must give byte for byte in
VS_ARITH_EXACT.  filter_track(arith="fma") restates the header's FMA form of step 4 with libm's fma(), and is what the
device must give byte for byte in VS_ARITH_FMA (tests/test_track_ref.py holds that fma to exact rational arithmetic)."""
import ctypes
import ctypes.util

import numpy as np

GROUP = 24
HOLD, GLIDE = 0, 1
NO_SET = 0x1

ROW_DTYPE = np.dtype([("n_sets", "<i4"), ("hop", "<i4"), ("offset", "<i4"), ("length", "<i4"), ("gain", "<f4"),
                      ("pre_emphasis", "<f4")])
STAT_DTYPE = np.dtype([("status", "<i4"), ("n_unusable", "<i4")])
P0, P1 = 22, 40       # the taps of the kernels' two window classes (csrc/vs_track.h): the FMA form runs over all of them

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma = np.frompyfunc(_libm.fma, 3, 1)


def fma(a, b, c):
    """a*b + c rounded once (libm's fma), elementwise on doubles"""
    return np.asarray(_fma(a, b, c), dtype=np.float64)


def round2int(x):
    """round2int() of vowel_new.c:413-427 on an array of doubles (tests/test_track_ref.py holds it to the oracle's)"""
    x = np.asarray(x, dtype=np.float64)
    dec = x - np.floor(x)
    x = np.where(dec > 0.5, x + 1, x)
    x = np.minimum(np.maximum(x, -32767.0), 32767.0)
    return np.floor(x).astype(np.int64).astype(np.int16)


def reflection(A):
    """step-down of A[..., 0..p] (element 0 ignored): (k[..., p], ok[...]); k is meaningless where ok is False"""
    A = np.asarray(A, dtype=np.float64)
    a = A[..., 1:].copy()
    p = a.shape[-1]
    ok = np.isfinite(a).all(axis=-1)
    with np.errstate(all="ignore"):
        for i in range(p, 0, -1):
            k = a[..., i - 1]
            ok = ok & (np.abs(k) < 1.0)
            if i > 1:
                d = 1.0 - k * k
                a[..., :i - 1] = (a[..., :i - 1] - k[..., None] * a[..., i - 2::-1]) / d[..., None]
    return a, ok


def step_up(kappa):
    """A[..., 0..p] (A[..., 0] = 1) of the reflection coefficients kappa[..., p]"""
    kappa = np.asarray(kappa, dtype=np.float64)
    p = kappa.shape[-1]
    a = np.zeros(kappa.shape[:-1] + (p + 1,), dtype=np.float64)
    a[..., 0] = 1.0
    t = a[..., 1:]
    with np.errstate(all="ignore"):
        for i in range(1, p + 1):
            ki = kappa[..., i - 1]
            if i > 1:
                t[..., :i - 1] = t[..., :i - 1] + ki[..., None] * t[..., i - 2::-1]
            t[..., i - 1] = ki
    return a


def glide_sets(A_from, A_to, n_sets):
    """n_sets >= 2 sets from A_from to A_to, evenly spaced in the reflection domain; None if an end fails its step-down"""
    kf, okf = reflection(A_from)
    kt, okt = reflection(A_to)
    if not (okf and okt):
        return None
    out = np.zeros((n_sets, len(kf) + 1))
    for s in range(n_sets):
        t = float(s) / float(n_sets - 1)
        out[s] = step_up(kf + t * (kt - kf))
    return out


def usable(coefs, mode, gains=None):
    """bool [rows][sets] of the header's step 1 (without regard to n_sets), and the reflection coefficients"""
    coefs = np.asarray(coefs, dtype=np.float64)
    ok = np.isfinite(coefs[..., 1:]).all(axis=-1)
    if gains is not None:
        ok = ok & np.isfinite(gains)
    k = None
    if mode == GLIDE:
        k, okk = reflection(coefs)
        ok = ok & okk
    return ok, k


def from_lpc(L, H, s0, n_frames, length, mode):
    """the row vs_track_from_lpc makes of a frame plan (tests/lpc_ref.frame_plan), or None where it refuses"""
    if n_frames < 1 or H < 1:
        return None
    off = s0 + L // 2 if mode == GLIDE else s0 + L // 2 - H // 2
    return (n_frames, H, off, length, 1.0, 0.0)


def filter_track(flow, coefs, rows, mode, gains=None, out=None, state_max=None, arith="exact", extremes=None, taps=None):
    """(pcm, stat): flow int16 [rows][samples], coefs [rows][sets][order+1], rows ROW_DTYPE records, gains [rows][sets]
    or None; out: the buffer written into (samples past a row's length keep its content; default zeros).  state_max: a
    list that receives the largest |y| seen (the tests' check that their sets keep the state small).  arith: "exact",
    or "fma" for the header's FMA form of step 4 (steps 1 to 3 are the same in every arithmetic).  extremes: a list that
    receives (lo, hi), two double arrays [rows]: the smallest and the largest o = the argument of round2int, before
    its clamp, over the samples the row is compared on (n < length, a usable set); +inf / -inf for a row without any.
    taps: a list that receives, per group of 24 samples, a_1..a_order of every row in that group, [rows][order]."""
    assert arith in ("exact", "fma")
    flow = np.asarray(flow, dtype=np.int16)
    coefs = np.asarray(coefs, dtype=np.float64)
    R, N = flow.shape
    p = coefs.shape[2] - 1
    S = coefs.shape[1]
    K = rows["n_sets"].astype(np.int64)
    hop = rows["hop"].astype(np.int64)
    offset = rows["offset"].astype(np.int64)
    length = rows["length"].astype(np.int64)
    gain = rows["gain"].astype(np.float64)
    pre = rows["pre_emphasis"].astype(np.float64)
    pcm = np.zeros((R, N), dtype=np.int16) if out is None else np.array(out, dtype=np.int16)

    ok, refl = usable(coefs, mode, gains)
    inK = np.arange(S)[None, :] < K[:, None]
    stat = np.zeros(R, dtype=STAT_DTYPE)
    stat["n_unusable"] = (inK & ~ok).sum(axis=1)
    okK = ok & inK
    none = ~okK.any(axis=1)
    stat["status"] = np.where(none, NO_SET, 0)
    # forward fill: eff[r][k] = the index of E_k
    first = np.argmax(okK, axis=1)
    eff = np.where(okK, np.arange(S)[None, :], -1)
    eff = np.maximum.accumulate(eff, axis=1)
    eff = np.where(eff < 0, first[:, None], eff)
    ri = np.arange(R)
    src = refl if mode == GLIDE else coefs[..., 1:]

    if arith == "fma":                           # the taps of the window class, zeros in the missing ones
        P = P0 if p <= P0 else P1
        pad = np.zeros((P - p, R))
        p = P
    Y = np.zeros((N + p, R), dtype=np.float64)   # y[n] at Y[n + p]
    O = np.zeros((N, R), dtype=np.int16)
    U = np.zeros((N, R), dtype=np.float64) if extremes is not None else None
    live = ~none
    worst = 0.0
    with np.errstate(all="ignore"):
        for m in range(0, int(length.max()) if R else 0, GROUP):
            mo = m - offset
            k = np.where(mo < 0, 0, np.minimum(mo // hop, K - 1))
            e0 = eff[ri, k]
            if mode == GLIDE:
                t = np.where((mo >= 0) & (k < K - 1), (mo - k * hop).astype(np.float64) / hop.astype(np.float64), 0.0)
                e1 = eff[ri, np.minimum(k + 1, K - 1)]
                ka, kb = src[ri, e0], src[ri, e1]
                a = step_up(ka + t[:, None] * (kb - ka))[:, 1:]
                if gains is not None:
                    ga, gb = gains[ri, e0], gains[ri, e1]
                    G = ga + t * (gb - ga)
            else:
                a = src[ri, e0]
                if gains is not None:
                    G = gains[ri, e0]
            if taps is not None:
                taps.append(np.array(a))
            aT = np.ascontiguousarray(a.T)
            if arith == "fma":
                aT = np.concatenate([aT, pad])
            xg = flow[:, m:m + GROUP].T.astype(np.float64)
            for n in range(m, min(m + GROUP, N)):
                acc = xg[n - m] * gain
                if gains is not None:
                    acc = acc * G
                if arith == "fma":
                    p0, p1 = acc, -(aT[1] * Y[n + p - 2])
                    for j in range(3, p + 1):
                        if j & 1:
                            p0 = fma(-aT[j - 1], Y[n + p - j], p0)
                        else:
                            p1 = fma(-aT[j - 1], Y[n + p - j], p1)
                    acc = fma(-aT[0], Y[n + p - 1], p0 + p1)
                    o = fma(-pre, Y[n + p - 1], acc)
                else:
                    for j in range(1, p + 1):
                        acc = acc - aT[j - 1] * Y[n + p - j]
                    o = acc - pre * Y[n + p - 1]
                Y[n + p] = acc
                O[n] = round2int(o)
                if U is not None:
                    U[n] = o
            if state_max is not None:
                seg = np.abs(Y[m + p:m + p + GROUP][:, live])
                if seg.size:
                    worst = max(worst, float(np.nanmax(np.where(np.isfinite(seg), seg, np.inf))))
    if state_max is not None:
        state_max.append(worst)
    inside = np.arange(N)[None, :] < length[:, None]
    if extremes is not None:
        seen = inside & live[:, None]
        extremes.append((np.where(seen, U.T, np.inf).min(axis=1, initial=np.inf),
                         np.where(seen, U.T, -np.inf).max(axis=1, initial=-np.inf)))
    pcm = np.where(inside, np.where(none[:, None], 0, O.T), pcm).astype(np.int16)
    return pcm, stat
