"""numpy restatement of the inverse filter (include/voice_synth.h, "inverse filtering"): the tests hold the device and
the library's host helper to it.

Steps 1 to 3 (usable sets, forward fill, which set per group of 24 samples, the glide through the reflection domain) are
the coefficient tracks' and are taken from tests/track_ref.py (usable / reflection / step_up), in the arrangement of
track_ref.filter_track.  Step 4 is vectorised over rows with a Python loop over samples for the one recurrence there is,
u[n] = s[n] + rho*u[n-1]; the tap sums of a group's samples do not depend on one another and are taken over the whole
group at once, which is the same operations on the same operands in the same order for every sample.  Every product and
sum is one numpy operation on doubles, i.e. rounded on its own; arith="fma" restates the header's FMA form with libm's
fma() (tests/test_track_ref.py holds that fma to exact rational arithmetic).  What inverse_filter returns is what the
device must give byte for byte, output and stat, in the matching arithmetic."""
import numpy as np

import track_ref as tr

GROUP = tr.GROUP
HOLD, GLIDE = tr.HOLD, tr.GLIDE
NO_SET = 0x1

ROW_DTYPE = np.dtype([("n_sets", "<i4"), ("hop", "<i4"), ("offset", "<i4"), ("length", "<i4"), ("scale", "<f4"),
                      ("de_emphasis", "<f4")])
STAT_DTYPE = np.dtype([("status", "<i4"), ("n_unusable", "<i4"), ("n_clipped", "<i4"), ("reserved_", "<i4")])


def rows_of(n, n_sets, hop, offset, length, scale=1.0, de_emphasis=0.0):
    rows = np.zeros(n, dtype=ROW_DTYPE)
    rows["n_sets"], rows["hop"], rows["offset"], rows["length"] = n_sets, hop, offset, length
    rows["scale"], rows["de_emphasis"] = scale, de_emphasis
    return rows


def from_lpc(L, H, s0, n_frames, length, mode):
    """the row vs_inverse_from_lpc makes of a frame plan (tests/lpc_ref.frame_plan), or None where it refuses"""
    t = tr.from_lpc(L, H, s0, n_frames, length, mode)
    return None if t is None else t[:4] + (1.0, 0.0)


def clipped(x):
    """bool: where round2int's clamp changes the value (x: its argument)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        dec = x - np.floor(x)
        fl = np.floor(np.where(dec > 0.5, x + 1, x))
        return (fl > 32767.0) | (fl < -32767.0)


def impulse_response(A, rho, n):
    """h[0..n) of A(z) / (1 - rho z^-1), A[0] taken as 1"""
    A = np.asarray(A, dtype=np.float64)
    h = np.zeros(n)
    prev = 0.0
    for i in range(n):
        a = 1.0 if i == 0 else (A[i] if i < len(A) else 0.0)
        prev = a + rho * prev
        h[i] = prev
    return h


def round_trip_bound(A, rho, scale, n):
    """consequence (c) of the header: 0.5 * scale * sum_{i<n} |h[i]| + 1.5"""
    return 0.5 * abs(float(scale)) * float(np.abs(impulse_response(A, float(rho), n)).sum()) + 1.5


def inverse_filter(pcm, coefs, rows, mode, out=None, arith="exact", extremes=None):
    """(flow, stat): pcm int16 [rows][samples], coefs [rows][sets][order+1], rows ROW_DTYPE records; out: the buffer
    written into (samples past a row's length keep its content; default zeros).  arith: "exact" or "fma".  extremes: a
    list that receives (lo, hi), two double arrays [rows]: the smallest and the largest e*c, the argument of round2int,
    over the samples the row is compared on (n < length, a usable set); +inf / -inf for a row without any."""
    assert arith in ("exact", "fma")
    pcm = np.asarray(pcm, dtype=np.int16)
    coefs = np.asarray(coefs, dtype=np.float64)
    R, N = pcm.shape
    p = coefs.shape[2] - 1
    S = coefs.shape[1]
    K = rows["n_sets"].astype(np.int64)
    hop = rows["hop"].astype(np.int64)
    offset = rows["offset"].astype(np.int64)
    length = rows["length"].astype(np.int64)
    c = rows["scale"].astype(np.float64)
    rho = rows["de_emphasis"].astype(np.float64)
    flow = np.zeros((R, N), dtype=np.int16) if out is None else np.array(out, dtype=np.int16)

    # steps 1 to 3: as track_ref.filter_track, without gains
    ok, refl = tr.usable(coefs, mode)
    inK = np.arange(S)[None, :] < K[:, None]
    stat = np.zeros(R, dtype=STAT_DTYPE)
    stat["n_unusable"] = (inK & ~ok).sum(axis=1)
    okK = ok & inK
    none = ~okK.any(axis=1)
    stat["status"] = np.where(none, NO_SET, 0)
    first = np.argmax(okK, axis=1)
    eff = np.where(okK, np.arange(S)[None, :], -1)
    eff = np.maximum.accumulate(eff, axis=1)
    eff = np.where(eff < 0, first[:, None], eff)
    ri = np.arange(R)
    src = refl if mode == GLIDE else coefs[..., 1:]

    if arith == "fma":                           # the taps of the window class, zeros in the missing ones
        P = tr.P0 if p <= tr.P0 else tr.P1
        pad = np.zeros((P - p, R))
        p = P
    U = np.zeros((N + p, R), dtype=np.float64)   # u[n] at U[n + p]
    X = np.zeros((N, R), dtype=np.float64)       # e*c
    sT = pcm.T.astype(np.float64)
    with np.errstate(all="ignore"):
        for m in range(0, int(length.max()) if R else 0, GROUP):
            mo = m - offset
            k = np.where(mo < 0, 0, np.minimum(mo // hop, K - 1))
            e0 = eff[ri, k]
            if mode == GLIDE:
                t = np.where((mo >= 0) & (k < K - 1), (mo - k * hop).astype(np.float64) / hop.astype(np.float64), 0.0)
                e1 = eff[ri, np.minimum(k + 1, K - 1)]
                ka, kb = src[ri, e0], src[ri, e1]
                a = tr.step_up(ka + t[:, None] * (kb - ka))[:, 1:]
            else:
                a = src[ri, e0]
            aT = np.ascontiguousarray(a.T)
            if arith == "fma":
                aT = np.concatenate([aT, pad])
            g1 = min(m + GROUP, N)
            for n in range(m, g1):               # the de-emphasis: the one chain from sample to sample
                if arith == "fma":
                    U[n + p] = tr.fma(rho, U[n + p - 1], sT[n])
                else:
                    U[n + p] = sT[n] + rho * U[n + p - 1]
            # the tap sums of the group's samples, all at once: w(j) = u[n-j] for n = m .. g1-1
            def w(j):
                return U[m + p - j:g1 + p - j]
            if arith == "fma":
                p0, p1 = w(0), aT[1] * w(2)
                for j in range(3, p + 1):
                    if j & 1:
                        p0 = tr.fma(aT[j - 1], w(j), p0)
                    else:
                        p1 = tr.fma(aT[j - 1], w(j), p1)
                e = tr.fma(aT[0], w(1), p0 + p1)
            else:
                e = w(0)
                for j in range(1, p + 1):
                    e = e + aT[j - 1] * w(j)
            X[m:g1] = e * c
    inside = np.arange(N)[None, :] < length[:, None]
    seen = inside & ~none[:, None]
    stat["n_clipped"] = (clipped(X.T) & seen).sum(axis=1)
    if extremes is not None:
        extremes.append((np.where(seen, X.T, np.inf).min(axis=1, initial=np.inf),
                         np.where(seen, X.T, -np.inf).max(axis=1, initial=-np.inf)))
    with np.errstate(all="ignore"):
        O = tr.round2int(X.T)
    flow = np.where(inside, np.where(none[:, None], 0, O), flow).astype(np.int16)
    return flow, stat
