"""numpy restatement of the IAIF analysis (include/voice_synth.h, "IAIF"): the tests hold the device to it.

Vectorised over the frames of one window length, like lpc_ref.levinson_batch: every fma of the header is one call of
fma() below on arrays, every other product, sum and quotient one numpy operation on doubles, in the header's order.
r0, err, start, status, coefs and glottal are what the device must give bit for bit; the formants come from numpy.roots
of the device's own V2 (lpc_ref.formants_of), within VS_LPC_FORMANT_TOL_HZ.

fma() is a*b + c rounded once, computed from error-free transformations and one addition rounded to odd (Boldo and
Melquiond, "Emulation of FMA and correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 2008):
(uh, ul) = a*b exactly, (th, tl) = c + uh exactly, v = RO(tl + ul), result RN(th + v).  It needs no overflow and no
underflow in the products, which holds here (|e| <= 2^15, taps of a stable predictor, windows below 2^8); libm's fma
through ctypes (track_ref.fma) gives the same doubles but takes a Python call per element.  tests/test_iaif_ref.py holds
the two to each other, and this module to a scalar transcription of the header that uses libm's."""
import numpy as np

import lpc_ref as lr

SILENT, UNSTABLE = lr.SILENT, lr.UNSTABLE
_SPLIT = 134217729.0          # 2^27 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    c = _SPLIT * a
    ah = c - (c - a)
    al = a - ah
    c = _SPLIT * b
    bh = c - (c - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """a*b + c rounded once, elementwise on doubles (broadcasting)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        s, e = _two_sum(tl, ul)
        # round to odd: where the sum is inexact and its last bit even, one step towards the error
        s = np.ascontiguousarray(s)
        bits = s.view(np.int64)
        fix = (e != 0.0) & ((bits & 1) == 0) & np.isfinite(s)
        away = (e > 0.0) == (s > 0.0)
        v = np.where(fix, bits + np.where(away, 1, -1), bits).view(np.float64)
        return th + v


def opts(order=22, glottal_order=4, window=lr.HAMMING, window_s=0.025, hop_s=0.010, n_formants=5, f_lo=50.0, leak=0.99):
    if isinstance(window, str):
        window = {"hamming": lr.HAMMING, "rectangular": lr.RECTANGULAR}[window]
    return dict(order=order, glottal_order=glottal_order, window=window, window_s=window_s, hop_s=hop_s,
                n_formants=n_formants, f_lo=f_lo, leak=leak)


def lpc_opts(o):
    """the lpc_ref.opts() of the same frame plan"""
    return lr.opts(order=o["order"], window=o["window"], window_s=o["window_s"], hop_s=o["hop_s"], pre_emphasis=0,
                   n_formants=o["n_formants"], f_lo=o["f_lo"])


def fir(e, c):
    """FIR_c(e) over the extended frames e [frames][M + L] (column 0 is n = -M, zeros before); c [frames][len]"""
    acc = e.copy()
    for j in range(1, c.shape[1] + 1):
        acc[:, j:] = fma(c[:, j - 1:j], e[:, :-j], acc[:, j:])
    return acc


def integrate(y, rho):
    out = np.empty_like(y)
    state = np.zeros(y.shape[0])
    for n in range(y.shape[1]):
        state = fma(rho, state, y[:, n])
        out[:, n] = state
    return out


def autocorr(y, w, q):
    """r(0..q) [frames][q+1] of v = w * y, y [frames][L]: one fma chain per lag, n ascending"""
    m, L = y.shape
    v = np.zeros((m, L + q))
    v[:, :L] = w[None, :].astype(np.float64) * y
    acc = np.zeros((m, q + 1))
    for n in range(L):
        acc = fma(v[:, n:n + 1], v[:, n:n + q + 1], acc)   # lags with n + k >= L add a zero product: acc stays
    return acc


def analyse_frames(e, w, M, p, g, rho):
    """the four stages on extended frames e [frames][M + L]: dict r0, err, status, coefs [frames][p+1], glottal
    [frames][g+1], r_stage1 [frames][2]"""
    m = e.shape[0]
    status = np.zeros(m, np.int32)
    r0 = np.zeros(m)
    taps = np.zeros((m, 0))
    out = {}
    with np.errstate(all="ignore"):
        for stage, q in ((1, 1), (2, p), (3, g), (4, p)):
            y = fir(e, taps)
            if stage == 3:
                y = integrate(y, rho)
            r = autocorr(y[:, M:], w, q)
            A, err, st = lr.levinson_batch(r, q)
            alive = status == 0
            r0 = np.where(alive, r[:, 0], r0)
            status = np.where(alive, st, status)
            dead = status != 0
            taps = np.where(dead[:, None], 0.0, A[:, 1:])     # (a frame that ended: its later stages are not looked at)
            A = np.where(dead[:, None], np.nan, A)
            A[:, 0] = 1.0
            if stage == 1:
                out["r_stage1"] = r
            if stage == 3:
                out["glottal"] = A
    out.update(r0=r0, err=np.where(dead, np.nan, err), status=status, coefs=A)
    return out


def analyse(pcm, fs, lengths=None, **kw):
    """rows of pcm like Engine.iaif(..., coefs=True, glottal=True), without the formants: r0, err, start, status,
    n_frames, coefs, glottal over [rows][frames] (the same fill past a row's frames), and r_stage1"""
    pcm = np.asarray(pcm)
    n = pcm.shape[0]
    fs = np.broadcast_to(np.asarray(fs), (n,))
    lengths = np.broadcast_to(np.asarray(pcm.shape[1] if lengths is None else lengths), (n,))
    o = opts(**kw)
    lo = lpc_opts(o)
    p, g, rho = o["order"], o["glottal_order"], float(o["leak"])
    M = p + 1
    plans = []
    for i in range(n):
        plan = lr.frame_plan(int(fs[i]), int(lengths[i]), lo)
        if plan is None:
            raise ValueError("row %d refused" % i)
        plans.append(plan)
    nfr = np.array([len(pl[2]) for pl in plans], np.int32)
    fp = max(1, int(nfr.max()))
    res = dict(r0=np.full((n, fp), np.nan), err=np.full((n, fp), np.nan), start=np.full((n, fp), -1, np.int32),
               status=np.full((n, fp), -1, np.int32), n_frames=nfr, coefs=np.full((n, fp, p + 1), np.nan),
               glottal=np.full((n, fp, g + 1), np.nan), r_stage1=np.full((n, fp, 2), np.nan))
    frames = [(i, j, s, plans[i][0]) for i in range(n) for j, s in enumerate(plans[i][2])]
    x = np.concatenate([np.zeros((n, M)), pcm.astype(np.float64)], axis=1)     # x[:, M + t] is sample t; zeros before
    for L in sorted({f[3] for f in frames}):
        sel = [f for f in frames if f[3] == L]
        w = lr.window(L, o["window"])
        for c in range(0, len(sel), 2048):
            part = sel[c:c + 2048]
            rows = np.array([f[0] for f in part])
            jj = np.array([f[1] for f in part])
            s = np.array([f[2] for f in part])
            e = x[rows[:, None], s[:, None] + np.arange(M + L)[None, :]]       # e[n] at column n + M
            got = analyse_frames(e, w, M, p, g, rho)
            res["start"][rows, jj] = s
            for k in ("r0", "err", "status", "coefs", "glottal", "r_stage1"):
                res[k][rows, jj] = got[k]
    return res
