"""numpy restatement of the closed-phase covariance LPC (include/voice_synth.h, "closed-phase covariance LPC"): the tests
hold the device to it.

Test infrastructure only: the product never imports it.  The steps follow the header's text in its order.  phi is made
of Python integers (exact, whatever the size); the solve runs on doubles with every fma of the header one call of
iaif_ref.fma (a*b + c rounded once) on arrays over the frames, every other product and quotient one numpy operation, so
r0, err, start, status, the taps and the counts are what the device must give bit for bit.  The step-down is
track_ref.reflection; the formants come from numpy.roots of the device's own set (lpc_ref.formants_of), within
VS_LPC_FORMANT_TOL_HZ.
"""
import math

import numpy as np

import acoustic_ref as ar
import glottal_ref as gl
import iaif_ref as ia
import inverse_ref as ir
import lpc_ref as lr
import track_ref as tr
from iaif_ref import fma

SILENT, NO_ROOTS = lr.SILENT, lr.NO_ROOTS
FEW_EQUATIONS, SINGULAR, NOT_MINIMUM_PHASE = 0x10, 0x20, 0x40
ANCHOR_CLOSE, ANCHOR_GCI, ANCHOR_PEAK = 0, 1, 2
ANCHOR_FIELD = {ANCHOR_CLOSE: "close", ANCHOR_GCI: "gci", ANCHOR_PEAK: "peak"}
CLAMP = 32767
MAX_EQUATIONS = 1 << 31

OPTS_DTYPE = np.dtype([("order", "<i4"), ("anchor", "<i4"), ("delay", "<i4"), ("span_q", "<i4"), ("min_equations", "<i4"),
                       ("n_formants", "<i4"), ("window_s", "<f8"), ("hop_s", "<f8"), ("f_lo", "<f8"), ("reserved_", "<i8")])


def opts(order=22, anchor=ANCHOR_CLOSE, delay=4, span_q=77, min_equations=0, n_formants=5, window_s=0.0, hop_s=0.010,
         f_lo=50.0):
    if isinstance(anchor, str):
        anchor = {"close": ANCHOR_CLOSE, "gci": ANCHOR_GCI, "peak": ANCHOR_PEAK}[anchor]
    return dict(order=order, anchor=anchor, delay=delay, span_q=span_q, min_equations=min_equations,
                n_formants=n_formants, window_s=window_s, hop_s=hop_s, f_lo=f_lo)


def lpc_opts(o):
    """the lpc_ref.opts() of the same frame plan (window_s > 0)"""
    return lr.opts(order=o["order"], window=lr.RECTANGULAR, window_s=o["window_s"], hop_s=o["hop_s"], pre_emphasis=0,
                   n_formants=o["n_formants"], f_lo=o["f_lo"])


def frames_of(fs, length, o):
    """[(start, L)] of a row: one frame over the row with window_s == 0, else the LPC analysis's; None where refused"""
    if o["window_s"] == 0:
        return [(0, length)]
    plan = lr.frame_plan(fs, length, lpc_opts(o))
    if plan is None:
        return None
    return [(s, plan[0]) for s in plan[2]]


def cycle_count(rec, cycles_pitch):
    """step 1: C"""
    if int(rec["status"]) & (gl.GL_NO_CYCLES | gl.GL_BAD_MARKS):
        return 0
    total = int(rec["n_cycles"]) + int(rec["n_rejected"])
    return 0 if total < 0 else min(total, cycles_pitch)


def accepted_spans(x, rec, cycles, o):
    """steps 1 to 4 on one row: x = the row's len samples (nothing else is handed over, so nothing else can be read);
    the accepted (b, e) in the order of their slots"""
    n = len(x)
    p = o["order"]
    out = []
    for c in range(cycle_count(rec, len(cycles))):
        cy = cycles[c]
        period = int(cy["period"])
        if int(cy["status"]) != 0 or period <= 0:
            continue
        b = int(cy[ANCHOR_FIELD[o["anchor"]]]) + int(o["delay"])
        e = b + (int(o["span_q"]) * period) // 256
        if not (0 <= b and e <= n and e - b >= p + 1):
            continue
        seg = np.asarray(x[b:e], dtype=np.int64)
        if ((seg >= CLAMP) | (seg <= -CLAMP)).any():
            continue
        out.append((b, e))
    return out


def pooled(spans, start, L, p):
    """steps 5 and 6: the spans of the frame [start, start + L), cut where n_eq would reach 2^31; (spans, n_eq)"""
    got, n_eq = [], 0
    for b, e in spans:
        if not (start <= b and e <= start + L):
            continue
        if n_eq + (e - b - p) >= MAX_EQUATIONS:
            break
        got.append((b, e))
        n_eq += e - b - p
    return got, n_eq


def phi_direct(x, spans, p):
    """phi(i, k) as the header writes it: an object array [p+1][p+1] of Python integers"""
    phi = np.zeros((p + 1, p + 1), dtype=object)
    x = np.asarray(x, dtype=np.int64)
    for b, e in spans:
        X = np.stack([x[b + p - i:e - i] for i in range(p + 1)])           # X[i][n - b - p] = x[n - i]
        blk = 1 << 20                                                      # products below 2^30: 2^20 of them in int64
        for c in range(0, X.shape[1], blk):
            phi = phi + (X[:, c:c + blk] @ X[:, c:c + blk].T).astype(object)
    return phi


def phi_recurrence(x, spans, p):
    """the same from the first row alone: phi(i+1,k+1) = phi(i,k) + x[b+p-1-i]*x[b+p-1-k] - x[e-1-i]*x[e-1-k] per span"""
    phi = np.zeros((p + 1, p + 1), dtype=object)
    for b, e in spans:
        xs = [int(v) for v in x[b:e]]                                      # xs[n - b]
        s = [[0] * (p + 1) for _ in range(p + 1)]
        for k in range(p + 1):
            s[0][k] = s[k][0] = sum(xs[n] * xs[n - k] for n in range(p, e - b))
        for i in range(p):
            for k in range(i, p):
                s[i + 1][k + 1] = s[k + 1][i + 1] = (s[i][k] + xs[p - 1 - i] * xs[p - 1 - k]
                                                     - xs[e - b - 1 - i] * xs[e - b - 1 - k])
        phi = phi + np.array(s, dtype=object)
    return phi


def solve_batch(c):
    """step 8 on c [frames][p+1][p+1] doubles, every frame at once: (a [frames][p+1] with element 0 = 1, err, singular)"""
    m, p = c.shape[0], c.shape[1] - 1
    l = np.zeros((m, p + 1, p + 1))
    d = np.ones((m, p + 1))
    singular = np.zeros(m, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(1, p + 1):
            u = l[:, j, :] * d                                             # u_k = l_jk * d_k
            dj = c[:, j, j].copy()
            for k in range(1, j):
                dj = fma(-l[:, j, k], u[:, k], dj)
            singular |= ~((dj > 0.0) & np.isfinite(dj))                    # (a frame that stopped: its later steps are not looked at)
            d[:, j] = dj
            if j < p:
                t = c[:, j + 1:, j].copy()
                for k in range(1, j):
                    t = fma(-l[:, j + 1:, k], u[:, k:k + 1], t)
                l[:, j + 1:, j] = t / dj[:, None]
        z = np.zeros((m, p + 1))
        for i in range(1, p + 1):
            zi = -c[:, i, 0]
            for k in range(1, i):
                zi = fma(-l[:, i, k], z[:, k], zi)
            z[:, i] = zi
        y = z / d
        a = np.zeros((m, p + 1))
        for i in range(p, 0, -1):
            ai = y[:, i].copy()
            for k in range(i + 1, p + 1):
                ai = fma(-l[:, k, i], a[:, k], ai)
            a[:, i] = ai
        err = c[:, 0, 0].copy()
        for i in range(1, p + 1):
            err = fma(a[:, i], c[:, 0, i], err)
    a[:, 0] = 1.0
    a[singular, 1:] = np.nan
    err[singular] = np.nan
    return a, err, singular


def finish_batch(phis, n_eqs, o):
    """steps 7 to 9 on the frames' phi (phi_direct's arrays) and n_eq: (r0, err, status, A [frames][p+1])"""
    p = o["order"]
    m = len(phis)
    need = o["min_equations"] if o["min_equations"] else 2 * p
    c = np.array([np.asarray(phi, dtype=np.float64) for phi in phis]).reshape(m, p + 1, p + 1)   # float(int): nearest-even
    status = np.zeros(m, np.int32)
    for f in range(m):
        if n_eqs[f] < need:
            status[f] = FEW_EQUATIONS
        elif phis[f][0][0] == 0:
            status[f] = SILENT
    a, err, singular = solve_batch(c) if m else (np.zeros((0, p + 1)), np.zeros(0), np.zeros(0, bool))
    early = status != 0
    status[~early & singular] = SINGULAR
    dead = status != 0
    a[dead, 1:] = np.nan
    err[dead] = np.nan
    if m:
        _, ok = tr.reflection(np.where(dead[:, None], 0.0, a))
        status[~dead & ~ok] = NOT_MINIMUM_PHASE
    return c[:, 0, 0].copy(), err, status, a


def analyse(pcm, fs, glottal, cycles, lengths=None, **kw):
    """rows of pcm like Engine.cplpc(..., coefs=True, counts=True), without the formants: r0, err, start, status, n_frames,
    coefs, counts over [rows][frames] (NaN, -1 and -1 past a row's frames), and spans: per row, per frame, the pooled
    (b, e).  glottal: the rows' records (glottal_ref.REC_DTYPE or the library's), cycles [rows][cycles_pitch]."""
    pcm = np.asarray(pcm)
    n = pcm.shape[0]
    fs = np.broadcast_to(np.asarray(fs), (n,))
    lengths = np.broadcast_to(np.asarray(pcm.shape[1] if lengths is None else lengths), (n,))
    o = opts(**kw)
    p = o["order"]
    plans = []
    for i in range(n):
        fr = frames_of(int(fs[i]), int(lengths[i]), o)
        if fr is None:
            raise ValueError("row %d refused" % i)
        plans.append(fr)
    nfr = np.array([len(fr) for fr in plans], np.int32)
    fp = max(1, int(nfr.max()))
    res = dict(r0=np.full((n, fp), np.nan), err=np.full((n, fp), np.nan), start=np.full((n, fp), -1, np.int32),
               status=np.full((n, fp), -1, np.int32), n_frames=nfr, coefs=np.full((n, fp, p + 1), np.nan),
               counts=np.full((n, fp, 2), -1, np.int32), spans=[[[] for _ in fr] for fr in plans])
    where, phis, n_eqs = [], [], []
    for i in range(n):
        x = pcm[i, :int(lengths[i])]                                       # the row as a slice: nothing else to read
        spans = accepted_spans(x, glottal[i], cycles[i], o)
        for j, (s, L) in enumerate(plans[i]):
            got, n_eq = pooled(spans, s, L, p)
            res["spans"][i][j] = got
            res["start"][i, j] = s
            res["counts"][i, j] = (len(got), n_eq)
            where.append((i, j))
            phis.append(phi_direct(x, got, p))
            n_eqs.append(n_eq)
    r0, err, status, a = finish_batch(phis, n_eqs, o)
    for f, (i, j) in enumerate(where):
        res["r0"][i, j], res["err"][i, j], res["status"][i, j], res["coefs"][i, j] = r0[f], err[f], status[f], a[f]
    return res


def first_pass(pcm, fs, f0_min=50.0, f0_max=500.0, polarity=1, first_de_emphasis=0.99, scale=1.0, level_open=26,
               level_mid=128, cycles_pitch=None, iaif=None):
    """the chain in front of the estimate, on the restatements: IAIF sets at their defaults (iaif: other iaif_ref.opts
    keywords), the inverse in hold mode, the measurement, the glottal parameters.  Returns a dict: residual, inv_stat,
    meas, marks, glottal, cycles, iaif (the analysis)"""
    pcm = np.asarray(pcm, dtype=np.int16)
    n, ns = pcm.shape
    io = ia.opts(**(iaif or {}))
    sets = ia.analyse(pcm, fs, **(iaif or {}))
    L, H, starts = lr.frame_plan(int(fs), ns, ia.lpc_opts(io))
    n_sets, hop, offset, length = ir.from_lpc(L, H, 0, len(starts), ns, ir.HOLD)[:4]
    rows = ir.rows_of(n, n_sets, hop, offset, ns, scale, first_de_emphasis)
    residual, inv_stat = ir.inverse_filter(pcm, sets["coefs"], rows, ir.HOLD)
    marks_pitch = ns // 2 + 2
    cp = marks_pitch if cycles_pitch is None else cycles_pitch
    meas, marks, rec, cyc = gl.measure_and_glottal(residual, fs, level_open, level_mid, polarity, f0_min, f0_max, None,
                                                   marks_pitch, cp)
    return dict(residual=residual, inv_stat=inv_stat, meas=meas, marks=marks, glottal=rec, cycles=cyc, iaif=sets)


def closed_phase(pcm, fs, de_emphasis=0.0, scale=1.0, **kw):
    """Engine.closed_phase on the restatements (one rate for all rows, whole rows): the first pass, the estimate
    (window_s == 0), the inverse with one set per row.  kw: first_pass()'s and opts()'s keywords.  Returns first_pass()'s
    dict and flow, flow_stat, sets (analyse()'s dict)"""
    fkeys = ("f0_min", "f0_max", "polarity", "first_de_emphasis", "level_open", "level_mid", "cycles_pitch", "iaif")
    fkw = {k: kw.pop(k) for k in fkeys if k in kw}
    p = opts(**kw)["order"]                                                # the first pass at the estimate's order
    fkw["iaif"] = dict(dict(glottal_order=min(4, p)), **dict(fkw.get("iaif") or {}, order=p))
    pcm = np.asarray(pcm, dtype=np.int16)
    n, ns = pcm.shape
    out = first_pass(pcm, fs, scale=scale, **fkw)
    sets = analyse(pcm, fs, out["glottal"], out["cycles"], **kw)
    if opts(**kw)["window_s"] == 0:
        rows = ir.rows_of(n, 1, 1, 0, ns, scale, de_emphasis)
    else:
        L, H, starts = lr.frame_plan(int(fs), ns, lpc_opts(opts(**kw)))
        n_sets, hop, offset, length = ir.from_lpc(L, H, 0, len(starts), ns, ir.HOLD)[:4]
        rows = ir.rows_of(n, n_sets, hop, offset, ns, scale, de_emphasis)
    flow, stat = ir.inverse_filter(pcm, sets["coefs"], rows, ir.HOLD)
    out.update(flow=flow, flow_stat=stat, sets=sets)
    return out


COLUMNS = ("file", "sets", "unusable", "clipped", "spans", "equations", "err_over_r0", "status")


def format_line(name, stat, counts, r0, err, status):
    """the line of the `vclosed` program for one file: counts [sets][2], r0, err and status [sets] of its sets, stat the
    record of the inverse that wrote the flow.  Spans and equations are summed over the sets, err / r0 is the largest of
    the sets that have one, the status the OR of theirs (the C program prints with these printf formats)"""
    q = [float(e) / float(r) for r, e in zip(np.atleast_1d(r0), np.atleast_1d(err)) if r != 0 and not math.isnan(e)]
    counts = np.atleast_2d(counts)
    return "%s %d %d %d %d %d %s %d" % (name, len(counts), int(stat["n_unusable"]), int(stat["n_clipped"]),
                                        int(counts[:, 0].sum()), int(counts[:, 1].sum()), "%.3e" % max(q) if q else "nan",
                                        int(np.bitwise_or.reduce(np.atleast_1d(status).astype(np.int64))))


def format_set(A):
    """a line of `vclosed -c`"""
    return "# set " + " ".join("%.17g" % v for v in A)
