"""Restatement of the source track (include/voice_synth.h, "source track") in Python: the walk over the frames, the
rescaling of the two recursions, the reference's cycle (flowgen_shimmer.c:248-411 as oracle/vs_oracle.c:136-208 restates
it) with P and A0 in the places of P and par.amp, and the cap on the rejection loops.  Scalars are np.float32 where the
reference's are float and Python floats where they are double; the flanks and the noise of a cycle are numpy arrays whose
elements take the same roundings one by one; the two power sums are np.add.accumulate in float32, which adds in index
order.  The cos values are math.cos (the host's libm, like vs_cos_row); the draws come from pyoracle.draw.
TEST INFRASTRUCTURE: nothing here is loaded by the product."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyoracle  # noqa: E402

F32 = np.float32
RAND_MAX = 2147483647
PI = 4.0 * math.atan(1.0)
AC_MAX_LAG = 2048
ST_NO_VOICED = 0x1
ST_INTERNAL = 0x2
FLAG_JITTER, FLAG_SHIMMER, FLAG_NOISE = 0x1, 0x2, 0x4

ROW_DTYPE = np.dtype([(n, "<i4") for n in ("n_frames", "hop", "offset", "length", "pmin", "pmax")])
STAT_DTYPE = np.dtype([("status", "<i4"), ("n_cycles", "<i4"), ("n_resets", "<i4"), ("n_unvoiced", "<i4"),
                       ("n_draws", "<u8")])
CYCLE_DTYPE = np.dtype([("start", "<i4"), ("T", "<i4"), ("frame", "<i4"), ("amp", "<i4"), ("S", "<f4"), ("x_pow", "<f4"),
                        ("w_pow", "<f4"), ("reserved_", "<i4")])

_cos_rows = {}


def cos_row(T2):
    """cos(PI*k/T2), k < T2, with the reference's PI (vs_cos_row)"""
    if T2 not in _cos_rows:
        _cos_rows[T2] = np.array([math.cos(PI * k / T2) for k in range(T2)], dtype=np.float64)
    return _cos_rows[T2]


def short_of(v):
    """(signed short) of a double as gcc/x86-64 converts it: through int32, the low 16 bits"""
    return ((int(v) + 32768) & 0xFFFF) - 32768


def shorts_of(v):
    """short_of() of every element of a float64 array of integers"""
    return ((v.astype(np.int64) + 32768) & 0xFFFF) - 32768


def t2_of(cq, P):
    return int(math.ceil(0.5 * float(cq) * P))


def row(n_frames, hop, offset=0, length=0, pmin=2, pmax=AC_MAX_LAG):
    r = np.zeros((), dtype=ROW_DTYPE)
    r["n_frames"], r["hop"], r["offset"], r["length"], r["pmin"], r["pmax"] = n_frames, hop, offset, length, pmin, pmax
    return r


def check_row(lane, r, n_samples, frames_pitch):
    """the VS_ERR_RANGE cases of a row: ValueError"""
    if not 1 <= int(r["n_frames"]) <= frames_pitch or int(r["hop"]) < 1 or not 0 <= int(r["length"]) <= n_samples:
        raise ValueError("row")
    if int(r["pmin"]) < 2 or int(r["pmax"]) > AC_MAX_LAG or int(r["pmin"]) > int(r["pmax"]):
        raise ValueError("period range")
    if t2_of(lane.cq, int(r["pmin"])) < 1:
        raise ValueError("T2(pmin)")


def frame_of(n, offset, hop, n_frames):
    """1: f(n)"""
    return 0 if n < offset else min((n - offset) // hop, n_frames - 1)


def source_track_one(lane, n_samples, r, period, amp=None, max_reject=256, out=None):
    """one row.  period (and amp) int [>= n_frames].  Returns (flow int16 [n_samples] -- `out`, or zeros, with the row's
    first `length` samples written --, stat (a STAT_DTYPE record), cycles (CYCLE_DTYPE [n_cycles]))"""
    period = [int(p) for p in period]
    amp = None if amp is None else [int(a) for a in amp]
    check_row(lane, r, n_samples, len(period))
    F, hop, offset, length = int(r["n_frames"]), int(r["hop"]), int(r["offset"]), int(r["length"])
    pmin, pmax = int(r["pmin"]), int(r["pmax"])
    flow = np.zeros(n_samples, dtype=np.int16) if out is None else np.array(out, dtype=np.int16)
    jitter, shimmer, K, Kvar = float(lane.jitter), float(lane.shimmer), float(lane.K), F32(lane.Kvar)
    DC, noise, cq, seed = F32(lane.DC), F32(lane.noise), float(lane.cq), int(lane.seed)
    jit = bool(lane.flags & FLAG_JITTER) and jitter != 0.0
    shim = bool(lane.flags & FLAG_SHIMMER) and shimmer != 0.0
    noisy = bool(lane.flags & FLAG_NOISE)
    dcs = short_of(int(float(DC)))

    def voiced(f):
        return pmin <= period[f] <= pmax and (amp is None or 0 <= amp[f] <= 32766)

    d = 0          # index of the next draw
    dp0 = ds0 = F32(0.0)
    T4 = g = 0
    prev = None    # (P, A0) of the cycle before
    status = n_resets = n_unvoiced = 0
    cycles = []
    with np.errstate(all="ignore"):
        while g < length:
            f = frame_of(g, offset, hop, F)
            if not voiced(f):
                f2 = next((k for k in range(f + 1, F) if voiced(k)), None)
                e = length if f2 is None else min(offset + f2 * hop, length)
                assert e > g
                flow[g:e] = dcs
                n_unvoiced += e - g
                g = e
                dp0 = ds0 = F32(0.0)
                T4 = 0
                prev = None
                continue
            P = period[f]
            A0 = int(lane.amp) if amp is None else amp[f]
            if prev is not None:
                if P != prev[0]:
                    dp0 = F32(float(dp0) * float(P) / float(prev[0]))
                    T4 = 0
                if A0 != prev[1]:
                    ds0 = F32(float(ds0) * float(A0) / float(prev[1])) if prev[1] else F32(0.0)
            # jitter, fg:248-291
            T = P
            if jit:
                dp1, rej = dp0, 0
                while True:
                    J = F32((pyoracle.draw(seed, d) / (RAND_MAX * 10000.0)) * 40000.0 * jitter - 2.0 * jitter)
                    d += 1
                    Jd = float(J)
                    dp0 = F32(float(dp1) * (2.0 + Jd) / (2.0 - Jd) + 2.0 * P * Jd / (2.0 - Jd))
                    T = short_of(math.ceil(float(F32(P) + dp0)))
                    if not (F32(T) > F32(1.2) * F32(P) or F32(T) < F32(0.8) * F32(P)):
                        break
                    rej += 1
                    if rej >= max_reject:
                        T, dp0 = P, F32(0.0)
                        n_resets += 1
                        break
            # shimmer, fg:293-313
            Amplitude, S = F32(A0), F32(0.0)
            if shim:
                ds1, rej = ds0, 0
                while True:
                    epsilon = F32(pyoracle.draw(seed, d)) / F32(2147483648.0)
                    d += 1
                    S = F32(float(epsilon) * 4.0 * shimmer - 2.0 * shimmer)
                    Sd = float(S)
                    ds0 = F32(float(ds1) * (2.0 + Sd) / (2.0 - Sd) + 2.0 * A0 * Sd / (2.0 - Sd))
                    Amplitude = F32(A0) + ds0
                    if not (Amplitude > F32(1.8) * F32(A0) or Amplitude < F32(0.2) * F32(A0)):
                        break
                    rej += 1
                    if rej >= max_reject:
                        Amplitude, ds0 = F32(A0), F32(0.0)
                        n_resets += 1
                        break
            # glottal flow, fg:317-336
            T2 = t2_of(cq, P)
            assert T2 >= 1 and T >= 1
            cosv = cos_row(T2)
            Ad = float(Amplitude)
            x = np.zeros(max(T, 2 * T2) + 1, dtype=np.int64)
            rise = shorts_of(np.ceil((Ad * 0.5) * (1.0 - cosv)))
            lt = rise.astype(np.float32) < DC
            rise[lt] = dcs
            if lt.any():
                T4 = int(np.nonzero(lt)[0][-1])
            x[:T2] = rise
            Knew = F32(K * (1.0 + float(F32(2.0) * Kvar) * ((pyoracle.draw(seed, d) / float(RAND_MAX)) - 0.5)))
            d += 1
            Kd = float(Knew)
            fall = shorts_of(np.ceil(Ad * ((Kd * cosv - Kd) + 1.0)))
            below = np.nonzero(fall.astype(np.float32) < DC)[0]
            T3 = T2 + int(below[0]) if len(below) else 2 * T2
            x[T2:T3] = fall[:T3 - T2]
            x[T3:] = 0
            if T > T3:
                x[T3:T] = dcs
            # closed-phase noise, fg:373-411
            x_pow = w_pow = F32(0.0)
            if noisy:
                sq = x[T4:T3].astype(np.float32)
                sq = sq * sq
                aux = np.add.accumulate(sq, dtype=np.float32)[-1] if len(sq) else F32(0.0)
                x_pow = aux / (F32(T3) - F32(T4))
                aux = F32(1.0 + float((F32(T3) - F32(T4)) / F32(T)))
                arg = float(F32(12.0) * aux * x_pow / noise)
                NDW = math.isqrt(int(arg)) if math.isfinite(arg) and arg > 0.0 else 0   # the floor of the root; NaN, -0: 0
                idx = np.concatenate([np.arange(0, T4), np.arange(T3, max(T, T3))]).astype(np.int64)
                m = len(idx)
                u = np.array([pyoracle.draw(seed, d + q) for q in range(m)], dtype=np.float64) / float(RAND_MAX)
                d += m
                w = shorts_of(np.ceil(u * float(NDW) - float(NDW) / 2.0))
                x[idx] = np.clip(x[idx] + w, -32767, 32767)
                wf = w.astype(np.float32)
                wf = wf * wf
                w_pow = (np.add.accumulate(wf, dtype=np.float32)[-1] if m else F32(0.0)) / F32(T)
            cycles.append((g, T, f, A0, S if shim else F32(0.0), x_pow, w_pow, 0))
            k = min(T, length - g)
            flow[g:g + k] = x[:k].astype(np.int16)
            g += T
            prev = (P, A0)
    stat = np.zeros((), dtype=STAT_DTYPE)
    stat["status"] = status | (0 if cycles else ST_NO_VOICED)
    stat["n_cycles"], stat["n_resets"], stat["n_unvoiced"], stat["n_draws"] = len(cycles), n_resets, n_unvoiced, d
    return flow, stat, np.array(cycles, dtype=CYCLE_DTYPE)


def source_track(lanes, n_samples, rows, period, amp=None, max_reject=256, out=None, log_cycles=0):
    """rows of a call: period (amp) int [n][frames_pitch].  Returns (flow [n][n_samples], stat [n], cycles
    [n][log_cycles] with start -1 past a row's cycles -- or None --, and the full logs as a list)"""
    n = len(lanes)
    flow = np.zeros((n, n_samples), dtype=np.int16) if out is None else np.array(out, dtype=np.int16)
    stat = np.zeros(n, dtype=STAT_DTYPE)
    cyc = None
    if log_cycles:
        cyc = np.zeros((n, log_cycles), dtype=CYCLE_DTYPE)
        cyc["start"] = -1
    logs = []
    for i in range(n):
        flow[i], stat[i], log = source_track_one(lanes[i], n_samples, rows[i], period[i], None if amp is None else amp[i],
                                                 max_reject, flow[i])
        logs.append(log)
        if log_cycles:
            k = min(len(log), log_cycles)
            cyc[i, :k] = log[:k]
    return flow, stat, cyc, logs


def row_from_pitch(fs, length, f0_min=50.0, f0_max=500.0, hop_s=0.010):
    """vs_strack_from_pitch: the f(n) of the guided marks"""
    import acoustic_ref as ar
    import pitch_ref as pt
    tmin, tmax = ar.lag_bounds(fs, f0_min, f0_max)
    H = pt.hop(fs, hop_s)
    nf = pt.frame_count(length, tmax, H)
    if nf < 1:
        raise ValueError("no frames")
    return row(nf, H, tmax + tmax // 2 - H // 2, length, tmin, tmax)


# the lanes of the constant-track consequence (flowgen_shimmer's options): six plain ones, one whose samples wrap
# (-a 30000 -s 10) and one with noise on a zero DC flow
CONSTANT_LANES = (
    [],
    ["-j", "2"],
    ["-s", "5.76"],
    ["-j", "1", "-s", "5", "-n", "20", "-r", "16000"],
    ["-z", "0.3", "-l", "0.1"],
    ["-j", "10", "-s", "10", "-n", "10", "-z", "1", "-a", "32000", "-f", "77.3", "-r", "44100"],
    ["-a", "30000", "-s", "10"],
    ["-l", "0", "-n", "20"],
)


def constant_period(lane):
    """P = (int)((float)fs / F0), flowgen_shimmer.c:244"""
    return int(F32(lane.fs) / F32(lane.F0))
