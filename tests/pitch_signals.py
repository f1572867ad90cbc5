"""The constructed signals of the pitch track's tests (tests/test_pitch_ref.py on the restatement, tests/test_gpu_pitch.py
on the device).  Test infrastructure only."""
import numpy as np


def pulse(width, amp):
    """one raised cosine of `width` samples"""
    k = np.arange(width)
    return amp * 0.5 * (1.0 - np.cos(2.0 * np.pi * k / width))


def train(periods, width_of, amp_of, tail=0):
    """a raised-cosine pulse train: cycle c has periods[c] samples, a pulse of width_of(P) and amplitude amp_of(c) at its
    start.  Returns (int16 signal, the peaks' positions)"""
    n = int(sum(periods)) + tail
    x = np.zeros(n)
    at, peaks = 0, []
    for c, P in enumerate(periods):
        w = int(width_of(P))
        x[at:at + w] += pulse(w, amp_of(c))
        peaks.append(at + w // 2)
        at += P
    return np.round(x).astype(np.int16), peaks


def glide():
    """16 kHz: width 0.6 P, amplitude 8000, periods from 220 down to 80 by a factor 0.99 per cycle, each rounded"""
    periods, P = [], 220.0
    while P >= 80.0:
        periods.append(int(round(P)))
        P *= 0.99
    x, peaks = train(periods, lambda p: int(0.6 * p), lambda c: 8000.0)
    return x, peaks, periods


def gaps(seed=5):
    """60 cycles of P = 123, 4000 zeros, 5000 samples of uniform noise +-3000, the 60 cycles again"""
    t, _ = train([123] * 60, lambda p: int(0.6 * p), lambda c: 8000.0)
    noise = np.random.default_rng(seed).integers(-3000, 3001, 5000).astype(np.int16)
    return np.concatenate([t, np.zeros(4000, np.int16), noise, t])


def octave_trap():
    """P = 160, width 0.4 P, 100 cycles, with an extra raised cosine of length 64 and amplitude 7900 at offset 80 of
    cycles 48..52: five frames' worth of a strong candidate at half the period"""
    x, _ = train([160] * 100, lambda p: int(0.4 * p), lambda c: 8000.0)
    y = x.astype(np.float64)
    for c in range(48, 53):
        y[c * 160 + 80:c * 160 + 144] += pulse(64, 7900.0)
    return np.round(y).astype(np.int16)


def subharmonic():
    """P = 100 with amplitudes alternating 8000 / 5600: the true period is 200"""
    x, _ = train([100] * 160, lambda p: int(0.6 * p), lambda c: 8000.0 if c % 2 == 0 else 5600.0)
    return x
