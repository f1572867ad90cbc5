"""One deterministic bank of signals a measurement tool meets on recordings and this project never synthesises: noise,
silence, DC, full-scale square waves and alternations, tones outside the F0 bounds, chirps, impulse trains, ramps.

Test infrastructure only (a plain module, imported by the CPU test of the restatements and by the GPU tests).  Every row
is int16 [n], clipped and rounded, and everything random comes from numpy.random.default_rng(seed).

For the coefficient tracks: track_models() (the bank and four rows with silent stretches, as models for vs_lpc),
reflection_sets() (stable sets that drive the filter far past int16 and int32) and scaled_radius()."""
import collections

import numpy as np

import track_ref as tr

# the four (fs, n, f0_min, f0_max) cases of the acoustic tests: each takes other paths of the period kernel
#   16 kHz: 2 <= S <= 3 k segments;  44.1 kHz at 30..800 Hz and 96 kHz at 47..500 Hz: more than 256 lag groups (two
#   passes of the group loop), the latter with more than 48 KB of LDS;  8 kHz at 200..2000 Hz: 10 groups, S = 25
ACOUSTIC_CASES = ((16000, 8000, 50.0, 500.0), (44100, 12000, 30.0, 800.0), (96000, 20000, 47.0, 500.0),
                  (8000, 3000, 200.0, 2000.0))

# rows whose status does not depend on the case (tests/test_hostile_signals_ref.py holds the restatement to these)
UNVOICED_ROWS = ("zeros",)
ZERO_AMPLITUDE_ROWS = ("constant", "constant_min", "chirp")
NOISE_ROWS = ("noise_full", "noise_small", "sine_150_noise")        # A(z) as well-conditioned as a vowel's
CROWDED_ROWS = ("constant", "constant_min", "sine_30", "sine_1500")  # constants and pure tones: roots near |z| = 1


def _int16(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def _jump_train(n, P, num, den):
    """single-sample pulses of +30000 every P samples and of -30000 half-way between them, and one more pulse of either
    sign num/den of P (0.7 or so) behind the first of its sign: under both polarities the second mark lies that far
    behind the first, the window of the third begins inside the stretch already walked, and the marks kernel has to
    walk it again.  (F0 300..333 Hz keeps 2/3 P above the shortest lag and 3/2 P below the longest in all four cases.)"""
    x = np.zeros(n)
    x[3::P] = 30000.0
    x[3 + P // 2::P] = -30000.0
    x[3 + (num * P) // den] = 30000.0
    x[3 + P // 2 + (num * P) // den] = -30000.0
    return _int16(x)


def bank(fs, n, seed=0):
    """ordered dict name -> int16 [n]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    b = collections.OrderedDict()
    b["noise_full"] = rng.integers(-32768, 32768, size=n).astype(np.int16)
    b["noise_small"] = rng.integers(-3, 4, size=n).astype(np.int16)
    b["zeros"] = np.zeros(n, dtype=np.int16)
    b["constant"] = np.full(n, 12345, dtype=np.int16)
    b["constant_min"] = np.full(n, -32768, dtype=np.int16)
    b["square_200"] = _int16(np.where(np.floor(2.0 * 200.0 * t) % 2 == 0, 32767.0, -32768.0))
    b["chirp"] = _int16(30000.0 * np.sin(2 * np.pi * (80.0 * t + 0.5 * (400.0 - 80.0) / (n / fs) * t * t)))
    b["am_sine_120"] = _int16(20000.0 * (1.0 + 0.5 * np.sin(2 * np.pi * 7.0 * t)) * np.sin(2 * np.pi * 120.0 * t))
    b["sine_30"] = _int16(30000.0 * np.sin(2 * np.pi * 30.0 * t))
    b["sine_1500"] = _int16(30000.0 * np.sin(2 * np.pi * 1500.0 * t))
    imp = np.zeros(n)
    imp[np.rint(np.arange(0.0, n / fs, 1.0 / 110.0) * fs).astype(np.int64).clip(0, n - 1)] = 32767.0
    b["impulses_110"] = _int16(imp)
    b["alternating"] = _int16(np.where(np.arange(n) % 2 == 0, 32767.0, -32768.0))
    b["ramp"] = _int16(np.linspace(-32768.0, 32767.0, n))
    b["sine_150_noise"] = _int16(12000.0 * np.sin(2 * np.pi * 150.0 * t) + rng.normal(0.0, 9000.0, size=n))
    b["two_tones"] = _int16(15000.0 * np.sin(2 * np.pi * 100.0 * t) + 15000.0 * np.sin(2 * np.pi * 200.0 * t))
    b["jump_300"] = _jump_train(n, int(round(fs / 300.0)), 7, 10)
    b["jump_320"] = _jump_train(n, int(round(fs / 320.0)), 3, 4)
    return b


def matrix(b):
    """(names, int16 [rows][n]) of a bank, in its order"""
    return list(b), np.stack(list(b.values()))


def track_models(fs, n, seed=0):
    """ordered dict name -> int16 [n]: the bank and four composite rows -- noise then zeros, zeros then noise, noise
    zeros noise, a constant then zeros -- whose silent stretches (a third of the row or more) give vs_lpc NaN frames
    at the end, at the start and in the middle of a row wherever an analysis window fits into n / 3 samples.  The bank's
    own draws are untouched: the composites draw from a generator of their own."""
    b = bank(fs, n, seed)
    rng = np.random.default_rng([seed, 1])
    noise = rng.integers(-32768, 32768, size=n).astype(np.int16)
    h, t = n // 2, n // 3
    b["noise_zeros"] = np.where(np.arange(n) < h, noise, 0).astype(np.int16)
    b["zeros_noise"] = np.where(np.arange(n) < h, 0, noise).astype(np.int16)
    b["noise_zeros_noise"] = np.where((np.arange(n) >= t) & (np.arange(n) < n - t), 0, noise).astype(np.int16)
    b["constant_zeros"] = np.where(np.arange(n) < h, 12345, 0).astype(np.int16)
    return b


def reflection_sets(rng, rows, K, order):
    """[rows][K][order+1]: the step-up of reflection coefficients drawn in +-0.95, times a scale per set in [0.2, 1]:
    every set is stable (|k_i| < 1), and the large ones lie close enough to the unit circle that a full-scale flow
    takes |y| to 1e14 at order 40 (tests/test_track_ref.py measures it)"""
    k = rng.uniform(-0.95, 0.95, (rows, K, order)) * rng.uniform(0.2, 1.0, (rows, K, 1))
    return tr.step_up(k)


def scaled_radius(A, s):
    """A_j * s^j: the set whose roots are those of A, every radius times s"""
    A = np.asarray(A, dtype=np.float64)
    return A * float(s) ** np.arange(A.shape[-1])


def walk_again_marks(marks, p0, tmin, tmax):
    """marks k (after m_0) whose next window begins at or before the last sample walked for them, w1 = m_prev + hi: the
    marks kernel must walk [k, w1] again from the row in memory.  (marks: the full list m_0..m_K of cycle_marks)"""
    lo1, hi1 = max(tmin, (2 * p0 + 2) // 3), min(tmax, (3 * p0) // 2)
    d = (p0 + 3) // 4
    lo, hi = lo1, hi1
    count = 0
    for i in range(1, len(marks)):
        w1 = marks[i - 1] + hi
        T = marks[i] - marks[i - 1]
        lo, hi = max(lo1, T - d), min(hi1, T + d)
        if marks[i] + lo <= w1:
            count += 1
    return count
