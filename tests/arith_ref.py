"""numpy restatements of the synthesis filter's recurrence: the reference's own loop (exact_unrounded, any order) and
the two opt-in arithmetics of the synthesis kernels (include/voice_synth.h, "the arithmetics of the 22-tap filter";
csrc/vs_dev_filter.h; with P = 40 the wide kernel of csrc/vs_filter_wide.hip): the tests hold the device to them byte for
byte.  Every form also gives its state y, and first_nonfinite() the sample at which a row's state leaves the finite
numbers: what is promised of a lane ends there (include/voice_synth.h).

Vectorised over rows, a Python loop over samples, in the style of tests/track_ref.py.  filter_fma() is the header's FMA
form with libm's fma() on doubles (tests/test_track_ref.py holds that fma to exact rational arithmetic) behind one of the
three roundings the kernels use; filter_f32() is the packed single-precision form, every product and sum one float32
operation, with a float32 fma made of double operations (tests/test_arith_ref.py holds it to exact rational arithmetic)."""
import numpy as np

import track_ref as tr

ORDER = 22
WIDE_ORDER = 40              # the taps of the wide kernel's FMA form
ROUNDINGS = ("round2int", "nearest_even", "half_up")
F32_MIN_NORMAL = 2.0 ** -126


# ---- the three roundings ---------------------------------------------------------------------------------------------

def nearest_even(x):
    """rint (ties to even), then the clamp to +-32767; NaN gives 0 (the saturating conversion)"""
    x = np.asarray(x, dtype=np.float64)
    r = np.rint(np.where(np.isnan(x), 0.0, x))
    return np.minimum(np.maximum(r, -32767.0), 32767.0).astype(np.int64).astype(np.int16)


def half_up(x):
    """floor(x + 0.5) with the sum taken exactly, then the clamp to +-32767; NaN gives 0"""
    x = np.asarray(x, dtype=np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    f = np.floor(x)
    with np.errstate(invalid="ignore"):
        r = np.where(x - f >= 0.5, f + 1.0, f)         # x - floor(x) is exact in double
    return np.minimum(np.maximum(r, -32767.0), 32767.0).astype(np.int64).astype(np.int16)


def rounded(o, rounding):
    """o (doubles, the arguments of the kernels' rounding) -> int16"""
    return {"round2int": tr.round2int, "nearest_even": nearest_even, "half_up": half_up}[rounding](o)


# ---- the FMA form ----------------------------------------------------------------------------------------------------

def fma_state(flow, A, gain, pre, P=ORDER):
    """(o, y), doubles [rows][samples]: the argument of the rounding and the state in the header's FMA form over P taps
    (22: the fused kernels; 40: the wide kernel).  flow int16 [rows][samples], A [rows][P+1] doubles (A[:, 0] ignored,
    zeros above a lane's order), gain and pre the lanes' float values, one per row."""
    assert P in (ORDER, WIDE_ORDER)
    flow = np.asarray(flow, dtype=np.int16)
    A = np.asarray(A, dtype=np.float64)
    R, N = flow.shape
    assert A.shape == (R, P + 1)
    gain = np.broadcast_to(np.asarray(gain, dtype=np.float32).astype(np.float64), (R,))
    pre = np.broadcast_to(np.asarray(pre, dtype=np.float32).astype(np.float64), (R,))
    na = np.ascontiguousarray(-A.T)                    # na[j] = -a_j
    p = P
    Y = np.zeros((N + p, R), dtype=np.float64)         # y[n] at Y[n + p]
    O = np.zeros((N, R), dtype=np.float64)
    x = flow.T.astype(np.float64)
    with np.errstate(all="ignore"):
        for n in range(N):
            acc = x[n] * gain
            p0, p1 = acc, -(A[:, 2] * Y[n + p - 2])
            for j in range(3, p + 1):
                if j & 1:
                    p0 = tr.fma(na[j], Y[n + p - j], p0)
                else:
                    p1 = tr.fma(na[j], Y[n + p - j], p1)
            acc = tr.fma(na[1], Y[n + p - 1], p0 + p1)
            O[n] = tr.fma(-pre, Y[n + p - 1], acc)
            Y[n + p] = acc
    return np.ascontiguousarray(O.T), np.ascontiguousarray(Y[p:].T)


def fma_unrounded(flow, A, gain, pre, P=ORDER):
    """o of fma_state()"""
    return fma_state(flow, A, gain, pre, P)[0]


def filter_fma(flow, A, gain, pre, rounding, P=ORDER):
    """int16 [rows][samples]: the FMA form over P taps behind one of ROUNDINGS"""
    return rounded(fma_unrounded(flow, A, gain, pre, P), rounding)


# ---- the reference's loop --------------------------------------------------------------------------------------------

def exact_unrounded(flow, A, gain, pre, order):
    """(o, y), doubles [rows][samples]: vowel_new.c:266-289 literally, each row with its own Order = order[row] (1..40):
    y_double[0] = 0.0 + B[0]*x[i]*gain (B = {1, 0, ..}: the further terms add 0.0*x*gain = +-0.0, which changes no
    value); for j = 1..Order: y_double[0] = y_double[0] - A[j]*y_double[j], every product and difference rounded on
    its own; o = y_double[0] - pre_emphasis*y_double[1], the argument of round2int.  The loop runs over exactly Order
    taps, as the reference's does: a row of lower order skips the later ones, it does not multiply by zero (which it
    would turn a state of +-inf into NaN by).  A [rows][>= max(order)+1]; what lies above a row's order is not read."""
    flow = np.asarray(flow, dtype=np.int16)
    A = np.asarray(A, dtype=np.float64)
    R, N = flow.shape
    order = np.broadcast_to(np.asarray(order, dtype=np.int64), (R,))
    assert (order >= 1).all() and A.shape[0] == R and A.shape[1] > order.max()
    gain = np.broadcast_to(np.asarray(gain, dtype=np.float32).astype(np.float64), (R,))
    pre = np.broadcast_to(np.asarray(pre, dtype=np.float32).astype(np.float64), (R,))
    p = int(order.max())
    aT = np.ascontiguousarray(A.T)
    runs = [order >= j for j in range(p + 1)]          # runs[j]: the rows whose loop reaches tap j
    Y = np.zeros((N + p, R), dtype=np.float64)         # y[n] at Y[n + p]
    O = np.zeros((N, R), dtype=np.float64)
    x = flow.T.astype(np.float64)
    with np.errstate(all="ignore"):
        for n in range(N):
            acc = 0.0 + 1.0 * x[n] * gain
            for j in range(1, p + 1):
                acc = np.where(runs[j], acc - aT[j] * Y[n + p - j], acc)
            O[n] = acc - pre * Y[n + p - 1]
            Y[n + p] = acc
    return np.ascontiguousarray(O.T), np.ascontiguousarray(Y[p:].T)


def first_nonfinite(y):
    """per row of a state y [rows][samples]: the first n at which y[n] is not finite, or the number of samples"""
    bad = ~np.isfinite(np.asarray(y))
    return np.where(bad.any(axis=1), bad.argmax(axis=1), bad.shape[1]).astype(np.int64)


# ---- the single-precision form ---------------------------------------------------------------------------------------

def _f32(x):
    """a double array rounded to float32, kept in doubles"""
    return x.astype(np.float32).astype(np.float64)


def fmaf(a, b, c):
    """a*b + c rounded once to float32, elementwise; a, b, c: doubles that hold float32 values, and so is the result.
    The product of two float32 is exact in double; TwoSum gives the error of the double sum; where that is non-zero
    the sum is forced odd (round to odd), after which the rounding to float32 -- 29 bits shorter -- is the rounding of
    the exact value.  Operands that are not finite give what the double operations give: +-inf or NaN."""
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = np.ascontiguousarray(s).view(np.int64)
    fix = np.isfinite(s) & (e != 0.0) & ((bits & 1) == 0)   # (s not finite: an operand was not, or the result passes
    #                                                          float32 by far -- a*b + c in double says which of inf, NaN)
    # the neighbour on e's side: one up in magnitude where e has the sign of s, one down where not
    step = np.where((e > 0.0) == (s > 0.0), 1, -1)
    s = np.where(fix, bits + step, bits).view(np.float64)
    return _f32(s)


class _Smallest:
    """per row, the smallest non-zero finite |value| among the float32 results it is shown ([.., rows] arrays), and
    whether one of them was not finite"""

    def __init__(self, rows):
        self.rows = np.full(rows, np.inf)
        self.nonfinite = np.zeros(rows, dtype=bool)

    def see(self, *arrays):
        for a in arrays:
            m = np.abs(a).reshape(-1, len(self.rows))
            fin = np.isfinite(m)
            self.nonfinite |= ~fin.all(axis=0)
            self.rows = np.minimum(self.rows, np.where((m == 0.0) | ~fin, np.inf, m).min(axis=0))

    @property
    def value(self):
        """the smallest non-zero |value| of all rows; 0 once one of them is not finite"""
        return 0.0 if self.nonfinite.any() else float(self.rows.min(initial=np.inf))


def f32_state(flow, A, gain, pre):
    """(o, y, smallest): the packed single-precision form of csrc/vs_dev_filter.h, vs_superstep_f32.
    Samples come in pairs n (even), n + 1; four chains of fused multiply-adds per pair, the two of the even sample over
    the tap pairs {A[2k+2], A[2k+1]}, the two of the odd sample over {A[2k+3], A[2k+2]}, its newest and its oldest tap on
    their own.  smallest: the smallest non-zero |intermediate| seen -- above 2^-126 no result depends on how the
    kernels treat denormals -- and 0 if an intermediate was not finite.  o, y: the argument of the rounding and the
    state, float32 values in doubles [rows][samples]; smallest: the _Smallest that saw every intermediate (.value: of
    the whole batch as above; .rows: per row, over the finite intermediates)."""
    flow = np.asarray(flow, dtype=np.int16)
    A = np.asarray(A, dtype=np.float64)
    R, N = flow.shape
    assert A.shape == (R, ORDER + 1)
    nA = -_f32(A.T)                                    # nA[j] = -(float)A[j]
    g = np.broadcast_to(_f32(np.asarray(gain, dtype=np.float64)), (R,))
    npre = -np.broadcast_to(_f32(np.asarray(pre, dtype=np.float64)), (R,))
    # the four chains side by side: [pex, pey, pox, poy]; step k multiplies tap T[k][c] with y[n - D[k][c]]
    T = np.zeros((11, 4, R))
    D = np.zeros((11, 4), dtype=np.int64)
    for k in range(10):
        T[k] = nA[2 * k + 2], nA[2 * k + 1], nA[2 * k + 3], nA[2 * k + 2]
        D[k] = 2 + 2 * k, 1 + 2 * k, 2 + 2 * k, 1 + 2 * k
    T[10, :2] = nA[22], nA[21]                         # the even sample's eleventh pair
    D[10, :2] = 22, 21
    p = ORDER + 2
    M = N + (N & 1)                                    # an odd length: the last pair's second sample is not kept
    Y = np.zeros((M + p, R))                           # y[n] at Y[n + p]
    O = np.zeros((M, R))
    x = np.zeros((M, R))
    x[:N] = flow.T
    small = _Smallest(R)
    with np.errstate(all="ignore"):
        for n in range(0, M, 2):
            W = Y[n + p - 22:n + p][::-1]              # W[d - 1] = y[n - d]
            c = _f32(T[0] * W[D[0] - 1])
            small.see(c)
            for k in range(1, 10):
                c = fmaf(T[k], W[D[k] - 1], c)
                small.see(c)
            pe = fmaf(T[10, :2], W[D[10, :2] - 1], c[:2])
            pox, poy = c[2], c[3]
            acc0 = fmaf(x[n], g, _f32(pe[0] + pe[1]))
            sc = fmaf(nA[22], W[20], poy)
            sc2 = fmaf(x[n + 1], g, _f32(sc + pox))
            acc1 = fmaf(nA[1], acc0, sc2)
            o0 = fmaf(npre, W[0], acc0)
            o1 = fmaf(npre, acc0, acc1)
            small.see(pe, acc0, sc, sc2, acc1, o0, o1, _f32(pe[0] + pe[1]), _f32(sc + pox))
            Y[n + p], Y[n + p + 1] = acc0, acc1
            O[n], O[n + 1] = o0, o1
    return np.ascontiguousarray(O[:N].T), np.ascontiguousarray(Y[p:p + N].T), small


def filter_f32(flow, A, gain, pre):
    """(int16 [rows][samples], smallest): f32_state() behind half-up; smallest: the smallest non-zero |intermediate| of
    the batch, 0 if one was not finite"""
    o, _, small = f32_state(flow, A, gain, pre)
    return half_up(o), small.value
