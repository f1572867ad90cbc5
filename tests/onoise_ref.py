"""numpy restatement of the output-noise stage, "vowel -n" (vowel_new.c:302-324; include/voice_synth.h, "Output noise"):
the tests hold the CPU oracle to it, and the device to the oracle.

It takes FINISHED PCM rows (what the filter left, before the noise) and returns what the stage makes of them.  Every
product, sum and quotient is one numpy operation in the reference's precision: the frame's power is a sequential float32
sum of float32 squares, the width a float32 quotient whose root goes through double, noiseval and aux are rounded to
float32, and the sample is round2int() of a double sum.  The draws are Philox4x32-10 (voice_synth_amd/configs.py, pinned by
tests/test_philox.py) under the draw contract of oracle/philox.h: draw n of a row -- the row's sample n, the stage draws
once per sample in order -- is word n & 3 of the block with counter (n >> 2, 0, 0, 0) and key (seed_lo, seed_hi), shifted
right by one bit."""
import numpy as np

from voice_synth_amd.configs import philox4x32_10

RAND_MAX = 2147483647.0
SMALL_BOUND = 2.0 ** -13     # the kernel's bounds of the "plain" class of widths (csrc/vs_dev_onoise.h,
BIG_BOUND = 65534.0          # vs_onoise_width_is_plain): {0} and [2^-13, 65534)
QUIRK_BOUND = 2.0 ** -38     # an aux in (-2^-38, 0) is where round2int and the plain formula can part


def frame_length(fs):
    """Lframe of vowel_new.c:361-363"""
    return 50 * (int(int(fs) * 0.001 / 2.0) * 2)


def draws(seed, n):
    """draws 0..n-1 of the stream of `seed` (what random() returns, 0..2^31-1), int64 [n]"""
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    zero = np.zeros_like(blocks)
    seed = int(seed)
    w = philox4x32_10([blocks, zero, zero, zero], [np.full_like(blocks, seed & 0xFFFFFFFF), np.full_like(blocks, seed >> 32)])
    return (np.stack(w, axis=1).reshape(-1)[:n] >> np.uint64(1)).astype(np.int64)


def round2int(x):
    """round2int() of vowel_new.c:413-427 on an array of doubles"""
    x = np.asarray(x, dtype=np.float64)
    dec = x - np.floor(x)
    x = np.where(dec > 0.5, x + 1, x)
    x = np.minimum(np.maximum(x, -32767.0), 32767.0)
    return np.floor(x).astype(np.int64).astype(np.int16)


def frame_sum(frame, pairs=False):
    """aux of vowel_new.c:303-306 for one frame of every row (int16 [rows][ni]): float32, in sample order.  pairs=True is
    NOT the reference: the squares of two neighbours are added first -- what a case uses to show that the order counts."""
    f = frame.astype(np.float32)
    sq = f * f
    if pairs:
        even = sq[:, 0::2].copy()
        even[:, :sq.shape[1] // 2] += sq[:, 1::2]
        sq = even
    if sq.shape[1] == 0:
        return np.zeros(len(frame), dtype=np.float32)
    return np.add.accumulate(sq, axis=1, dtype=np.float32)[:, -1]


def widths(pcm, fs, out_snr, pairs=False):
    """NoiseDistWidth of every frame, float32 [rows][frames] (the last frame may be a partial one; rows whose out_snr is
    not > 0 carry zeros and are left alone by add_noise)"""
    pcm = np.asarray(pcm, dtype=np.int16)
    R, N = pcm.shape
    L = frame_length(fs)
    snr = np.broadcast_to(np.asarray(out_snr, dtype=np.float32), (R,))
    on = snr > 0
    frames = (N + L - 1) // L
    W = np.zeros((R, frames), dtype=np.float32)
    with np.errstate(all="ignore"):
        for fr in range(frames):
            seg = pcm[:, fr * L:min(N, (fr + 1) * L)]
            aux = frame_sum(seg, pairs)
            sig_power = aux / np.float32(seg.shape[1])
            q = (np.float32(12.0) * sig_power) / np.where(on, snr, np.float32(1.0))
            W[:, fr] = np.where(on, np.sqrt(q.astype(np.float64)).astype(np.float32), np.float32(0.0))
    return W


def width_class(w):
    """'zero', 'small', 'plain' or 'big' of a width (an array gives an array of str)"""
    w = np.asarray(w, dtype=np.float32)
    out = np.where(w == 0, "zero", np.where(w < SMALL_BOUND, "small", np.where(w < BIG_BOUND, "plain", "big")))
    return out if out.ndim else str(out)


def is_plain(w):
    c = width_class(w)
    return (c == "zero") | (c == "plain")


def plain_form(pcm, aux):
    """the one-instruction form of the kernel's plain class: clamp(y + ceil(aux - 0.5)) (aux - 0.5 is exact in double for
    every float aux that is not tiny, and a tiny one gives 0 either way)"""
    r = np.ceil(np.asarray(aux, dtype=np.float64) - 0.5)
    return np.clip(np.asarray(pcm, dtype=np.float64) + r, -32767.0, 32767.0).astype(np.int16)


def add_noise(pcm, fs, out_snr, out_seed, pairs=False):
    """(noisy int16 [rows][n], NoiseDistWidth float32 [rows][frames], aux float32 [rows][n]) of finished PCM int16
    [rows][n]; out_snr and out_seed a value per row or one for all.  Rows whose out_snr is not > 0 come back as they are
    (widths and aux zero)."""
    pcm = np.asarray(pcm, dtype=np.int16)
    R, N = pcm.shape
    L = frame_length(fs)
    snr = np.broadcast_to(np.asarray(out_snr, dtype=np.float32), (R,))
    seeds = np.broadcast_to(np.asarray(out_seed, dtype=np.uint64), (R,))
    if (snr > 0).any() and L <= 0:
        raise ValueError("fs < 2000: frames of no length")
    W = widths(pcm, fs, snr, pairs)
    r = np.stack([draws(s, N) for s in seeds]) if N else np.zeros((R, 0), dtype=np.int64)
    noiseval = (r.astype(np.float64) / RAND_MAX).astype(np.float32)
    wn = W[:, np.arange(N) // max(L, 1)] if N else np.zeros((R, 0), dtype=np.float32)
    with np.errstate(all="ignore"):
        aux = (wn.astype(np.float64) * (noiseval.astype(np.float64) - 0.5)).astype(np.float32)
        noisy = round2int(1.0 * pcm.astype(np.float64) + 1.0 * aux.astype(np.float64))
    on = (snr > 0)[:, None]
    return np.where(on, noisy, pcm).astype(np.int16), W, np.where(on, aux, np.float32(0.0)).astype(np.float32)
