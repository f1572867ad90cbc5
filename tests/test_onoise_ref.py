"""The numpy restatement of the output-noise stage (tests/onoise_ref.py) on the CPU, and the cases of
tests/test_gpu_onoise.py.

The restatement is held to the oracle (pyoracle.filter, pyoracle.synth) byte for byte on every case; the device is then
held to the oracle on the same cases.  What the restatement adds is the view inside: the width of every frame, its class
under the kernel's bounds (zero, small, plain, big), the aux of every sample, and the kernel's one-instruction "plain"
form next to the literal one.  From those the conditions are asserted under which the GPU comparisons mean something --
which classes a case meets, that octets of eight samples have their two quads in frames of different classes both ways
round, that the small-width branch is observable, that the order of the float power sum counts, that the clamp is met on
both sides.  Every case prints one line (pytest -s).

The rows are put in front of the noise stage by "identity lanes": a custom set A = [1, 0] with gain 1 and pre-emphasis 0
filters x to clip(x, -32767, 32767)."""
import functools
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_signals as hs  # noqa: E402
import onoise_ref as on  # noqa: E402

BANK_ROWS = ("noise_full", "noise_small", "zeros", "constant_min", "square_200", "impulses_110", "alternating", "ramp")
ROW_NAMES = ("patchwork",) + BANK_ROWS
# out_snr as the ABI takes it (a power ratio): the program's -n 1 is 10^0.1; 3e37 makes 12*sig_power/snr a float32 denormal
SNRS = (1e-3, 10 ** 0.1, 100.0, 1e16, 1e20, 1e30, 3e37)
RATES = (22050, 11025, 16000)          # Lframe 1100 and 500 (= 4 mod 8: every other frame ends inside an octet), 800
SEED = 9
# the classes of the patchwork row's five frames at 22050 Hz (z = zero, s = small, p = plain, b = big)
PATCHWORK_CLASSES = {1e-3: "pbzpb", 10 ** 0.1: "pbzpp", 100.0: "ppzpp", 1e16: "spzsp", 1e20: "sszss", 1e30: "sszss"}
LETTER = {"zero": "z", "small": "s", "plain": "p", "big": "b"}


def patchwork(L):
    """five frames of length L (the last one a tail of five samples): small noise, full scale alternating, silence, a
    single 1, and a tail that starts at both clamps"""
    row = np.zeros(4 * L + 5, dtype=np.int16)
    row[:L] = np.random.default_rng(3).integers(-3, 4, L)
    row[L:2 * L] = np.where(np.arange(L) % 2 == 0, 32767, -32767)
    row[3 * L + 7] = 1
    row[4 * L:] = [32767, -32767, 0, 1, -1]
    return row


@functools.lru_cache(maxsize=None)
def rows_for(fs, n=None):
    """int16 [9][n]: the patchwork row and the bank's rows at 4*Lframe + 5 samples, cut or repeated to n"""
    L = on.frame_length(fs)
    base = 4 * L + 5
    bank = hs.bank(fs, base, seed=0)
    rows = np.stack([patchwork(L)] + [bank[k] for k in BANK_ROWS])
    if n is not None and n != base:
        rows = np.tile(rows, (1, (n + base - 1) // base))[:, :n]
    rows.setflags(write=False)
    return rows


def identity_lane(fs, out_snr, out_seed, order=1):
    lane = vs.default_lane()
    lane.fs = int(fs)
    lane.gain, lane.pre_emphasis = 1.0, 0.0
    vs.set_coefficients(lane, [1.0] + [0.0] * order)
    lane.out_snr = float(out_snr)
    lane.out_seed = int(out_seed)
    return lane


def lane_plan(n_lanes):
    """[(row index, out_snr, out_seed)] of n_lanes lanes: every third lane has out_snr 0; the others walk the 63 pairs of
    (row, out_snr) -- 9 and 7 have no common factor, so 94 lanes hold every pair.  Lane 0 is the patchwork row at the
    first out_snr with seed 9; the other seeds differ in both words of the key."""
    out = []
    k = 0
    for i in range(n_lanes):
        seed = SEED + i * 0x100000001
        if i % 3 == 2:
            out.append(((k + 4) % len(ROW_NAMES), 0.0, seed))
        else:
            out.append((k % len(ROW_NAMES), SNRS[k % len(SNRS)], seed))
            k += 1
    return out


class Case:
    """lanes, their input rows (flow), the oracle's answer (want) and the noiseless answer (quiet)"""

    def __init__(self, fs, n, n_lanes, order=1):
        self.fs, self.n, self.L = fs, n, on.frame_length(fs)
        self.plan = lane_plan(n_lanes)
        rows = rows_for(fs, n)
        self.flow = np.ascontiguousarray(rows[[p[0] for p in self.plan]])
        self.lanes = [identity_lane(fs, snr, seed, order) for _, snr, seed in self.plan]
        self.snr = np.array([l.out_snr for l in self.lanes], dtype=np.float32)
        self.seeds = np.array([p[2] for p in self.plan], dtype=np.uint64)
        self.quiet = np.clip(self.flow, -32767, 32767).astype(np.int16)
        self.want = pyoracle.filter(self.lanes, self.flow)


@functools.lru_cache(maxsize=None)
def class_case(fs, n_lanes=94, order=1):
    """case 1: whole rows of 4*Lframe + 5 samples"""
    return Case(fs, 4 * on.frame_length(fs) + 5, n_lanes, order)


def tail_sizes(L):
    sizes = [1, 3, 4, 5, 8, 12, 99, 100, 101, L - 1, L, L + 1, L + 4, 2 * L, 2 * L + 5, 4 * L + 5]
    if L == 100:
        sizes.append(4405)      # 45 frames of the shortest length the stage takes, three segments of 2048 samples
    return sizes


@functools.lru_cache(maxsize=None)
def tail_case(fs, n):
    """case 2: 130 lanes (with three segments: a block -> (utterance, segment) division by no power of two)"""
    return Case(fs, n, 130)


def restated(c):
    """(noisy, widths, aux) of the restatement on a case"""
    return on.add_noise(c.quiet, c.fs, c.snr, c.seeds)


def classes_of(W):
    return ["".join(LETTER[k] for k in on.width_class(w)) for w in W]


def mixed_octets(c, W):
    """(octets whose first quad lies in a plain frame and whose second in a non-plain one, ... the other way round),
    over the lanes with noise"""
    i0 = np.arange(0, c.n - 4, 8)
    f0, f1 = i0 // c.L, (i0 + 4) // c.L
    straddle = f0 != f1
    plain = on.is_plain(W)[c.snr > 0]
    a, b = plain[:, f0[straddle]], plain[:, f1[straddle]]
    return int((a & ~b).sum()), int((~a & b).sum())


def literal_samples(c, W):
    """samples the kernel computes in the literal form: those of octets one of whose quads lies in a non-plain frame"""
    i0 = np.arange(0, c.n, 8)
    f0, f1 = i0 // c.L, np.minimum(i0 + 4, max(c.n - 1, 0)) // c.L
    plain = on.is_plain(W)
    lit = ~(plain[:, f0] & plain[:, f1]) & (c.snr > 0)[:, None]
    return int((lit * np.minimum(8, c.n - i0)[None, :]).sum())


def clamped(c, aux):
    """(samples the noise takes past +32767, past -32767): y + aux beyond the clamp's half-way points"""
    s = c.quiet.astype(np.float64) + aux.astype(np.float64)
    return int((s > 32767.5).sum()), int((s < -32767.5).sum())


def describe(c, W, aux):
    cls = classes_of(W[c.snr > 0])
    met = "".join(k for k in "zspb" if any(k in s for s in cls))
    hi, lo = clamped(c, aux)
    return "fs %5d n %4d lanes %3d: classes met %s, %d samples on the literal path, clamped +%d -%d" % (
        c.fs, c.n, len(c.lanes), met, literal_samples(c, W), hi, lo)


# ---- the restatement's own parts

def test_frame_length_and_draws_equal_the_oracle():
    assert [on.frame_length(fs) for fs in (1999, 2000, 8000, 11025, 16000, 22050, 48000)] == [0, 100, 400, 500, 800, 1100, 2400]
    for seed in (0, 9, 0x123456789ABCDEF0):
        got = on.draws(seed, 23)
        assert [int(v) for v in got] == [pyoracle.draw(seed, k) for k in range(23)]


def test_identity_lanes_put_pcm_in_front_of_the_stage():
    c = Case(22050, 4405, 9)
    lanes = [identity_lane(22050, 0.0, 1, order) for order in (1, 23) for _ in range(9)]
    flow = np.concatenate([rows_for(22050), rows_for(22050)])
    assert np.array_equal(pyoracle.filter(lanes, flow), np.clip(flow, -32767, 32767))
    assert c.quiet.min() == -32767 and c.quiet.max() == 32767


# ---- case 1: width classes and mixed octets

def check_class_conditions(fs):
    """asserts what makes case 1 at this rate mean something; returns the line to print"""
    c = class_case(fs)
    noisy, W, aux = restated(c)
    assert np.array_equal(noisy, c.want), np.argwhere(noisy != c.want)[:8]
    pairs = {(r, s) for r, s, _ in c.plan if s > 0}
    assert len(pairs) == len(ROW_NAMES) * len(SNRS)
    off = c.snr == 0
    assert off[2::3].all() and not off[0::3].any() and not off[1::3].any()
    assert np.array_equal(c.want[off], c.quiet[off])
    cls = classes_of(W)
    for i, (r, s, _) in enumerate(c.plan):
        if r == 0 and s in PATCHWORK_CLASSES and fs == 22050:
            assert cls[i] == PATCHWORK_CLASSES[s], (s, cls[i])
    met = set("".join(np.array(cls)[~off]))
    assert met == set("zspb"), met
    # 3e37: the quotient under the root is a float32 denormal (and not zero) in some frame
    i37 = [i for i, p in enumerate(c.plan) if p[1] == SNRS[-1]]
    q = (W[i37].astype(np.float64) ** 2)
    assert ((q > 0) & (q < 2.0 ** -126)).any()
    pn, npl = mixed_octets(c, W)
    if c.L % 8 == 4:
        assert pn >= 1 and npl >= 1, (pn, npl)
    else:
        assert c.L % 8 == 0 and pn == 0 and npl == 0
    hi, lo = clamped(c, aux)
    assert hi >= 1 and lo >= 1 and (c.want == 32767).any() and (c.want == -32767).any()
    # the float power sum: a full-scale frame's is far past 2^24, and summing it in pairs gives other PCM
    full = [i for i, p in enumerate(c.plan) if ROW_NAMES[p[0]] == "alternating" and p[1] > 0]
    assert on.frame_sum(c.quiet[full[:1], :c.L])[0] > 2.0 ** 24
    other = on.add_noise(c.quiet, c.fs, c.snr, c.seeds, pairs=True)
    assert (other[1] != W).any() and (other[0] != c.want).any()
    return describe(c, W, aux) + ", octets plain|other %d other|plain %d, in pairs: %d frames %d samples differ" % (
        pn, npl, (other[1] != W).sum(), (other[0] != c.want).sum())


@pytest.mark.parametrize("fs", RATES)
def test_class_cases_meet_their_conditions(fs):
    print(check_class_conditions(fs))


def test_small_width_branch_is_observable_at_1e30():
    """the patchwork row at 22050 Hz, seed 9: at out_snr 1e30 the literal round2int and the plain form part on hundreds of
    samples; at 1e16 the small class is met and the two forms agree"""
    row = np.clip(patchwork(1100), -32767, 32767)[None, :]
    seen = {}
    for snr in (1e16, 1e20, 1e30):
        noisy, W, aux = on.add_noise(row, 22050, snr, SEED)
        lane = identity_lane(22050, snr, SEED)
        assert np.array_equal(noisy, pyoracle.filter([lane], patchwork(1100)[None, :]))
        quirk = (aux < 0) & (aux > -on.QUIRK_BOUND)
        differ = noisy != on.plain_form(row, aux)
        assert not (differ & ~quirk).any()          # outside (-2^-38, 0) the plain form IS round2int
        seen[snr] = (int(quirk.sum()), int(differ.sum()))
    print("patchwork 22050 Hz seed 9: (aux in (-2^-38, 0), literal != plain) at 1e16 %s, 1e20 %s, 1e30 %s" % (
        seen[1e16], seen[1e20], seen[1e30]))
    assert seen[1e16][1] == 0                       # taken but indistinguishable
    assert seen[1e20][0] >= 100
    assert seen[1e30][0] >= 1000 and seen[1e30][1] >= 100
    # ... and over the case's lanes a device that took every width for plain would be caught
    c = class_case(22050)
    noisy, W, aux = restated(c)
    assert (on.plain_form(c.quiet, aux) != c.want)[c.snr > 0].sum() >= 100


# ---- case 2: tails

@pytest.mark.parametrize("fs", [22050, 2000])
def test_tail_cases_equal_the_oracle(fs):
    L = on.frame_length(fs)
    for n in tail_sizes(L) + ([2049, 2048] if fs == 22050 else []):
        c = tail_case(fs, n)
        noisy, W, aux = restated(c)
        assert np.array_equal(noisy, c.want), (n, np.argwhere(noisy != c.want)[:8])
        assert W.shape[1] == (n + L - 1) // L
        off = c.snr == 0
        assert np.array_equal(c.want[off], c.quiet[off])
        print(describe(c, W, aux))
    assert tail_sizes(1100) == [1, 3, 4, 5, 8, 12, 99, 100, 101, 1099, 1100, 1101, 1104, 2200, 2205, 4405]
    assert tail_sizes(100)[-5:] == [104, 200, 205, 405, 4405]


# ---- case 4b: behind the fused kernels

@functools.lru_cache(maxsize=None)
def synth_case():
    """130 config-3 lanes at 2405 samples, the out_snr values of case 1 spread over them (every third lane none)"""
    specs, fs, dur, label = configs.config_specs(3, 130)
    lanes, _ = vs.lanes_from_specs(specs)
    for i, (_, snr, seed) in enumerate(lane_plan(130)):
        lanes[i].out_snr = snr
    return lanes, fs, 2405


def test_synth_case_equals_the_oracle_from_its_own_prenoise_pcm():
    lanes, fs, n = synth_case()
    want = pyoracle.synth(lanes, n)
    quiet_lanes = (vs.Lane * len(lanes))()
    for i, l in enumerate(lanes):
        vs.C.memmove(vs.C.byref(quiet_lanes[i]), vs.C.byref(l), vs.C.sizeof(vs.Lane))
        quiet_lanes[i].out_snr = 0.0
    quiet = pyoracle.synth(quiet_lanes, n)
    snr = np.array([l.out_snr for l in lanes], dtype=np.float32)
    seeds = np.array([l.out_seed for l in lanes], dtype=np.uint64)
    noisy, W, aux = on.add_noise(quiet, fs, snr, seeds)
    assert np.array_equal(noisy, want), np.argwhere(noisy != want)[:8]
    cls = classes_of(W[snr > 0])
    met = "".join(k for k in "zspb" if any(k in s for s in cls))
    assert "s" in met and "p" in met
    assert (noisy != quiet)[snr > 0].any(axis=1).sum() >= 30 and np.array_equal(noisy[snr == 0], quiet[snr == 0])
    print("synth: 130 config-3 lanes x %d samples at %d Hz: classes met %s, %d samples changed by the noise" % (
        n, fs, met, (noisy != quiet).sum()))
