"""voice_synth_amd -- Python test/bench driver over the C ABI of libvoicesynth.so.

The product is the C library (include/voice_synth.h, voice_synth_amd/csrc) and the two drop-in
command-line programs (voice_synth_amd/cli).  This package only wraps the C ABI with numpy
conveniences for tests/ and bench.py.  Nothing here computes samples: every synthesis call
goes to the gfx950 kernels and raises if the library or the device is missing.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import (  # noqa: F401
    Acoustic,
    CycleRec,
    MeasureOpts,
    GlottalOpts,
    GlottalRec,
    GlottalCycle,
    FlowgenCmd,
    Lane,
    LpcOpts,
    IaifOpts,
    CplpcOpts,
    PitchOpts,
    PitchFrame,
    GuidedOpts,
    GuidedRec,
    GuidedSeg,
    StrackOpts,
    StrackRow,
    StrackCycle,
    StrackStat,
    PsolaOpts,
    PsolaTsOpts,
    PsolaAnchor,
    PsolaMark,
    PsolaStat,
    TrackRow,
    TrackStat,
    InverseRow,
    InverseStat,
    Tuning,
    VowelCmd,
    VsError,
    VS_ARITH_EXACT,
    VS_ARITH_FMA,
    VS_ARITH_F32,
    VS_FLAG_JITTER,
    VS_FLAG_NOISE,
    VS_FLAG_SHIMMER,
    VS_KIND_FILTER,
    VS_KIND_SOURCE,
    VS_KIND_SYNTH,
    VS_KERNEL_AUTO,
    VS_KERNEL_SINGLE,
    VS_KERNEL_WS,
    VS_FAULT_WITHHOLD_PROGRESS,
    VS_FAULT_SHORT_COS_ROWS,
    VS_FAULT_SHARD_PREPARE,
    VS_FAULT_SHARD_HANDOVER,
    VS_FAULT_SIMD_DEALING,
    VS_FAULT_REROUND,
    VS_AC_TOO_SHORT,
    VS_AC_UNVOICED,
    VS_AC_FEW_PERIODS,
    VS_AC_ZERO_AMPLITUDE,
    VS_GL_NO_CYCLES,
    VS_GL_BAD_MARKS,
    VS_GL_REJECTED,
    VS_GL_ALL_REJECTED,
    VS_GLC_ZERO_AMPLITUDE,
    VS_GLC_NO_CLOSURE,
    VS_LPC_MAX_WINDOW,
    VS_LPC_MAX_FORMANTS,
    VS_LPC_MAX_ITER,
    VS_LPC_FORMANT_TOL_HZ,
    VS_LPC_HAMMING,
    VS_LPC_RECTANGULAR,
    VS_LPC_SILENT,
    VS_LPC_UNSTABLE,
    VS_LPC_NO_ROOTS,
    VS_CP_ANCHOR_CLOSE,
    VS_CP_ANCHOR_GCI,
    VS_CP_ANCHOR_PEAK,
    VS_CP_FEW_EQUATIONS,
    VS_CP_SINGULAR,
    VS_CP_NOT_MINIMUM_PHASE,
    VS_PT_MAX_CAND,
    VS_PT_SILENT,
    VS_PT_UNVOICED,
    VS_PT_NO_CANDIDATE,
    VS_PT_MAX_COST,
    VS_MG_ALL,
    VS_MG_LONGEST,
    VS_MG_MAX_EDGE,
    VS_ST_NO_VOICED,
    VS_ST_INTERNAL,
    VS_ST_MAX_REJECT,
    VS_PS_BAD_RUN,
    VS_PS_OVERFLOW,
    VS_PS_NO_RUN,
    VS_PS_RUN_END,
    VS_PS_BAD_MAP,
    VS_PS_UNVOICED,
    VS_PS_UNVOICED_FLIP,
    VS_TRACK_GROUP,
    VS_TRACK_HOLD,
    VS_TRACK_GLIDE,
    VS_TRACK_NO_SET,
    VS_INVERSE_NO_SET,
    check,
    load,
)

__all__ = [
    "Lane",
    "Engine",
    "DeviceScope",
    "Node",
    "Plan",
    "default_lane",
    "parse_flowgen",
    "parse_vowel",
    "lane_from_cli",
    "lanes_from_specs",
    "num_samples",
    "vowel_coefficients",
]


def default_lane():
    lane = Lane()
    check(load().vs_lane_defaults(C.byref(lane)), "vs_lane_defaults")
    return lane


def _argv(args):
    arr = (C.c_char_p * (len(args) + 1))()
    for i, a in enumerate(args):
        arr[i] = a.encode() if isinstance(a, str) else a
    arr[len(args)] = None
    return arr


def parse_flowgen(args):
    """args: flowgen_shimmer's argv[1:] (list of str).  Returns (rc, FlowgenCmd)."""
    cmd = FlowgenCmd()
    argv = _argv(["flowgen_shimmer"] + list(args))
    rc = load().vs_flowgen_parse(len(args) + 1, argv, C.byref(cmd))
    return rc, cmd


def parse_vowel(args):
    cmd = VowelCmd()
    argv = _argv(["vowel"] + list(args))
    rc = load().vs_vowel_parse(len(args) + 1, argv, C.byref(cmd))
    return rc, cmd


def lane_from_cli(flowgen_args, vowel_args, seed=0):
    """One lane from the two reference command lines (without -o / -i file arguments)."""
    rc, fc = parse_flowgen(["-o", "x.wav"] + list(flowgen_args))
    check(rc, "vs_flowgen_parse %r" % (flowgen_args,))
    rc, vc = parse_vowel(["-i", "x.wav", "-o", "y.wav"] + list(vowel_args))
    check(rc, "vs_vowel_parse %r" % (vowel_args,))
    lane = Lane()
    C.memmove(C.byref(lane), C.byref(fc.lane), C.sizeof(Lane))
    lane.gain = vc.gain
    lane.pre_emphasis = vc.pre_emphasis
    lane.vowel = vc.vowel
    lane.out_snr = vc.snr if vc.noise_arg != -1 else 0.0
    lane.seed = seed
    lane.out_seed = seed  # the two reference processes read the same VS_SEED in the shimmed build
    return lane, fc.dur


def lanes_from_specs(specs):
    """specs: iterable of (flowgen_args, vowel_args, seed).  Returns (Lane array, dur).

    Distinct command lines are parsed once by the C parser; lanes that share them only differ
    in their seed."""
    specs = list(specs)
    arr = (Lane * len(specs))()
    cache = {}
    dur = None
    for i, (fa, va, seed) in enumerate(specs):
        key = (tuple(fa), tuple(va))
        if key not in cache:
            cache[key] = lane_from_cli(fa, va, 0)
        proto, d = cache[key]
        if dur is None:
            dur = d
        elif d != dur:
            raise ValueError("all lanes of a batch share one duration")
        C.memmove(C.byref(arr[i]), C.byref(proto), C.sizeof(Lane))
        arr[i].seed = seed
        arr[i].out_seed = seed
    return arr, dur


def num_samples(fs, dur):
    n = C.c_uint64()
    check(load().vs_num_samples(int(fs), float(dur), C.byref(n)), "vs_num_samples")
    return int(n.value)


def row_pitch(n_samples):
    """vs_row_pitch: the row pitch (samples) the kernels' stores like for rows of n_samples"""
    return int(load().vs_row_pitch(int(n_samples)))


def vowel_coefficients(vowel):
    a = (C.c_double * _ffi.VS_NCOEF)()
    v = ord(vowel) if isinstance(vowel, str) else int(vowel)
    check(load().vs_vowel_coefficients(v, a), "vs_vowel_coefficients")
    return np.array(a[:], dtype=np.float64)


# the records of vs_measure as a numpy structured array (struct vs_acoustic, 96 bytes)
ACOUSTIC_DTYPE = np.dtype([(n, "<f8") for n in ("f0_hz", "jitter_local", "jitter_abs_s", "jitter_rap", "jitter_ppq5",
                                                 "shimmer_local", "shimmer_db", "shimmer_apq3", "shimmer_apq5", "hnr_db")]
                          + [(n, "<i4") for n in ("p0", "n_periods", "first_mark", "status")])


def measure_opts(f0_min=50.0, f0_max=500.0, polarity=1):
    o = MeasureOpts()
    check(load().vs_measure_defaults(C.byref(o)), "vs_measure_defaults")
    o.f0_min, o.f0_max, o.polarity = float(f0_min), float(f0_max), int(polarity)
    return o


# the records of vs_glottal (struct vs_glottal_rec, 56 bytes; struct vs_glottal_cycle, 48 bytes)
GLOTTAL_DTYPE = np.dtype([(n, "<f8") for n in ("oq", "clq", "sq", "qoq", "naq")]
                         + [(n, "<i4") for n in ("n_cycles", "n_rejected", "status", "reserved_")])
GLOTTAL_CYCLE_DTYPE = np.dtype([(n, "<i4") for n in ("peak", "period", "trough", "amp", "open", "close", "open_mid",
                                                      "close_mid", "gci", "decl", "status", "reserved_")])


def glottal_opts(level_open=26, level_mid=128, polarity=1):
    o = GlottalOpts()
    check(load().vs_glottal_defaults(C.byref(o)), "vs_glottal_defaults")
    o.level_open, o.level_mid, o.polarity = int(level_open), int(level_mid), int(polarity)
    return o


# the records of vs_lpc (struct vs_lpc_frame, 32 bytes)
LPC_FRAME_DTYPE = np.dtype([("r0", "<f8"), ("err", "<f8"), ("start", "<i4"), ("n_formants", "<i4"), ("status", "<i4"),
                            ("reserved_", "<i4")])


def lpc_opts(order=22, window=VS_LPC_HAMMING, window_s=0.025, hop_s=0.010, pre_emphasis=0, n_formants=5, f_lo=50.0):
    """struct vs_lpc_opts from vs_lpc_defaults and the given fields (window: VS_LPC_HAMMING / VS_LPC_RECTANGULAR, or
    "hamming" / "rectangular")"""
    o = LpcOpts()
    check(load().vs_lpc_defaults(C.byref(o)), "vs_lpc_defaults")
    if isinstance(window, str):
        window = {"hamming": VS_LPC_HAMMING, "rectangular": VS_LPC_RECTANGULAR}[window]
    o.order, o.window, o.pre_emphasis, o.n_formants = int(order), int(window), int(pre_emphasis), int(n_formants)
    o.window_s, o.hop_s, o.f_lo = float(window_s), float(hop_s), float(f_lo)
    return o


def lpc_frames(fs, length, **opts):
    """vs_lpc_frames: the number of analysis frames of a row of `length` samples at rate fs"""
    n = C.c_int32()
    check(load().vs_lpc_frames(C.byref(lpc_opts(**opts)), int(fs), int(length), C.byref(n)), "vs_lpc_frames")
    return int(n.value)


def lpc_window(L, window=VS_LPC_HAMMING):
    """vs_lpc_window: the integer window table w[0..L)"""
    w = np.zeros(int(L), dtype=np.int32)
    check(load().vs_lpc_window(int(L), int(window), w.ctypes.data), "vs_lpc_window")
    return w


def iaif_opts(order=22, glottal_order=4, window=VS_LPC_HAMMING, window_s=0.025, hop_s=0.010, n_formants=5, f_lo=50.0,
              leak=0.99):
    """struct vs_iaif_opts from vs_iaif_defaults and the given fields (window as in lpc_opts())"""
    o = IaifOpts()
    check(load().vs_iaif_defaults(C.byref(o)), "vs_iaif_defaults")
    if isinstance(window, str):
        window = {"hamming": VS_LPC_HAMMING, "rectangular": VS_LPC_RECTANGULAR}[window]
    o.order, o.glottal_order, o.window, o.n_formants = int(order), int(glottal_order), int(window), int(n_formants)
    o.window_s, o.hop_s, o.f_lo, o.leak = float(window_s), float(hop_s), float(f_lo), float(leak)
    return o


def iaif_lpc_opts(**opts):
    """vs_iaif_lpc_opts: the lpc_opts() keywords with the frame plan of iaif_opts(**opts), for lpc_frames(),
    track_from_lpc() and inverse_from_lpc(); VsError where vs_iaif_launch refuses the options"""
    lo = LpcOpts()
    check(load().vs_iaif_lpc_opts(C.byref(iaif_opts(**opts)), C.byref(lo)), "vs_iaif_lpc_opts")
    return dict(order=lo.order, window=lo.window, window_s=lo.window_s, hop_s=lo.hop_s, pre_emphasis=lo.pre_emphasis,
                n_formants=lo.n_formants, f_lo=lo.f_lo)


def cplpc_opts(order=22, anchor=VS_CP_ANCHOR_CLOSE, delay=4, span_q=77, min_equations=0, n_formants=5, window_s=0.0,
               hop_s=0.010, f_lo=50.0):
    """struct vs_cplpc_opts from vs_cplpc_defaults and the given fields (anchor: VS_CP_ANCHOR_*, or "close" / "gci" /
    "peak")"""
    o = CplpcOpts()
    check(load().vs_cplpc_defaults(C.byref(o)), "vs_cplpc_defaults")
    if isinstance(anchor, str):
        anchor = {"close": VS_CP_ANCHOR_CLOSE, "gci": VS_CP_ANCHOR_GCI, "peak": VS_CP_ANCHOR_PEAK}[anchor]
    o.order, o.anchor, o.delay, o.span_q = int(order), int(anchor), int(delay), int(span_q)
    o.min_equations, o.n_formants = int(min_equations), int(n_formants)
    o.window_s, o.hop_s, o.f_lo = float(window_s), float(hop_s), float(f_lo)
    return o


def cplpc_frames(fs, length, **opts):
    """vs_cplpc_frames: the frames of a row of `length` samples at rate fs: 1 with window_s == 0"""
    n = C.c_int32()
    check(load().vs_cplpc_frames(C.byref(cplpc_opts(**opts)), int(fs), int(length), C.byref(n)), "vs_cplpc_frames")
    return int(n.value)


def cplpc_lpc_opts(**opts):
    """vs_cplpc_lpc_opts: the lpc_opts() keywords with the frame plan of cplpc_opts(**opts) (window_s > 0), for
    lpc_frames(), track_from_lpc() and inverse_from_lpc(); VsError where vs_cplpc_launch refuses the options"""
    lo = LpcOpts()
    check(load().vs_cplpc_lpc_opts(C.byref(cplpc_opts(**opts)), C.byref(lo)), "vs_cplpc_lpc_opts")
    return dict(order=lo.order, window=lo.window, window_s=lo.window_s, hop_s=lo.hop_s, pre_emphasis=lo.pre_emphasis,
                n_formants=lo.n_formants, f_lo=lo.f_lo)


# the records of vs_pitch (struct vs_pitch_frame, 96 bytes)
PITCH_FRAME_DTYPE = np.dtype([("r0", "<i8"), ("start", "<i4"), ("lag", "<i4"), ("q", "<i4"), ("status", "<i4"),
                              ("n_cand", "<i4"), ("reserved_", "<i4"), ("cand_lag", "<i4", (VS_PT_MAX_CAND,)),
                              ("cand_q", "<i4", (VS_PT_MAX_CAND,)), ("back", "u1", (VS_PT_MAX_CAND + 1,))])


def pitch_opts(f0_min=50.0, f0_max=500.0, voicing_q=14746, octave_q=328, jump_q=11469, vuv_q=4588, silence_rms=16,
               hop_s=0.010):
    """struct vs_pitch_opts from vs_pitch_defaults and the given fields (the four costs in Q15)"""
    o = PitchOpts()
    check(load().vs_pitch_defaults(C.byref(o)), "vs_pitch_defaults")
    o.f0_min, o.f0_max, o.hop_s = float(f0_min), float(f0_max), float(hop_s)
    o.voicing_q, o.octave_q, o.jump_q, o.vuv_q = int(voicing_q), int(octave_q), int(jump_q), int(vuv_q)
    o.silence_rms = int(silence_rms)
    return o


def pitch_frames(fs, length, **opts):
    """vs_pitch_frames: the frames of a row of `length` samples at rate fs"""
    n = C.c_int32()
    check(load().vs_pitch_frames(C.byref(pitch_opts(**opts)), int(fs), int(length), C.byref(n)), "vs_pitch_frames")
    return int(n.value)


def pitch_log2_table(n=_ffi.VS_AC_MAX_LAG + 1):
    """vs_pitch_log2_table: Lg[0..n)"""
    lg = np.zeros(int(n), dtype=np.int32)
    check(load().vs_pitch_log2_table(int(n), lg.ctypes.data), "vs_pitch_log2_table")
    return lg


# the records of vs_guided (struct vs_guided_rec and struct vs_guided_seg, 16 bytes each)
GUIDED_REC_DTYPE = np.dtype([(n, "<i4") for n in ("n_segments", "n_marks", "n_frames_walked", "reserved_")])
GUIDED_SEG_DTYPE = np.dtype([(n, "<i4") for n in ("first_frame", "n_frames", "first_mark_index", "n_marks")])


def guided_opts(f0_min=50.0, f0_max=500.0, polarity=1, segments=VS_MG_ALL, edge_frames=1, min_frames=3, hop_s=0.010):
    """struct vs_guided_opts from vs_guided_defaults and the given fields (segments: VS_MG_ALL / VS_MG_LONGEST, or "all" /
    "longest")"""
    o = GuidedOpts()
    check(load().vs_guided_defaults(C.byref(o)), "vs_guided_defaults")
    if isinstance(segments, str):
        segments = {"all": VS_MG_ALL, "longest": VS_MG_LONGEST}[segments]
    o.f0_min, o.f0_max, o.hop_s = float(f0_min), float(f0_max), float(hop_s)
    o.polarity, o.segments, o.edge_frames, o.min_frames = int(polarity), int(segments), int(edge_frames), int(min_frames)
    return o


def guided_plan(fs, length, **opts):
    """vs_guided_plan: dict(tmin, tmax, hop, n_frames, centre) of a row of `length` samples at rate fs"""
    v = [C.c_int32() for _ in range(5)]
    check(load().vs_guided_plan(C.byref(guided_opts(**opts)), int(fs), int(length), *[C.byref(x) for x in v]),
          "vs_guided_plan")
    return dict(zip(("tmin", "tmax", "hop", "n_frames", "centre"), (int(x.value) for x in v)))


def set_coefficients(lane, A):
    """make `lane` filter with the all-pole set 1/A(z): VS_VOWEL_CUSTOM, order = len(A) - 1, A[0] must be 1 (e.g. a
    row of Engine.lpc(..., coefs=True)["coefs"]).  Returns the lane."""
    A = np.asarray(A, dtype=np.float64).ravel()
    order = len(A) - 1
    if not 1 <= order <= _ffi.VS_MAX_ORDER or A[0] != 1.0 or not np.all(np.isfinite(A)):
        raise ValueError("A: 2..%d finite coefficients with A[0] == 1" % (_ffi.VS_MAX_ORDER + 1))
    lane.vowel = 0                               # VS_VOWEL_CUSTOM
    lane.order = order
    for j in range(len(lane.A)):
        lane.A[j] = float(A[j]) if j <= order else 0.0
    return lane


# the records of the coefficient tracks (struct vs_track_row, 24 bytes; struct vs_track_stat, 8 bytes)
TRACK_ROW_DTYPE = np.dtype([("n_sets", "<i4"), ("hop", "<i4"), ("offset", "<i4"), ("length", "<i4"), ("gain", "<f4"),
                            ("pre_emphasis", "<f4")])
TRACK_STAT_DTYPE = np.dtype([("status", "<i4"), ("n_unusable", "<i4")])


def _track_mode(mode):
    if isinstance(mode, str):
        return {"hold": VS_TRACK_HOLD, "glide": VS_TRACK_GLIDE}[mode]
    return int(mode)


def _coef_set(A, name):
    A = np.ascontiguousarray(A, dtype=np.float64).ravel()
    if not 2 <= len(A) <= _ffi.VS_MAX_NCOEF:
        raise ValueError("%s: 2..%d coefficients" % (name, _ffi.VS_MAX_NCOEF))
    return A


def track_reflection(A):
    """vs_track_reflection: the reflection coefficients k_1..k_p of the set A[0..p] (step-down); VsError(VS_ERR_RANGE)
    for a tap that is not finite or a |k_i| >= 1"""
    A = _coef_set(A, "A")
    k = np.zeros(len(A) - 1, dtype=np.float64)
    check(load().vs_track_reflection(len(A) - 1, A.ctypes.data, k.ctypes.data), "vs_track_reflection")
    return k


def track_glide_sets(A_from, A_to, n_sets):
    """vs_track_glide_sets: n_sets sets [n_sets][order+1] from A_from to A_to, evenly spaced in the reflection domain"""
    A_from, A_to = _coef_set(A_from, "A_from"), _coef_set(A_to, "A_to")
    if len(A_from) != len(A_to):
        raise ValueError("A_from and A_to: the same order")
    out = np.zeros((max(int(n_sets), 0), len(A_from)), dtype=np.float64)
    check(load().vs_track_glide_sets(len(A_from) - 1, A_from.ctypes.data, A_to.ctypes.data, int(n_sets),
                                     out.ctypes.data), "vs_track_glide_sets")
    return out


def track_from_lpc(fs, length, mode="hold", **opts):
    """vs_track_from_lpc: the track row (a TRACK_ROW_DTYPE record) that plays the frames Engine.lpc(**opts) makes of a
    row of `length` samples at rate fs"""
    row = TrackRow()
    check(load().vs_track_from_lpc(C.byref(lpc_opts(**opts)), int(fs), int(length), _track_mode(mode), C.byref(row)),
          "vs_track_from_lpc")
    return np.frombuffer(bytes(row), dtype=TRACK_ROW_DTYPE)[0].copy()


def track_rows(n, n_sets, hop, offset=0, lengths=0, gain=1.0, pre_emphasis=0.0):
    """n vs_track_row records (TRACK_ROW_DTYPE); every argument takes one value or one per row"""
    rows = np.zeros(n, dtype=TRACK_ROW_DTYPE)
    rows["n_sets"] = _row_array(n_sets, n, "n_sets")
    rows["hop"] = _row_array(hop, n, "hop")
    rows["offset"] = _row_array(offset, n, "offset")
    rows["length"] = _row_array(lengths, n, "lengths")
    rows["gain"] = np.broadcast_to(np.asarray(gain, dtype=np.float32), (n,))
    rows["pre_emphasis"] = np.broadcast_to(np.asarray(pre_emphasis, dtype=np.float32), (n,))
    return rows


# the records of the source track (struct vs_strack_row, 24 bytes; vs_strack_stat, 24 bytes; vs_strack_cycle, 32 bytes)
STRACK_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("n_frames", "hop", "offset", "length", "pmin", "pmax")])
STRACK_STAT_DTYPE = np.dtype([("status", "<i4"), ("n_cycles", "<i4"), ("n_resets", "<i4"), ("n_unvoiced", "<i4"),
                              ("n_draws", "<u8")])
STRACK_CYCLE_DTYPE = np.dtype([("start", "<i4"), ("T", "<i4"), ("frame", "<i4"), ("amp", "<i4"), ("S", "<f4"),
                               ("x_pow", "<f4"), ("w_pow", "<f4"), ("reserved_", "<i4")])


def strack_opts(max_reject=256):
    """struct vs_strack_opts: vs_strack_defaults() with max_reject replaced"""
    o = StrackOpts()
    check(load().vs_strack_defaults(C.byref(o)), "vs_strack_defaults")
    o.max_reject = int(max_reject)
    return o


def strack_row_from_pitch(fs, length, **opts):
    """vs_strack_from_pitch: the source-track row (a STRACK_ROW_DTYPE record) that plays the frames Engine.pitch(**opts)
    makes of a row of `length` samples at rate fs"""
    row = StrackRow()
    check(load().vs_strack_from_pitch(C.byref(pitch_opts(**opts)), int(fs), int(length), C.byref(row)),
          "vs_strack_from_pitch")
    return np.frombuffer(bytes(row), dtype=STRACK_ROW_DTYPE)[0].copy()


def strack_rows(n, n_frames, hop, offset=0, lengths=0, pmin=2, pmax=2048):
    """n vs_strack_row records (STRACK_ROW_DTYPE); every argument takes one value or one per row"""
    rows = np.zeros(n, dtype=STRACK_ROW_DTYPE)
    for name, v in (("n_frames", n_frames), ("hop", hop), ("offset", offset), ("length", lengths), ("pmin", pmin),
                    ("pmax", pmax)):
        rows[name] = _row_array(v, n, name)
    return rows


# the records of PSOLA (struct vs_psola_mark, 16 bytes; vs_psola_stat, 24 bytes)
PSOLA_MARK_DTYPE = np.dtype([(n, "<i4") for n in ("t", "k", "cycle", "gain")])
PSOLA_STAT_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_runs", "n_runs_done", "n_synth", "n_governed", "n_clipped")])


def psola_opts(pmin=None, pmax=None):
    """struct vs_psola_opts: vs_psola_defaults() (32 and 320: the default F0 range at 16 kHz) with what is given replaced"""
    o = PsolaOpts()
    check(load().vs_psola_defaults(C.byref(o)), "vs_psola_defaults")
    if pmin is not None:
        o.pmin = int(pmin)
    if pmax is not None:
        o.pmax = int(pmax)
    return o


# the anchors of PSOLA's time map (struct vs_psola_anchor, 8 bytes)
PSOLA_ANCHOR_DTYPE = np.dtype([("u", "<i4"), ("v", "<i4")])


def psola_ts_opts(pmin=None, pmax=None, unvoiced_period=None):
    """struct vs_psola_ts_opts: vs_psola_ts_defaults() (32, 320 and 80 samples: 5 ms at 16 kHz) with what is given
    replaced"""
    o = PsolaTsOpts()
    check(load().vs_psola_ts_defaults(C.byref(o)), "vs_psola_ts_defaults")
    if pmin is not None:
        o.pmin = int(pmin)
    if pmax is not None:
        o.pmax = int(pmax)
    if unvoiced_period is not None:
        o.unvoiced_period = int(unvoiced_period)
    return o


def psola_two_anchors(lengths, out_lengths, map_pitch=2):
    """the map of a uniform change of duration, one row each: (anchors PSOLA_ANCHOR_DTYPE [rows][map_pitch], counts)"""
    lengths, out_lengths = np.atleast_1d(lengths), np.atleast_1d(out_lengths)
    an = np.zeros((len(lengths), int(map_pitch)), dtype=PSOLA_ANCHOR_DTYPE)
    an["u"][:, 1], an["v"][:, 1] = out_lengths, lengths
    return an, np.full(len(lengths), 2, dtype=np.int32)


# the records of the inverse filter (struct vs_inverse_row, 24 bytes; struct vs_inverse_stat, 16 bytes)
INVERSE_ROW_DTYPE = np.dtype([("n_sets", "<i4"), ("hop", "<i4"), ("offset", "<i4"), ("length", "<i4"), ("scale", "<f4"),
                              ("de_emphasis", "<f4")])
INVERSE_STAT_DTYPE = np.dtype([("status", "<i4"), ("n_unusable", "<i4"), ("n_clipped", "<i4"), ("reserved_", "<i4")])


def inverse_from_lpc(fs, length, mode="hold", **opts):
    """vs_inverse_from_lpc: the inverse row (an INVERSE_ROW_DTYPE record) over the frames Engine.lpc(**opts) makes of a
    row of `length` samples at rate fs: the sets of track_from_lpc() at the same samples, scale 1, de_emphasis 0"""
    row = InverseRow()
    check(load().vs_inverse_from_lpc(C.byref(lpc_opts(**opts)), int(fs), int(length), _track_mode(mode), C.byref(row)),
          "vs_inverse_from_lpc")
    return np.frombuffer(bytes(row), dtype=INVERSE_ROW_DTYPE)[0].copy()


def inverse_rows(n, n_sets, hop, offset=0, lengths=0, scale=1.0, de_emphasis=0.0):
    """n vs_inverse_row records (INVERSE_ROW_DTYPE); every argument takes one value or one per row"""
    rows = np.zeros(n, dtype=INVERSE_ROW_DTYPE)
    rows["n_sets"] = _row_array(n_sets, n, "n_sets")
    rows["hop"] = _row_array(hop, n, "hop")
    rows["offset"] = _row_array(offset, n, "offset")
    rows["length"] = _row_array(lengths, n, "lengths")
    rows["scale"] = np.broadcast_to(np.asarray(scale, dtype=np.float32), (n,))
    rows["de_emphasis"] = np.broadcast_to(np.asarray(de_emphasis, dtype=np.float32), (n,))
    return rows


def _row_array(v, n, name):
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.int32), (n,)))
    if a.shape != (n,):
        raise ValueError("%s: one value per row" % name)
    return a


def _row_pair(fs, lengths, n, default=None):
    """fs and lengths as one int32 per row; without lengths: `default` for every row, or None where there is none"""
    if lengths is None:
        lengths = default
    return _row_array(fs, n, "fs"), None if lengths is None else _row_array(lengths, n, "lengths")


def _pcm_rows(pcm, fs, lengths, whole=False):
    """the prelude of the host-buffer analyses: pcm as contiguous int16 [rows][samples] and its _row_pair (whole: rows
    without a length are pcm.shape[1] long, not None)"""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    assert pcm.ndim == 2
    return (pcm,) + _row_pair(fs, lengths, pcm.shape[0], pcm.shape[1] if whole else None)


def _ptr(a):
    """the address of an array for the C call: NULL for None and for an empty one"""
    return a.ctypes.data if a is not None and a.size else None


def _frame_fill(n, fp):
    """[n][fp] frame records as a call finds them: NaN r0 and err, start and status -1"""
    fr = np.zeros((n, fp), dtype=LPC_FRAME_DTYPE)
    fr["r0"] = fr["err"] = np.nan
    fr["start"] = fr["status"] = -1
    return fr


def _frame_result(fr, nfr):
    """the head of the result dict of lpc(), iaif(), cplpc() and closed_phase()'s sets: the records' fields, n_frames"""
    out = {k: fr[k].copy() for k in ("r0", "err", "start", "status", "n_formants")}
    out["n_frames"] = nfr
    return out


def _as_lane_array(lanes):
    if isinstance(lanes, C.Array):
        return lanes
    lanes = list(lanes)
    arr = (Lane * len(lanes))()
    for i, l in enumerate(lanes):
        C.memmove(C.byref(arr[i]), C.byref(l), C.sizeof(Lane))
    return arr


class _Closing:
    """`with` for what has a close(): Engine, Node and Plan"""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DeviceScope:
    """Engine.scope(): the device buffers and plans of one `with` block.  On exit the plans are closed, then the buffers
    freed, each in reverse order of creation, whether or not the body raised.  While an exception is on its way out an
    error from a close or a free gives way to it; on a clean exit the first such error is raised, after the rest has
    been released.  The scope waits for nothing itself: vs_dev_free waits for the device."""

    def __init__(self, engine):
        self.engine = engine
        self._plans, self._ptrs = [], []

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        failed = None
        for release, held in ((lambda plan: plan.close(), self._plans), (self.engine.dev_free, self._ptrs)):
            while held:
                try:
                    release(held.pop())
                except Exception as e:
                    failed = failed or e
        if failed is not None and exc_type is None:
            raise failed

    def room(self, nbytes):
        """a device pointer to max(1, nbytes) bytes"""
        self._ptrs.append(self.engine.dev_alloc(max(1, int(nbytes))))
        return self._ptrs[-1]

    def put(self, array):
        """a device pointer to an uploaded copy of array"""
        array = np.ascontiguousarray(array)
        ptr = self.room(array.nbytes)
        self.engine.dev_upload(ptr, array)
        return ptr

    def filled(self, count, value, dtype):
        """a device pointer to count items of value"""
        return self.put(np.full(int(count), value, dtype=dtype))

    def get(self, ptr, shape, dtype=np.int16):
        return self.engine.dev_download(ptr, shape, dtype)

    def plan(self, lanes, n_samples):
        """a Plan that the scope closes"""
        self._plans.append(self.engine.plan(lanes, n_samples))
        return self._plans[-1]


class Engine(_Closing):
    """A vs_ctx.  Raises VsError(VS_ERR_NODEVICE) when no gfx950 device is usable."""

    def __init__(self, device=0, arith=VS_ARITH_EXACT, stream=None):
        self._lib = load()
        self._ctx = C.c_void_p()
        check(self._lib.vs_ctx_create(int(device), C.byref(self._ctx)), "vs_ctx_create")
        self.set_arith(arith)
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if self._ctx:
            self._lib.vs_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_arith(self, arith):
        check(self._lib.vs_ctx_set_arith(self._ctx, int(arith)), "vs_ctx_set_arith")
        self.arith = int(arith)

    def set_tuning(self, **kw):
        """vs_ctx_set_tuning(): keyword arguments are vs_tuning fields (kernel=, ring_slots=,
        ready_min=, ws_pairs=, gen_low=, gen_min=, spin_limit=, fault=); no arguments resets.
        Applies to plans made afterwards."""
        if not kw:
            check(self._lib.vs_ctx_set_tuning(self._ctx, None), "vs_ctx_set_tuning")
            return
        t = Tuning()
        for k, v in kw.items():
            setattr(t, k, int(v))
        check(self._lib.vs_ctx_set_tuning(self._ctx, C.byref(t)), "vs_ctx_set_tuning")

    def set_stream(self, hip_stream):
        check(self._lib.vs_ctx_set_stream(self._ctx, C.c_void_p(int(hip_stream))), "vs_ctx_set_stream")

    def synchronize(self):
        check(self._lib.vs_ctx_synchronize(self._ctx), "vs_ctx_synchronize")

    def timer_mark(self, which):
        """vs_ctx_timer_mark(): an event behind what has been enqueued on the context's stream so far (0 = start, 1 = end)"""
        check(self._lib.vs_ctx_timer_mark(self._ctx, int(which)), "vs_ctx_timer_mark")

    def timer_elapsed(self):
        """vs_ctx_timer_elapsed(): waits for mark 1, milliseconds of device time from mark 0 to it"""
        ms = C.c_double()
        check(self._lib.vs_ctx_timer_elapsed(self._ctx, C.byref(ms)), "vs_ctx_timer_elapsed")
        return ms.value

    def selftest(self):
        """(rc, [division shortcut, philox, isqrt, round2int, noise sample, philox2, wave-to-SIMD dealing, output-noise sample] failure counts)"""
        f = (C.c_uint64 * 8)()
        rc = self._lib.vs_ctx_selftest(self._ctx, f)
        return rc, [int(v) for v in f]

    def simd_dealing(self):
        """vs_ctx_simd_dealing(): (wavefront w of a 12-wavefront workgroup ran on SIMD w % 4, ... of an 8-wavefront one)"""
        a, b = C.c_int(), C.c_int()
        check(self._lib.vs_ctx_simd_dealing(self._ctx, C.byref(a), C.byref(b)), "vs_ctx_simd_dealing")
        return bool(a.value), bool(b.value)

    def device_info(self):
        name = C.create_string_buffer(128)
        cu = C.c_int()
        check(self._lib.vs_ctx_device_info(self._ctx, name, 128, C.byref(cu)), "vs_ctx_device_info")
        return name.value.decode(), cu.value

    def device_pci(self):
        """PCI bus id of the device in use ("0000:05:00.0")"""
        buf = C.create_string_buffer(32)
        check(self._lib.vs_ctx_device_pci(self._ctx, buf, 32), "vs_ctx_device_pci")
        return buf.value.decode()

    # ---- host-buffer conveniences ----
    def synth(self, lanes, n_samples):
        arr = _as_lane_array(lanes)
        out = np.empty((len(arr), n_samples), dtype=np.int16)
        check(self._lib.vs_synth(self._ctx, arr, len(arr), n_samples, out.ctypes.data), "vs_synth")
        return out

    def synth_pinned(self, lanes, n_samples):
        """vs_synth() into PINNED host memory from vs_host_alloc(): the finished rows are DMAed
        straight into the destination.  Returns a numpy view; free it with host_free(view)."""
        arr = _as_lane_array(lanes)
        nbytes = len(arr) * n_samples * 2
        p = C.c_void_p()
        check(self._lib.vs_host_alloc(self._ctx, nbytes, C.byref(p)), "vs_host_alloc")
        buf = (C.c_int16 * (len(arr) * n_samples)).from_address(p.value)
        out = np.frombuffer(buf, dtype=np.int16).reshape(len(arr), n_samples)
        try:
            check(self._lib.vs_synth(self._ctx, arr, len(arr), n_samples, p), "vs_synth")
        except Exception:
            self._lib.vs_host_free(self._ctx, p)
            raise
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[out.ctypes.data] = p.value
        return out

    def host_free(self, view):
        p = self._pinned.pop(view.ctypes.data)
        check(self._lib.vs_host_free(self._ctx, C.c_void_p(p)), "vs_host_free")

    def synth_rows(self, lanes, n_samples, fn):
        """vs_synth_rows(): fn(row0, rows_array) is called for every delivered block (from the
        library's delivery threads, possibly concurrently); rows_array is only valid inside fn."""
        arr = _as_lane_array(lanes)

        def tramp(user, row0, rows, ptr):
            try:
                buf = (C.c_int16 * (rows * n_samples)).from_address(ptr)
                return int(fn(int(row0), np.frombuffer(buf, dtype=np.int16).reshape(rows, n_samples)) or 0)
            except Exception:  # pragma: no cover - surfaces as VS_ERR_IO
                return 1

        cb = _ffi.ROWS_CB(tramp)
        check(self._lib.vs_synth_rows(self._ctx, arr, len(arr), n_samples, cb, None), "vs_synth_rows")

    def trim(self):
        check(self._lib.vs_ctx_trim(self._ctx), "vs_ctx_trim")

    def source(self, lanes, n_samples, log_cycles=0):
        arr = _as_lane_array(lanes)
        out = np.empty((len(arr), n_samples), dtype=np.int16)
        if log_cycles:
            recs = (CycleRec * (len(arr) * log_cycles))()
            ncyc = np.zeros(len(arr), dtype=np.int32)
            check(
                self._lib.vs_source(self._ctx, arr, len(arr), n_samples, out.ctypes.data,
                                    C.addressof(recs), log_cycles, ncyc.ctypes.data),
                "vs_source",
            )
            rec_np = np.frombuffer(recs, dtype=[("S", "<f4"), ("x_pow", "<f4"), ("w_pow", "<f4"), ("T", "<i4")])
            return out, rec_np.reshape(len(arr), log_cycles).copy(), ncyc
        check(self._lib.vs_source(self._ctx, arr, len(arr), n_samples, out.ctypes.data, None, 0, None),
              "vs_source")
        return out

    def filter(self, lanes, flow):
        arr = _as_lane_array(lanes)
        flow = np.ascontiguousarray(flow, dtype=np.int16)
        assert flow.ndim == 2 and flow.shape[0] == len(arr)
        out = np.empty_like(flow)
        check(self._lib.vs_filter(self._ctx, arr, len(arr), flow.shape[1], flow.ctypes.data,
                                  out.ctypes.data), "vs_filter")
        return out

    def measure(self, pcm, fs, f0_min=50, f0_max=500, polarity=1, lengths=None, marks=0):
        """vs_measure(): F0, jitter, shimmer and HNR of every row of pcm (int16 [rows][samples]) on the device.  fs and
        lengths: a value per row (or one for all).  Returns the records (ACOUSTIC_DTYPE) and, with marks > 0, an int32
        [rows][marks] array of the cycle marks m_0..m_K (-1 past the last)."""
        pcm, fs, ln = _pcm_rows(pcm, fs, lengths)
        n = pcm.shape[0]
        out = np.zeros(n, dtype=ACOUSTIC_DTYPE)
        mk = np.full((n, marks), -1, dtype=np.int32) if marks else None
        o = measure_opts(f0_min, f0_max, polarity)
        check(self._lib.vs_measure(self._ctx, C.byref(o), pcm.ctypes.data, pcm.shape[1], n, pcm.shape[1], fs.ctypes.data,
                                   _ptr(ln), out.ctypes.data, _ptr(mk), int(marks)), "vs_measure")
        return (out, mk) if marks else out

    def measure_dev(self, pcm_ptr, pitch, n_lanes, n_samples, fs, out_ptr, f0_min=50, f0_max=500, polarity=1,
                    lengths=None, marks_ptr=None, marks_pitch=0):
        """vs_measure_launch(): device pointers (PCM [n_lanes][pitch] int16, records [n_lanes] vs_acoustic, marks
        [n_lanes][marks_pitch] int32 or None), enqueued on the context's stream behind what is there -- e.g. a
        Plan.launch() into pcm_ptr; returns without waiting.  fs / lengths: host values, one per row (or one for all)."""
        fs, ln = _row_pair(fs, lengths, n_lanes)
        o = measure_opts(f0_min, f0_max, polarity)
        check(self._lib.vs_measure_launch(self._ctx, C.byref(o), C.c_void_p(pcm_ptr), int(pitch), int(n_lanes),
                                          int(n_samples), fs.ctypes.data, _ptr(ln), C.c_void_p(out_ptr),
                                          C.c_void_p(marks_ptr), int(marks_pitch)), "vs_measure_launch")

    def measure_guided(self, pcm, fs, lengths=None, marks=0, segs=0, pitch=None, **opts):
        """vs_guided(): the pitch track of every row of pcm (int16 [rows][samples]) and, steered by it, the guided marks
        and their summary.  fs and lengths: a value per row (or one for all); opts: those of guided_opts(); pitch: a dict
        of pitch_opts() keywords for the track's costs and silence_rms (its f0_min, f0_max and hop_s are opts').  marks:
        marks_pitch; segs: seg_pitch.  Returns (records ACOUSTIC_DTYPE [rows], marks int32 [rows][marks] with -1 past the
        last or None, rec GUIDED_REC_DTYPE [rows], segs GUIDED_SEG_DTYPE [rows][segs] or None, frames PITCH_FRAME_DTYPE
        [rows][frames_pitch])."""
        pcm, fs, ln = _pcm_rows(pcm, fs, lengths, whole=True)
        n = pcm.shape[0]
        shapes = set(zip(fs.tolist(), ln.tolist()))
        fp = max(1, max(guided_plan(f, l, **opts)["n_frames"] for f, l in shapes))
        out = np.zeros(n, dtype=ACOUSTIC_DTYPE)
        mk = np.full((n, int(marks)), -1, dtype=np.int32) if marks else None
        rec = np.zeros(n, dtype=GUIDED_REC_DTYPE)
        sg = np.zeros((n, int(segs)), dtype=GUIDED_SEG_DTYPE) if segs else None
        fr = np.zeros((n, fp), dtype=PITCH_FRAME_DTYPE)
        o, po = guided_opts(**opts), pitch_opts(**dict(pitch or {}))
        check(self._lib.vs_guided(self._ctx, C.byref(o), C.byref(po), pcm.ctypes.data, pcm.shape[1], n, pcm.shape[1],
                                  fs.ctypes.data, ln.ctypes.data, fp, fr.ctypes.data, out.ctypes.data, _ptr(mk),
                                  int(marks), rec.ctypes.data, _ptr(sg), int(segs)), "vs_guided")
        return out, mk, rec, sg, fr

    def measure_guided_dev(self, pcm_ptr, pitch, n_lanes, n_samples, fs, frames_ptr, frames_pitch, out_ptr, rec_ptr,
                           marks_ptr=None, marks_pitch=0, segs_ptr=None, seg_pitch=0, lengths=None, **opts):
        """vs_guided_launch(): device pointers (PCM [n_lanes][pitch] int16; the records [n_lanes][frames_pitch]
        vs_pitch_frame a pitch_dev() before it on the context's stream wrote, with the same f0_min, f0_max and hop_s;
        records [n_lanes] vs_acoustic and vs_guided_rec; marks [n_lanes][marks_pitch] int32 and segments
        [n_lanes][seg_pitch] vs_guided_seg, or None); returns without waiting.  fs / lengths: host values, one per row
        (or one for all); opts: those of guided_opts()."""
        fs, ln = _row_pair(fs, lengths, n_lanes)
        o = guided_opts(**opts)
        check(self._lib.vs_guided_launch(self._ctx, C.byref(o), C.c_void_p(pcm_ptr), int(pitch), int(n_lanes),
                                         int(n_samples), fs.ctypes.data, _ptr(ln), C.c_void_p(frames_ptr),
                                         int(frames_pitch), C.c_void_p(out_ptr), C.c_void_p(marks_ptr), int(marks_pitch),
                                         C.c_void_p(rec_ptr), C.c_void_p(segs_ptr), int(seg_pitch)), "vs_guided_launch")

    def _guided_marks_dev(self, dev, d_pcm, n, ns, fs, lengths, d_meas, d_marks, mp, f0_min, f0_max, polarity):
        """pitch_dev() and measure_guided_dev() (VS_MG_LONGEST, the other options at their defaults) where a chain has
        measure_dev(): returns (the frames' buffer, frames_pitch, the guided records' buffer)"""
        fsr, ln = _row_pair(fs, lengths, n, ns)
        fp = max(1, max(guided_plan(f, l, f0_min=f0_min, f0_max=f0_max)["n_frames"]
                        for f, l in set(zip(fsr.tolist(), ln.tolist()))))
        d_fr = dev.put(np.zeros((n, fp), dtype=PITCH_FRAME_DTYPE))
        d_rec = dev.room(n * GUIDED_REC_DTYPE.itemsize)
        self.pitch_dev(d_pcm, ns, n, ns, fsr, fp, d_fr, lengths=ln, f0_min=f0_min, f0_max=f0_max)
        self.measure_guided_dev(d_pcm, ns, n, ns, fsr, d_fr, fp, d_meas, d_rec, d_marks, mp, lengths=ln, f0_min=f0_min,
                                f0_max=f0_max, polarity=polarity, segments=VS_MG_LONGEST)
        return d_fr, fp, d_rec

    def _glottal_guided(self, pcm, fs, level_open, level_mid, polarity, f0_min, f0_max, lengths, marks, cycles):
        """glottal(..., guided=True): pitch_dev -> measure_guided_dev (VS_MG_LONGEST) -> glottal_dev on the context's
        stream"""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        assert pcm.ndim == 2
        n, ns = pcm.shape
        mp = ns // 2 + 2 if marks is None else int(marks)
        cyc = None
        if isinstance(cycles, np.ndarray):
            cyc = np.ascontiguousarray(cycles, dtype=GLOTTAL_CYCLE_DTYPE)
            assert cyc.ndim == 2 and cyc.shape[0] == n
        elif cycles:
            cyc = np.zeros((n, int(cycles)), dtype=GLOTTAL_CYCLE_DTYPE)
        with self.scope() as dev:
            d_pcm = dev.put(pcm)
            d_meas = dev.room(n * ACOUSTIC_DTYPE.itemsize)
            d_marks = dev.filled(n * mp, -1, np.int32)
            d_gl = dev.room(n * GLOTTAL_DTYPE.itemsize)
            d_cyc = dev.put(cyc) if cyc is not None else None
            d_fr, fp, d_rec = self._guided_marks_dev(dev, d_pcm, n, ns, fs, lengths, d_meas, d_marks, mp, f0_min, f0_max,
                                                     polarity)
            self.glottal_dev(d_pcm, ns, n, ns, d_meas, d_marks, mp, d_gl, level_open, level_mid, polarity, d_cyc,
                             cyc.shape[1] if cyc is not None else 0)
            self.synchronize()
            res = {"glottal": dev.get(d_gl, (n,), GLOTTAL_DTYPE), "meas": dev.get(d_meas, (n,), ACOUSTIC_DTYPE),
                   "marks": dev.get(d_marks, (n, mp), np.int32), "frames": dev.get(d_fr, (n, fp), PITCH_FRAME_DTYPE),
                   "guided": dev.get(d_rec, (n,), GUIDED_REC_DTYPE)}
            if cyc is not None:
                res["cycles"] = dev.get(d_cyc, cyc.shape, GLOTTAL_CYCLE_DTYPE)
            return res

    def glottal(self, pcm, fs, level_open=26, level_mid=128, polarity=1, f0_min=50, f0_max=500, lengths=None, marks=None,
                cycles=0, guided=False):
        """vs_glottal(): the measurement and, behind it, OQ, ClQ, SQ, QOQ and NAQ of every row of pcm (int16
        [rows][samples]) on the device.  marks: marks_pitch (default: samples // 2 + 2, room for every mark); cycles:
        cycles_pitch, or an array [rows][cycles_pitch] of GLOTTAL_CYCLE_DTYPE whose untouched slots come back as they
        are.  Returns a dict: glottal (GLOTTAL_DTYPE), meas (ACOUSTIC_DTYPE), marks (int32, -1 past the last) and, with
        cycles, cycles.  guided: the marks come from the pitch track and the guided walk (VS_MG_LONGEST; default options
        but f0_min, f0_max and polarity) instead of vs_measure's; the dict gains frames (PITCH_FRAME_DTYPE) and guided
        (GUIDED_REC_DTYPE)."""
        if guided:
            return self._glottal_guided(pcm, fs, level_open, level_mid, polarity, f0_min, f0_max, lengths, marks, cycles)
        pcm, fs, ln = _pcm_rows(pcm, fs, lengths)
        n = pcm.shape[0]
        mp = pcm.shape[1] // 2 + 2 if marks is None else int(marks)
        meas = np.zeros(n, dtype=ACOUSTIC_DTYPE)
        mk = np.full((n, mp), -1, dtype=np.int32)
        out = np.zeros(n, dtype=GLOTTAL_DTYPE)
        cyc = None
        if isinstance(cycles, np.ndarray):
            cyc = np.ascontiguousarray(cycles, dtype=GLOTTAL_CYCLE_DTYPE)
            assert cyc.ndim == 2 and cyc.shape[0] == n
        elif cycles:
            cyc = np.zeros((n, int(cycles)), dtype=GLOTTAL_CYCLE_DTYPE)
        mo, go = measure_opts(f0_min, f0_max, polarity), glottal_opts(level_open, level_mid, polarity)
        check(self._lib.vs_glottal(self._ctx, C.byref(mo), C.byref(go), pcm.ctypes.data, pcm.shape[1], n, pcm.shape[1],
                                   fs.ctypes.data, _ptr(ln), mp, meas.ctypes.data, mk.ctypes.data, out.ctypes.data,
                                   cyc.ctypes.data if cyc is not None else None,
                                   cyc.shape[1] if cyc is not None else 0), "vs_glottal")
        res = {"glottal": out, "meas": meas, "marks": mk}
        if cyc is not None:
            res["cycles"] = cyc
        return res

    def glottal_dev(self, pcm_ptr, pitch, n_lanes, n_samples, meas_ptr, marks_ptr, marks_pitch, out_ptr, level_open=26,
                    level_mid=128, polarity=1, cycles_ptr=None, cycles_pitch=0):
        """vs_glottal_launch(): device pointers (PCM [n_lanes][pitch] int16; the records and marks a measure_dev() before
        it on the context's stream wrote, with the same polarity; records [n_lanes] vs_glottal_rec; cycle records
        [n_lanes][cycles_pitch] or None); returns without waiting.  Nothing is uploaded."""
        o = glottal_opts(level_open, level_mid, polarity)
        check(self._lib.vs_glottal_launch(self._ctx, C.byref(o), C.c_void_p(pcm_ptr), int(pitch), int(n_lanes),
                                          int(n_samples), C.c_void_p(meas_ptr), C.c_void_p(marks_ptr), int(marks_pitch),
                                          C.c_void_p(out_ptr), C.c_void_p(cycles_ptr), int(cycles_pitch)),
              "vs_glottal_launch")

    def _frame_call(self, name, o, frames_of, pcm, fs, lengths, coefs, ins=(), outs=()):
        """what lpc(), iaif() and cplpc() share: the row arrays, n_frames, the filled frame records and output buffers,
        the call and the result dict.  o: the call's options; frames_of(fs, length): the frames of such a row; ins: what
        the C call takes between lengths and frames_pitch; outs: the buffers it takes behind the coefficients, each
        (key, wanted, shape of a frame's entry, dtype, fill)."""
        pcm, fs, ln = _pcm_rows(pcm, fs, lengths, whole=True)
        n = pcm.shape[0]
        shapes = list(zip(fs.tolist(), ln.tolist()))
        per = {key: frames_of(*key) for key in set(shapes)}  # one call per distinct row shape
        nfr = np.array([per[key] for key in shapes], dtype=np.int32)
        fp = max(1, int(nfr.max()))
        fr = _frame_fill(n, fp)
        outs = [("formants", True, (int(o.n_formants), 2), np.float64, np.nan),
                ("coefs", coefs, (int(o.order) + 1,), np.float64, np.nan)] + list(outs)
        bufs = {k: np.full((n, fp) + tail, fill, dtype=dt) for k, wanted, tail, dt, fill in outs if wanted}
        check(getattr(self._lib, name)(self._ctx, C.byref(o), pcm.ctypes.data, pcm.shape[1], n, pcm.shape[1],
                                       fs.ctypes.data, ln.ctypes.data, *ins, fp, fr.ctypes.data,
                                       *[_ptr(bufs.get(k)) for k, *_ in outs]), name)
        out = _frame_result(fr, nfr)
        out.update(bufs)
        return out

    def lpc(self, pcm, fs, lengths=None, coefs=False, **opts):
        """vs_lpc(): LPC analysis of every row of pcm (int16 [rows][samples]) on the device.  fs and lengths: a value per
        row (or one for all); opts: those of lpc_opts().  Returns a dict of arrays over [rows][frames] (frames = the
        largest n_frames): r0, err, start, status, n_formants; n_frames [rows]; formants [rows][frames][n][2] (f, bw in
        Hz); with coefs, coefs [rows][frames][order+1].  Frames past a row's n_frames keep the fill: NaN, start -1,
        status -1."""
        return self._frame_call("vs_lpc", lpc_opts(**opts), lambda f, l: lpc_frames(f, l, **opts), pcm, fs, lengths,
                                coefs)

    def lpc_dev(self, pcm_ptr, pitch, n_lanes, n_samples, fs, frames_pitch, frames_ptr, formants_ptr=None,
                coefs_ptr=None, lengths=None, **opts):
        """vs_lpc_launch(): device pointers (PCM [n_lanes][pitch] int16, records [n_lanes][frames_pitch] vs_lpc_frame,
        formants [n_lanes][frames_pitch][2*n_formants] and coefs [n_lanes][frames_pitch][order+1] doubles, or None),
        enqueued on the context's stream behind what is there -- e.g. a Plan.launch() into pcm_ptr; returns without
        waiting.  fs / lengths: host values, one per row (or one for all)."""
        fs, ln = _row_pair(fs, lengths, n_lanes)
        o = lpc_opts(**opts)
        check(self._lib.vs_lpc_launch(self._ctx, C.byref(o), C.c_void_p(pcm_ptr), int(pitch), int(n_lanes),
                                      int(n_samples), fs.ctypes.data, _ptr(ln), int(frames_pitch),
                                      C.c_void_p(frames_ptr), C.c_void_p(formants_ptr), C.c_void_p(coefs_ptr)),
              "vs_lpc_launch")

    def iaif(self, pcm, fs, lengths=None, coefs=False, glottal=False, **opts):
        """vs_iaif(): IAIF analysis of every row of pcm (int16 [rows][samples]) on the device.  opts: those of
        iaif_opts().  Returns what lpc() returns (coefs: V2) and, with glottal, glottal [rows][frames][glottal_order+1]
        (c2), with the same fill past a row's n_frames."""
        o, ilo = iaif_opts(**opts), iaif_lpc_opts(**opts)
        return self._frame_call("vs_iaif", o, lambda f, l: lpc_frames(f, l, **ilo), pcm, fs, lengths, coefs,
                                outs=[("glottal", glottal, (int(o.glottal_order) + 1,), np.float64, np.nan)])

    def iaif_dev(self, pcm_ptr, pitch, n_lanes, n_samples, fs, frames_pitch, frames_ptr, formants_ptr=None,
                 coefs_ptr=None, glottal_ptr=None, lengths=None, **opts):
        """vs_iaif_launch(): device pointers as lpc_dev(), and glottal [n_lanes][frames_pitch][glottal_order+1] doubles
        or None; enqueued on the context's stream behind what is there, returns without waiting."""
        fs, ln = _row_pair(fs, lengths, n_lanes)
        o = iaif_opts(**opts)
        check(self._lib.vs_iaif_launch(self._ctx, C.byref(o), C.c_void_p(pcm_ptr), int(pitch), int(n_lanes),
                                       int(n_samples), fs.ctypes.data, _ptr(ln), int(frames_pitch),
                                       C.c_void_p(frames_ptr), C.c_void_p(formants_ptr), C.c_void_p(coefs_ptr),
                                       C.c_void_p(glottal_ptr)), "vs_iaif_launch")

    def cplpc(self, pcm, fs, glottal, cycles, lengths=None, coefs=False, counts=False, **opts):
        """vs_cplpc(): closed-phase covariance LPC of every row of pcm (int16 [rows][samples]) on the device.  glottal
        (GLOTTAL_DTYPE [rows]) and cycles (GLOTTAL_CYCLE_DTYPE [rows][cycles_pitch]): what glottal(..., cycles=...)
        returned, typically for a first-pass residual of the same rows.  opts: those of cplpc_opts().  Returns what
        lpc() returns and, with counts, counts int32 [rows][frames][2] = (spans pooled, equations), -1 past a row's
        frames."""
        glottal = np.ascontiguousarray(glottal, dtype=GLOTTAL_DTYPE)
        cycles = np.ascontiguousarray(cycles, dtype=GLOTTAL_CYCLE_DTYPE)
        assert glottal.shape == (np.shape(pcm)[0],) and cycles.ndim == 2 and cycles.shape[0] == glottal.shape[0]
        return self._frame_call("vs_cplpc", cplpc_opts(**opts), lambda f, l: cplpc_frames(f, l, **opts), pcm, fs, lengths,
                                coefs, ins=(glottal.ctypes.data, cycles.ctypes.data, cycles.shape[1]),
                                outs=[("counts", counts, (2,), np.int32, -1)])

    def cplpc_dev(self, pcm_ptr, pitch, n_lanes, n_samples, fs, glottal_ptr, cycles_ptr, cycles_pitch, frames_pitch,
                  frames_ptr, formants_ptr=None, coefs_ptr=None, counts_ptr=None, lengths=None, **opts):
        """vs_cplpc_launch(): device pointers as lpc_dev(); glottal [n_lanes] vs_glottal_rec and cycles
        [n_lanes][cycles_pitch] vs_glottal_cycle as a glottal_dev() before it on the context's stream wrote them; counts
        [n_lanes][frames_pitch][2] int32 or None.  Enqueued on the context's stream, returns without waiting."""
        fs, ln = _row_pair(fs, lengths, n_lanes)
        o = cplpc_opts(**opts)
        check(self._lib.vs_cplpc_launch(self._ctx, C.byref(o), C.c_void_p(pcm_ptr), int(pitch), int(n_lanes),
                                        int(n_samples), fs.ctypes.data, _ptr(ln), C.c_void_p(glottal_ptr),
                                        C.c_void_p(cycles_ptr), int(cycles_pitch), int(frames_pitch),
                                        C.c_void_p(frames_ptr), C.c_void_p(formants_ptr), C.c_void_p(coefs_ptr),
                                        C.c_void_p(counts_ptr)), "vs_cplpc_launch")

    def pitch(self, pcm, fs, lengths=None, frames=None, **opts):
        """vs_pitch(): the pitch track of every row of pcm (int16 [rows][samples]) on the device.  fs and lengths: a value
        per row (or one for all); opts: those of pitch_opts().  frames: frames_pitch (default: the largest n_frames, at
        least 1), or an array [rows][frames_pitch] of PITCH_FRAME_DTYPE whose records past a row's frames come back as
        they are (without one they are zero).  Returns (records [rows][frames_pitch], n_frames [rows])."""
        pcm, fs, ln = _pcm_rows(pcm, fs, lengths, whole=True)
        n = pcm.shape[0]
        shapes = list(zip(fs.tolist(), ln.tolist()))
        per = {key: pitch_frames(*key, **opts) for key in set(shapes)}  # one call per distinct row shape
        nfr = np.array([per[key] for key in shapes], dtype=np.int32)
        if isinstance(frames, np.ndarray):
            fr = np.ascontiguousarray(frames, dtype=PITCH_FRAME_DTYPE).copy()
            assert fr.ndim == 2 and fr.shape[0] == n
        else:
            fr = np.zeros((n, max(1, int(nfr.max())) if frames is None else int(frames)), dtype=PITCH_FRAME_DTYPE)
        o = pitch_opts(**opts)
        check(self._lib.vs_pitch(self._ctx, C.byref(o), pcm.ctypes.data, pcm.shape[1], n, pcm.shape[1], fs.ctypes.data,
                                 ln.ctypes.data, fr.shape[1], fr.ctypes.data), "vs_pitch")
        return fr, nfr

    def pitch_dev(self, pcm_ptr, pitch, n_lanes, n_samples, fs, frames_pitch, frames_ptr, lengths=None, **opts):
        """vs_pitch_launch(): device pointers (PCM [n_lanes][pitch] int16, records [n_lanes][frames_pitch]
        vs_pitch_frame), enqueued on the context's stream behind what is there; returns without waiting.  fs / lengths:
        host values, one per row (or one for all)."""
        fs, ln = _row_pair(fs, lengths, n_lanes)
        o = pitch_opts(**opts)
        check(self._lib.vs_pitch_launch(self._ctx, C.byref(o), C.c_void_p(pcm_ptr), int(pitch), int(n_lanes),
                                        int(n_samples), fs.ctypes.data, _ptr(ln), int(frames_pitch),
                                        C.c_void_p(frames_ptr)), "vs_pitch_launch")

    def closed_phase(self, pcm, fs, f0_min=50, f0_max=500, polarity=1, first_de_emphasis=0.99, de_emphasis=0.0, scale=1.0,
                     level_open=26, level_mid=128, cycles_pitch=None, iaif=None, guided=False, **opts):
        """The whole blind chain on the context's stream, without a host round trip: vs_iaif_launch (iaif: iaif_opts()
        keywords; its order is opts' order, its glottal order 4 or that order if smaller) -> vs_inverse_launch (hold, first_de_emphasis, scale) -> vs_measure_launch ->
        vs_glottal_launch -> vs_cplpc_launch (opts: cplpc_opts() keywords) -> vs_inverse_launch with the closed-phase
        sets (hold, de_emphasis, scale).  pcm: int16 [rows][samples], one rate fs for all rows.  Returns a dict: flow and
        flow_stat (the second inverse), sets (what cplpc(..., coefs=True, counts=True) returns), and the first pass:
        residual, inv_stat, meas, marks, glottal, cycles.  guided: pitch_dev -> measure_guided_dev (VS_MG_LONGEST) on the
        residual stand where vs_measure_launch stands, and the dict gains frames: the residual's pitch track."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        assert pcm.ndim == 2
        n, ns = pcm.shape
        fs = int(fs)
        o = cplpc_opts(**opts)
        p, nf = int(o.order), int(o.n_formants)
        ikw = dict(dict(glottal_order=min(4, p)), **dict(iaif or {}, order=p, n_formants=0))
        ilo = iaif_lpc_opts(**ikw)
        ifp = max(1, lpc_frames(fs, ns, **ilo))
        row1 = inverse_from_lpc(fs, ns, "hold", **ilo)
        row1["scale"], row1["de_emphasis"] = scale, first_de_emphasis
        fp = max(1, cplpc_frames(fs, ns, **opts))
        if o.window_s > 0:
            row2 = inverse_from_lpc(fs, ns, "hold", **cplpc_lpc_opts(**opts))
        else:
            row2 = inverse_rows(1, 1, 1, 0, ns)[0]
        row2["scale"], row2["de_emphasis"] = scale, de_emphasis
        mp = ns // 2 + 2
        cp = mp if cycles_pitch is None else int(cycles_pitch)
        fr = _frame_fill(n, fp)
        with self.scope() as dev:
            d_pcm = dev.put(pcm)
            d_ifr = dev.room(n * ifp * LPC_FRAME_DTYPE.itemsize)
            d_icf = dev.filled(n * ifp * (p + 1), np.nan, np.float64)
            d_res = dev.put(np.zeros((n, ns), dtype=np.int16))
            d_st1 = dev.room(n * INVERSE_STAT_DTYPE.itemsize)
            d_meas = dev.room(n * ACOUSTIC_DTYPE.itemsize)
            d_marks = dev.filled(n * mp, -1, np.int32)
            d_gl = dev.room(n * GLOTTAL_DTYPE.itemsize)
            d_cyc = dev.put(np.zeros((n, cp), dtype=GLOTTAL_CYCLE_DTYPE))
            d_fr = dev.put(fr)
            d_fm = dev.filled(n * fp * nf * 2, np.nan, np.float64)
            d_cf = dev.filled(n * fp * (p + 1), np.nan, np.float64)
            d_cnt = dev.filled(n * fp * 2, -1, np.int32)
            d_flow = dev.put(np.zeros((n, ns), dtype=np.int16))
            d_st2 = dev.room(n * INVERSE_STAT_DTYPE.itemsize)
            self.iaif_dev(d_pcm, ns, n, ns, fs, ifp, d_ifr, None, d_icf, None, **ikw)
            self.inverse_filter_dev("hold", p, d_pcm, ns, d_res, ns, n, ns, row1, d_icf, ifp, d_st1)
            if guided:
                d_ptf, ptfp, _ = self._guided_marks_dev(dev, d_res, n, ns, fs, None, d_meas, d_marks, mp, f0_min, f0_max,
                                                        polarity)
            else:
                self.measure_dev(d_res, ns, n, ns, fs, d_meas, f0_min, f0_max, polarity, None, d_marks, mp)
            self.glottal_dev(d_res, ns, n, ns, d_meas, d_marks, mp, d_gl, level_open, level_mid, polarity, d_cyc, cp)
            self.cplpc_dev(d_pcm, ns, n, ns, fs, d_gl, d_cyc, cp, fp, d_fr, d_fm if nf else None, d_cf, d_cnt, **opts)
            self.inverse_filter_dev("hold", p, d_pcm, ns, d_flow, ns, n, ns, row2, d_cf, fp, d_st2)
            self.synchronize()
            sets = _frame_result(dev.get(d_fr, (n, fp), LPC_FRAME_DTYPE),
                                 np.full(n, cplpc_frames(fs, ns, **opts), dtype=np.int32))
            sets["formants"] = dev.get(d_fm, (n, fp, nf, 2), np.float64) if nf else np.zeros((n, fp, 0, 2))
            sets["coefs"] = dev.get(d_cf, (n, fp, p + 1), np.float64)
            sets["counts"] = dev.get(d_cnt, (n, fp, 2), np.int32)
            res = dict(flow=dev.get(d_flow, (n, ns)), flow_stat=dev.get(d_st2, (n,), INVERSE_STAT_DTYPE), sets=sets,
                       residual=dev.get(d_res, (n, ns)), inv_stat=dev.get(d_st1, (n,), INVERSE_STAT_DTYPE),
                       meas=dev.get(d_meas, (n,), ACOUSTIC_DTYPE), marks=dev.get(d_marks, (n, mp), np.int32),
                       glottal=dev.get(d_gl, (n,), GLOTTAL_DTYPE),
                       cycles=dev.get(d_cyc, (n, cp), GLOTTAL_CYCLE_DTYPE))
            if guided:
                res["frames"] = dev.get(d_ptf, (n, ptfp), PITCH_FRAME_DTYPE)
            return res

    def filter_track(self, flow, coefs, hop, offset=0, n_sets=None, lengths=None, gain=1.0, pre_emphasis=0.0,
                     mode="hold", gains=None, out=None):
        """vs_track(): the all-pole filter with a coefficient track on every row of flow (int16 [rows][samples]).  coefs:
        double [rows][sets][order+1]; hop, offset, n_sets (default: all sets), lengths (default: all samples), gain and
        pre_emphasis: one value or one per row; mode "hold" / "glide"; gains: optional double [rows][sets].  out: an
        int16 array like flow whose samples past a row's length are kept (default: zeros).  Returns (pcm, stat) with
        stat a TRACK_STAT_DTYPE record per row."""
        flow = np.ascontiguousarray(flow, dtype=np.int16)
        coefs = np.ascontiguousarray(coefs, dtype=np.float64)
        assert flow.ndim == 2 and coefs.ndim == 3 and coefs.shape[0] == flow.shape[0]
        n, ns = flow.shape
        sp, order = coefs.shape[1], coefs.shape[2] - 1
        rows = track_rows(n, sp if n_sets is None else n_sets, hop, offset, ns if lengths is None else lengths, gain,
                          pre_emphasis)
        if gains is not None:
            gains = np.ascontiguousarray(gains, dtype=np.float64)
            assert gains.shape == (n, sp)
        pcm = np.zeros_like(flow) if out is None else np.ascontiguousarray(out, dtype=np.int16).copy()
        assert pcm.shape == flow.shape
        stat = np.zeros(n, dtype=TRACK_STAT_DTYPE)
        check(self._lib.vs_track(self._ctx, _track_mode(mode), order, flow.ctypes.data, pcm.ctypes.data, n, ns,
                                 rows.ctypes.data, coefs.ctypes.data, gains.ctypes.data if gains is not None else None,
                                 sp, stat.ctypes.data), "vs_track")
        return pcm, stat

    def filter_track_dev(self, mode, order, flow_ptr, in_pitch, out_ptr, out_pitch, n_lanes, n_samples, rows, coefs_ptr,
                         sets_pitch, gains_ptr=None, stat_ptr=None):
        """vs_track_launch(): device pointers (flow [n_lanes][in_pitch] and PCM [n_lanes][out_pitch] int16, coefs
        [n_lanes][sets_pitch][order+1] and gains [n_lanes][sets_pitch] doubles, stat [n_lanes] vs_track_stat; the last
        two or None), enqueued on the context's stream behind what is there -- e.g. an lpc_dev() into coefs_ptr; returns
        without waiting.  rows: host records (track_rows(), or track_from_lpc() for one row = for all)."""
        rows = np.ascontiguousarray(np.broadcast_to(np.asarray(rows, dtype=TRACK_ROW_DTYPE), (n_lanes,)))
        check(self._lib.vs_track_launch(self._ctx, _track_mode(mode), int(order), C.c_void_p(flow_ptr), int(in_pitch),
                                        C.c_void_p(out_ptr), int(out_pitch), int(n_lanes), int(n_samples),
                                        rows.ctypes.data, C.c_void_p(coefs_ptr), C.c_void_p(gains_ptr), int(sets_pitch),
                                        C.c_void_p(stat_ptr)), "vs_track_launch")

    def source_track(self, lanes, n_samples, period, hop, offset=0, n_frames=None, lengths=None, pmin=2, pmax=2048,
                     amp=None, log_cycles=0, max_reject=256, out=None):
        """vs_strack(): the glottal source of every lane on a period track.  period: int32 [rows][frames] (one row serves
        every lane), amp: optional int32 like period; hop, offset, n_frames (default: all frames), lengths (default: all
        samples), pmin and pmax: one value or one per row.  out: an int16 array [rows][n_samples] whose samples past a
        row's length are kept (default: zeros).  Returns (flow, stat) with stat a STRACK_STAT_DTYPE record per row, and
        with log_cycles also cycles, STRACK_CYCLE_DTYPE [rows][log_cycles] (start -1 past a row's cycles)."""
        arr = _as_lane_array(lanes)
        n, ns = len(arr), int(n_samples)
        period = np.asarray(period, dtype=np.int32)
        period = np.ascontiguousarray(np.broadcast_to(period, (n, period.shape[-1])))
        fp = period.shape[1]
        if amp is not None:
            amp = np.ascontiguousarray(np.broadcast_to(np.asarray(amp, dtype=np.int32), (n, fp)))
        rows = strack_rows(n, fp if n_frames is None else n_frames, hop, offset, ns if lengths is None else lengths, pmin,
                           pmax)
        flow = np.zeros((n, ns), dtype=np.int16) if out is None else np.ascontiguousarray(out, dtype=np.int16).copy()
        assert flow.shape == (n, ns)
        stat = np.zeros(n, dtype=STRACK_STAT_DTYPE)
        cycles = None
        if log_cycles:
            cycles = np.zeros((n, int(log_cycles)), dtype=STRACK_CYCLE_DTYPE)
            cycles["start"] = -1
        check(self._lib.vs_strack(self._ctx, C.byref(strack_opts(max_reject)), arr, n, ns, rows.ctypes.data,
                                  period.ctypes.data, fp, _ptr(amp), flow.ctypes.data, stat.ctypes.data, _ptr(cycles),
                                  int(log_cycles)), "vs_strack")
        return (flow, stat, cycles) if log_cycles else (flow, stat)

    def source_track_dev(self, lanes, n_samples, rows, period_ptr, period_stride, frames_pitch, flow_ptr, out_pitch,
                         stat_ptr, amp_ptr=None, amp_stride=0, cycles_ptr=None, cycles_pitch=0, max_reject=256):
        """vs_strack_launch(): device pointers (the period of frame f of row i is the int32 at byte
        (i*frames_pitch + f) * period_stride of period_ptr -- the lag field of pitch_dev()'s records with stride 96 --,
        amp_ptr likewise or None, flow [n_lanes][out_pitch] int16, stat [n_lanes] vs_strack_stat, cycles
        [n_lanes][cycles_pitch] vs_strack_cycle or None), enqueued on the context's stream behind what is there; returns
        without waiting.  rows: host records (strack_rows(), or strack_row_from_pitch() for one row = for all)."""
        arr = _as_lane_array(lanes)
        rows = np.ascontiguousarray(np.broadcast_to(np.asarray(rows, dtype=STRACK_ROW_DTYPE), (len(arr),)))
        check(self._lib.vs_strack_launch(self._ctx, C.byref(strack_opts(max_reject)), arr, len(arr), int(n_samples),
                                         rows.ctypes.data, C.c_void_p(period_ptr), int(period_stride), int(frames_pitch),
                                         C.c_void_p(amp_ptr), int(amp_stride), C.c_void_p(flow_ptr), int(out_pitch),
                                         C.c_void_p(stat_ptr), C.c_void_p(cycles_ptr), int(cycles_pitch)),
              "vs_strack_launch")

    @staticmethod
    def _psola_inputs(who, pcm, fs, lengths, marks, rec, segs, start, period, gain, count, width, synth, f0_min, f0_max,
                      pmin, pmax, out, synth_fill):
        """What psola() and psola_ts() make of their arguments alike: the rows and their lengths, pmin and pmax, the
        marks and runs, the target broadcast to every row, and the output, status and synthesis records (width: of an
        output row; None: the input's)."""
        pcm, fsr, ln = _pcm_rows(pcm, fs, lengths)
        n, ns = pcm.shape
        if pmin is None or pmax is None:
            if len(set(fsr.tolist())) != 1:
                raise ValueError("%s: rows at several rates need pmin and pmax" % who)
            plan = guided_plan(int(fsr[0]), ns, f0_min=f0_min, f0_max=f0_max)
            pmin, pmax = (plan["tmin"] if pmin is None else pmin), (plan["tmax"] if pmax is None else pmax)
        marks = np.ascontiguousarray(marks, dtype=np.int32)
        rec = np.ascontiguousarray(rec, dtype=GUIDED_REC_DTYPE)
        segs = None if segs is None else np.ascontiguousarray(segs, dtype=GUIDED_SEG_DTYPE)
        assert marks.ndim == 2 and marks.shape[0] == n and rec.shape == (n,) and (segs is None or segs.shape[0] == n)
        start = np.asarray(start, dtype=np.int32)
        tp = start.shape[-1]
        start = np.ascontiguousarray(np.broadcast_to(start, (n, tp)))
        period = np.ascontiguousarray(np.broadcast_to(np.asarray(period, dtype=np.int32), (n, tp)))
        if gain is not None:
            gain = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.int32), (n, tp)))
        count = _row_array(tp if count is None else count, n, "count")
        width = ns if width is None else int(width)
        y = np.zeros((n, width), dtype=np.int16) if out is None else np.ascontiguousarray(out, dtype=np.int16).copy()
        assert y.shape == (n, width)
        sy = (np.zeros((n, int(synth)), dtype=PSOLA_MARK_DTYPE) if synth_fill is None
              else np.ascontiguousarray(synth_fill, dtype=PSOLA_MARK_DTYPE).copy())
        assert sy.shape == (n, int(synth))
        stat = np.zeros(n, dtype=PSOLA_STAT_DTYPE)
        return pcm, ln, pmin, pmax, marks, rec, segs, start, period, gain, count, tp, y, stat, sy

    def psola(self, pcm, fs, marks, rec, start, period, count=None, segs=None, gain=None, lengths=None, synth=512,
              f0_min=50.0, f0_max=500.0, pmin=None, pmax=None, out=None, synth_fill=None):
        """vs_psola(): the cycles of every row of pcm (int16 [rows][samples]) between its marks (int32 [rows][marks_pitch],
        rec GUIDED_REC_DTYPE [rows] and, optionally, segs GUIDED_SEG_DTYPE [rows][seg_pitch], as measure_guided() returns
        them) placed at the target's periods: start and period int32 [rows][target_pitch] (one row serves every row),
        gain likewise or None, count int32 per row (default: all of them).  pmin and pmax default to the lag bounds of
        guided_plan() for f0_min and f0_max at the rate fs, one rate for all rows.  synth: synth_pitch.  out and
        synth_fill: what the output rows and the synthesis records hold before the call (default: zeros).  Returns (y
        int16 [rows][samples], stat PSOLA_STAT_DTYPE [rows], synth PSOLA_MARK_DTYPE [rows][synth])."""
        pcm, ln, pmin, pmax, marks, rec, segs, start, period, gain, count, tp, y, stat, sy = self._psola_inputs(
            "psola", pcm, fs, lengths, marks, rec, segs, start, period, gain, count, None, synth, f0_min, f0_max, pmin, pmax,
            out, synth_fill)
        n, ns = pcm.shape
        check(self._lib.vs_psola(self._ctx, C.byref(psola_opts(pmin, pmax)), pcm.ctypes.data, ns, n, ns, _ptr(ln),
                                 marks.ctypes.data, marks.shape[1], rec.ctypes.data, _ptr(segs),
                                 0 if segs is None else segs.shape[1], start.ctypes.data, period.ctypes.data, _ptr(gain),
                                 count.ctypes.data, tp, y.ctypes.data, stat.ctypes.data, sy.ctypes.data, int(synth)),
              "vs_psola")
        return y, stat, sy

    def psola_dev(self, pcm_ptr, pitch, n_lanes, n_samples, marks_ptr, marks_pitch, rec_ptr, start_ptr, start_stride,
                  period_ptr, period_stride, count_ptr, count_stride, target_pitch, out_ptr, out_pitch, stat_ptr,
                  synth_ptr, synth_pitch, segs_ptr=None, seg_pitch=0, gain_ptr=None, gain_stride=0, lengths=None,
                  pmin=None, pmax=None):
        """vs_psola_launch(): device pointers (PCM [n_lanes][pitch] int16; marks [n_lanes][marks_pitch] int32, rec
        [n_lanes] vs_guided_rec and segs [n_lanes][seg_pitch] vs_guided_seg or None, as measure_guided_dev() before it
        on the context's stream wrote them; the target read in place -- start[j] of row i is the int32 at byte
        (i*target_pitch + j) * start_stride of start_ptr, the period and the gain (or None) likewise, the row's count
        the int32 at byte i * count_stride of count_ptr: the start, T and n_cycles fields of source_track_dev()'s cycle
        log and status records with strides 32, 32 and 24 --; out [n_lanes][out_pitch] int16, which must not overlap
        the PCM; stat [n_lanes] vs_psola_stat; synth [n_lanes][synth_pitch] vs_psola_mark); returns without waiting.
        lengths: host values, one per row (or one for all)."""
        ln = None if lengths is None else _row_array(lengths, n_lanes, "lengths")
        check(self._lib.vs_psola_launch(self._ctx, C.byref(psola_opts(pmin, pmax)), C.c_void_p(pcm_ptr), int(pitch),
                                        int(n_lanes), int(n_samples), _ptr(ln), C.c_void_p(marks_ptr), int(marks_pitch),
                                        C.c_void_p(rec_ptr), C.c_void_p(segs_ptr), int(seg_pitch), C.c_void_p(start_ptr),
                                        int(start_stride), C.c_void_p(period_ptr), int(period_stride),
                                        C.c_void_p(gain_ptr), int(gain_stride), C.c_void_p(count_ptr), int(count_stride),
                                        int(target_pitch), C.c_void_p(out_ptr), int(out_pitch), C.c_void_p(stat_ptr),
                                        C.c_void_p(synth_ptr), int(synth_pitch)), "vs_psola_launch")

    def psola_ts(self, pcm, fs, marks, rec, start, period, anchors, n_anchors, out_samples, out_lengths=None, count=None,
                 segs=None, gain=None, lengths=None, synth=512, f0_min=50.0, f0_max=500.0, pmin=None, pmax=None,
                 unvoiced_period=None, out=None, synth_fill=None):
        """vs_psola_ts(): psola() with a time map, so that the duration changes too.  As psola(), and: anchors
        PSOLA_ANCHOR_DTYPE [rows][map_pitch] with n_anchors int32 per row (psola_two_anchors() for a uniform change),
        out_samples the width of the output rows, out_lengths per row (default: out_samples), unvoiced_period in samples
        (default 80).  Returns (y int16 [rows][out_samples], stat PSOLA_STAT_DTYPE [rows], synth PSOLA_MARK_DTYPE
        [rows][synth])."""
        pcm, ln, pmin, pmax, marks, rec, segs, start, period, gain, count, tp, y, stat, sy = self._psola_inputs(
            "psola_ts", pcm, fs, lengths, marks, rec, segs, start, period, gain, count, out_samples, synth, f0_min, f0_max,
            pmin, pmax, out, synth_fill)
        n, ns = pcm.shape
        nout = y.shape[1]
        anchors = np.ascontiguousarray(anchors, dtype=PSOLA_ANCHOR_DTYPE)
        assert anchors.ndim == 2 and anchors.shape[0] == n
        n_anchors = _row_array(n_anchors, n, "n_anchors")
        lo = None if out_lengths is None else _row_array(out_lengths, n, "out_lengths")
        check(self._lib.vs_psola_ts(self._ctx, C.byref(psola_ts_opts(pmin, pmax, unvoiced_period)), pcm.ctypes.data, ns, n,
                                    ns, _ptr(ln), marks.ctypes.data, marks.shape[1], rec.ctypes.data, _ptr(segs),
                                    0 if segs is None else segs.shape[1], start.ctypes.data, period.ctypes.data,
                                    _ptr(gain), count.ctypes.data, tp, anchors.ctypes.data, n_anchors.ctypes.data,
                                    anchors.shape[1], y.ctypes.data, nout, _ptr(lo), stat.ctypes.data, sy.ctypes.data,
                                    int(synth)), "vs_psola_ts")
        return y, stat, sy

    def psola_ts_dev(self, pcm_ptr, pitch, n_lanes, n_samples, marks_ptr, marks_pitch, rec_ptr, start_ptr, start_stride,
                     period_ptr, period_stride, count_ptr, count_stride, target_pitch, map_ptr, map_count_ptr, map_pitch,
                     out_ptr, out_pitch, out_samples, stat_ptr, synth_ptr, synth_pitch, segs_ptr=None, seg_pitch=0,
                     gain_ptr=None, gain_stride=0, lengths=None, out_lengths=None, pmin=None, pmax=None,
                     unvoiced_period=None):
        """vs_psola_ts_launch(): device pointers as psola_dev(), and: map [n_lanes][map_pitch] vs_psola_anchor with
        map_count int32 [n_lanes]; out [n_lanes][out_pitch] int16 of out_samples samples a row, which must not overlap
        the PCM; returns without waiting.  lengths and out_lengths: host values, one per row (or one for all)."""
        ln = None if lengths is None else _row_array(lengths, n_lanes, "lengths")
        lo = None if out_lengths is None else _row_array(out_lengths, n_lanes, "out_lengths")
        check(self._lib.vs_psola_ts_launch(self._ctx, C.byref(psola_ts_opts(pmin, pmax, unvoiced_period)),
                                           C.c_void_p(pcm_ptr), int(pitch), int(n_lanes), int(n_samples), _ptr(ln),
                                           C.c_void_p(marks_ptr), int(marks_pitch), C.c_void_p(rec_ptr),
                                           C.c_void_p(segs_ptr), int(seg_pitch), C.c_void_p(start_ptr), int(start_stride),
                                           C.c_void_p(period_ptr), int(period_stride), C.c_void_p(gain_ptr),
                                           int(gain_stride), C.c_void_p(count_ptr), int(count_stride), int(target_pitch),
                                           C.c_void_p(map_ptr), C.c_void_p(map_count_ptr), int(map_pitch),
                                           C.c_void_p(out_ptr), int(out_pitch), int(out_samples), _ptr(lo),
                                           C.c_void_p(stat_ptr), C.c_void_p(synth_ptr), int(synth_pitch)),
              "vs_psola_ts_launch")

    def inverse_filter(self, pcm, coefs, hop, offset=0, n_sets=None, lengths=None, scale=1.0, de_emphasis=0.0,
                       mode="hold", out=None):
        """vs_inverse(): A(z) as an FIR filter behind the de-emphasis on every row of pcm (int16 [rows][samples]): the
        inverse of filter_track() with the same coefs, hop, offset, n_sets and mode, scale = 1 / gain and de_emphasis =
        pre_emphasis.  coefs: double [rows][sets][order+1]; hop, offset, n_sets (default: all sets), lengths (default: all
        samples), scale and de_emphasis: one value or one per row.  out: an int16 array like pcm whose samples past a
        row's length are kept (default: zeros).  Returns (flow, stat) with stat an INVERSE_STAT_DTYPE record per row."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        coefs = np.ascontiguousarray(coefs, dtype=np.float64)
        assert pcm.ndim == 2 and coefs.ndim == 3 and coefs.shape[0] == pcm.shape[0]
        n, ns = pcm.shape
        sp, order = coefs.shape[1], coefs.shape[2] - 1
        rows = inverse_rows(n, sp if n_sets is None else n_sets, hop, offset, ns if lengths is None else lengths, scale,
                            de_emphasis)
        flow = np.zeros_like(pcm) if out is None else np.ascontiguousarray(out, dtype=np.int16).copy()
        assert flow.shape == pcm.shape
        stat = np.zeros(n, dtype=INVERSE_STAT_DTYPE)
        check(self._lib.vs_inverse(self._ctx, _track_mode(mode), order, pcm.ctypes.data, flow.ctypes.data, n, ns,
                                   rows.ctypes.data, coefs.ctypes.data, sp, stat.ctypes.data), "vs_inverse")
        return flow, stat

    def inverse_filter_dev(self, mode, order, pcm_ptr, in_pitch, out_ptr, out_pitch, n_lanes, n_samples, rows, coefs_ptr,
                           sets_pitch, stat_ptr=None):
        """vs_inverse_launch(): device pointers (speech [n_lanes][in_pitch] and flow [n_lanes][out_pitch] int16, which
        must not overlap, coefs [n_lanes][sets_pitch][order+1] doubles, stat [n_lanes] vs_inverse_stat or None), enqueued
        on the context's stream behind what is there -- e.g. an lpc_dev() into coefs_ptr; returns without waiting.
        rows: host records (inverse_rows(), or inverse_from_lpc() for one row = for all)."""
        rows = np.ascontiguousarray(np.broadcast_to(np.asarray(rows, dtype=INVERSE_ROW_DTYPE), (n_lanes,)))
        check(self._lib.vs_inverse_launch(self._ctx, _track_mode(mode), int(order), C.c_void_p(pcm_ptr), int(in_pitch),
                                          C.c_void_p(out_ptr), int(out_pitch), int(n_lanes), int(n_samples),
                                          rows.ctypes.data, C.c_void_p(coefs_ptr), int(sets_pitch),
                                          C.c_void_p(stat_ptr)), "vs_inverse_launch")

    # ---- device-pointer path ----
    def plan(self, lanes, n_samples):
        return Plan(self, lanes, n_samples)

    def scope(self):
        """a DeviceScope: `with engine.scope() as dev:` owns the buffers and plans made through dev"""
        return DeviceScope(self)

    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        check(self._lib.vs_dev_alloc(self._ctx, nbytes, C.byref(p)), "vs_dev_alloc")
        return p.value

    def dev_free(self, ptr):
        check(self._lib.vs_dev_free(self._ctx, C.c_void_p(ptr)), "vs_dev_free")

    def dev_download(self, ptr, shape, dtype=np.int16):
        out = np.empty(shape, dtype=dtype)
        check(self._lib.vs_dev_download(self._ctx, out.ctypes.data, C.c_void_p(ptr), out.nbytes),
              "vs_dev_download")
        return out

    def dev_upload(self, ptr, array):
        array = np.ascontiguousarray(array)
        check(self._lib.vs_dev_upload(self._ctx, C.c_void_p(ptr), array.ctypes.data, array.nbytes),
              "vs_dev_upload")


class Node(_Closing):
    """A vs_node: one batch over several devices (or logical shards of one device)."""

    OVERLAP = 1
    STAGE_ALL = 2

    def __init__(self, devices, arith=VS_ARITH_EXACT):
        self._lib = load()
        self._node = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        check(self._lib.vs_node_create(arr, len(devices), C.byref(self._node)), "vs_node_create")
        check(self._lib.vs_node_set_arith(self._node, int(arith)), "vs_node_set_arith")
        self.shards = len(devices)

    def close(self):
        if self._node:
            self._lib.vs_node_destroy(self._node)
            self._node = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    TRANSPORT_PEER, TRANSPORT_RCCL = 0, 1
    LINKS = {0: "self", 1: "peer", 2: "staged", 3: "rccl"}

    def set_transport(self, transport):
        """vs_node_set_transport(): peer DMA (default) or one RCCL communicator owned by the node"""
        check(self._lib.vs_node_set_transport(self._node, int(transport)), "vs_node_set_transport")

    def link(self, shard):
        """how the shard's PCM reaches the root: 'self', 'peer', 'staged' (through host memory), 'rccl'"""
        v = self._lib.vs_node_link(self._node, int(shard))
        if v < 0:
            raise VsError(v, "vs_node_link")
        return self.LINKS[v]

    def rccl_ranks(self, shard):
        """vs_node_rccl_ranks(): ncclCommCount of the shard's communicator (0 on the peer transport)"""
        v = self._lib.vs_node_rccl_ranks(self._node, int(shard))
        if v < 0:
            raise VsError(v, "vs_node_rccl_ranks")
        return v

    def last_rccl_error(self):
        """vs_node_last_rccl_error(): the ncclResult_t of the last failing RCCL call (0: none)"""
        return int(self._lib.vs_node_last_rccl_error(self._node))

    def set_shard_tuning(self, shard, **kw):
        """vs_ctx_set_tuning() on the context that serves one shard (vs_node_ctx); no keywords resets"""
        ctx = C.c_void_p()
        check(self._lib.vs_node_ctx(self._node, int(shard), C.byref(ctx)), "vs_node_ctx")
        if not kw:
            check(self._lib.vs_ctx_set_tuning(ctx, None), "vs_ctx_set_tuning")
            return
        t = Tuning()
        for k, v in kw.items():
            setattr(t, k, int(v))
        check(self._lib.vs_ctx_set_tuning(ctx, C.byref(t)), "vs_ctx_set_tuning")

    def shard_range(self, n_lanes, shard):
        lo, hi = C.c_size_t(), C.c_size_t()
        check(self._lib.vs_node_shard_range(self._node, n_lanes, shard, C.byref(lo), C.byref(hi)), "vs_node_shard_range")
        return lo.value, hi.value

    def synth_gather(self, lanes, n_samples, root_ptr, root_pitch, flags=1):
        """PCM of all shards gathered into device memory of the root; returns (total_ms, max_compute_ms)"""
        arr = _as_lane_array(lanes)
        tot, comp = C.c_double(), C.c_double()
        check(self._lib.vs_node_synth_gather(self._node, arr, len(arr), n_samples, C.c_void_p(root_ptr), root_pitch,
                                             int(flags), C.byref(tot), C.byref(comp)), "vs_node_synth_gather")
        return tot.value, comp.value

    def synth_rows(self, lanes, n_samples, fn):
        arr = _as_lane_array(lanes)

        def tramp(user, row0, rows, ptr):
            try:
                buf = (C.c_int16 * (rows * n_samples)).from_address(ptr)
                return int(fn(int(row0), np.frombuffer(buf, dtype=np.int16).reshape(rows, n_samples)) or 0)
            except Exception:  # pragma: no cover
                return 1

        cb = _ffi.ROWS_CB(tramp)
        check(self._lib.vs_node_synth_rows(self._node, arr, len(arr), n_samples, cb, None), "vs_node_synth_rows")


class Plan(_Closing):
    """A vs_plan: lane records + cos tables resident on the device; launches are asynchronous."""

    def __init__(self, engine, lanes, n_samples):
        self.engine = engine
        self._lib = engine._lib
        arr = _as_lane_array(lanes)
        self.n_lanes = len(arr)
        self.n_samples = int(n_samples)
        self._plan = C.c_void_p()
        check(self._lib.vs_plan_create(engine._ctx, arr, len(arr), n_samples, C.byref(self._plan)),
              "vs_plan_create")

    def timing(self):
        """(host_ms, upload_ms) of vs_plan_create for this plan"""
        h, u = C.c_double(), C.c_double()
        check(self._lib.vs_plan_timing(self._plan, C.byref(h), C.byref(u)), "vs_plan_timing")
        return h.value, u.value

    def kernel_name(self, kind=VS_KIND_SYNTH):
        buf = C.create_string_buffer(128)
        check(self._lib.vs_plan_kernel_name(self._plan, int(kind), buf, 128), "vs_plan_kernel_name")
        return buf.value.decode()

    def roles(self):
        """vs_plan_roles(): wavefronts per 64 utterances of the fused kind (1 = the one-wave kernel), the layout, and whether
        the plan fell back from three roles to two because the wavefronts are not dealt w % 4"""
        r, l, f = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.vs_plan_roles(self._plan, C.byref(r), C.byref(l), C.byref(f)), "vs_plan_roles")
        return {"roles": r.value, "layout": "spread" if l.value else "role-major", "simd_fallback": bool(f.value)}

    def reseed(self, seeds, out_seeds=None):
        """vs_plan_reseed(): the same utterances with new draws -- seeds[i] (uint64) belongs to lane i of the plan's lane array"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert seeds.shape == (self.n_lanes,)
        if out_seeds is not None:
            out_seeds = np.ascontiguousarray(out_seeds, dtype=np.uint64)
            assert out_seeds.shape == (self.n_lanes,)
        check(self._lib.vs_plan_reseed(self._plan, seeds.ctypes.data, out_seeds.ctypes.data if out_seeds is not None else None),
              "vs_plan_reseed")

    def info(self):
        lds, wgs, slots = C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(self._lib.vs_plan_info(self._plan, C.byref(lds), C.byref(wgs), C.byref(slots)), "vs_plan_info")
        return {"lds_bytes": lds.value, "workgroups": wgs.value, "ring_slots": slots.value}

    def launch(self, kind, out_ptr, out_pitch=None, in_ptr=None, in_pitch=None, log_ptr=None,
               log_pitch=0, ncyc_ptr=None):
        out_pitch = self.n_samples if out_pitch is None else out_pitch
        in_pitch = self.n_samples if in_pitch is None else in_pitch
        check(
            self._lib.vs_plan_launch(self._plan, int(kind), C.c_void_p(in_ptr), in_pitch,
                                     C.c_void_p(out_ptr), out_pitch, C.c_void_p(log_ptr), log_pitch,
                                     C.c_void_p(ncyc_ptr)),
            "vs_plan_launch",
        )

    def status(self):
        """Waits for the stream; raises VsError(VS_ERR_INTERNAL) if a device-side wait ran out."""
        flags = C.c_int()
        check(self._lib.vs_plan_status(self._plan, C.byref(flags)), "vs_plan_status")
        return flags.value

    def close(self):
        if self._plan:
            self._lib.vs_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
