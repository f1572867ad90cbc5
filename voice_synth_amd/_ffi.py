"""ctypes binding of include/voice_synth.h (the C ABI of libvoicesynth.so).

Python is only the test / bench driver of this repository; the host side of the product is C
(voice_synth_amd/csrc, voice_synth_amd/cli).  This module therefore does nothing but declare
the entry points and fail loudly when the library is missing: there is no Python or CPU
fallback for any of them.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", os.environ.get("VS_LIB", "libvoicesynth.so"))  # VS_LIB: A/B builds in tools/

VS_ORDER = 22
VS_NCOEF = 23
VS_MAX_ORDER = 40
VS_MAX_NCOEF = 41

VS_OK = 0
VS_ERR_ARG = -1
VS_ERR_RANGE = -2
VS_ERR_UNSUPPORTED = -3
VS_ERR_HIP = -4
VS_ERR_NOMEM = -5
VS_ERR_NODEVICE = -6
VS_ERR_IO = -7
VS_USAGE = -8
VS_ERR_INTERNAL = -9

VS_FLAG_JITTER = 0x1
VS_FLAG_SHIMMER = 0x2
VS_FLAG_NOISE = 0x4

VS_ARITH_EXACT = 0
VS_ARITH_FMA = 1
VS_ARITH_F32 = 2

VS_KIND_SYNTH = 0
VS_KIND_SOURCE = 1
VS_KIND_FILTER = 2


class Lane(C.Structure):
    """struct vs_lane"""

    _fields_ = [
        ("jitter", C.c_float),
        ("cq", C.c_float),
        ("K", C.c_float),
        ("Fg", C.c_float),
        ("F0", C.c_float),
        ("DC", C.c_float),
        ("noise", C.c_float),
        ("Kvar", C.c_float),
        ("shimmer", C.c_float),
        ("fs", C.c_int32),
        ("amp", C.c_int32),
        ("flags", C.c_uint32),
        ("seed", C.c_uint64),
        ("gain", C.c_float),
        ("pre_emphasis", C.c_float),
        ("vowel", C.c_int32),
        ("out_snr", C.c_float),
        ("A", C.c_double * VS_MAX_NCOEF),
        ("order", C.c_int32),
        ("reserved_", C.c_int32),
        ("out_seed", C.c_uint64),
    ]


class CycleRec(C.Structure):
    """struct vs_cycle_rec"""

    _fields_ = [("S", C.c_float), ("x_pow", C.c_float), ("w_pow", C.c_float), ("T", C.c_int32)]


class FlowgenCmd(C.Structure):
    _fields_ = [("lane", Lane), ("dur", C.c_float), ("wav_arg", C.c_int)]


class VowelCmd(C.Structure):
    _fields_ = [
        ("gain", C.c_float),
        ("pre_emphasis", C.c_float),
        ("snr", C.c_float),
        ("vowel", C.c_int),
        ("input_arg", C.c_int),
        ("output_arg", C.c_int),
        ("noise_arg", C.c_int),
    ]


class DevLane(C.Structure):
    """struct VsDevLane of csrc/vs_device.h (host expansion of a lane; CPU-side tests only)."""

    _fields_ = [
        ("gain", C.c_double),
        ("pre", C.c_double),
        ("jitter", C.c_float),
        ("shimmer", C.c_float),
        ("K", C.c_float),
        ("Kvar", C.c_float),
        ("DC", C.c_float),
        ("noise", C.c_float),
        ("t_hi", C.c_float),
        ("t_lo", C.c_float),
        ("a_hi", C.c_float),
        ("a_lo", C.c_float),
        ("amp", C.c_int32),
        ("P", C.c_int32),
        ("T2", C.c_int32),
        ("tab_off", C.c_int32),
        ("tbound", C.c_int32),
        ("dcs", C.c_int32),
        ("flags", C.c_uint32),
        ("key0", C.c_uint32),
        ("key1", C.c_uint32),
        ("row", C.c_int32),
        ("out_snr", C.c_float),
        ("Lframe", C.c_int32),
        ("okey0", C.c_uint32),
        ("okey1", C.c_uint32),
        ("thr", C.c_int32),
        ("ready_min", C.c_int32),
        ("tap_row", C.c_int32),
        ("lframe_magic", C.c_uint32),
    ]


class Tuning(C.Structure):
    """struct vs_tuning (all zero = the library's own choices)"""

    _fields_ = [
        ("kernel", C.c_int32),
        ("ring_slots", C.c_int32),
        ("ready_min", C.c_int32),
        ("ws_pairs", C.c_int32),
        ("gen_low", C.c_int32),
        ("gen_min", C.c_int32),
        ("spin_limit", C.c_int32),
        ("fault", C.c_int32),
        ("ws_filter_prio", C.c_int32),
        ("ws_roles", C.c_int32),
        ("mixed_rings", C.c_int32),
    ]


class MeasureOpts(C.Structure):
    """struct vs_measure_opts"""

    _fields_ = [("f0_min", C.c_float), ("f0_max", C.c_float), ("polarity", C.c_int32), ("reserved_", C.c_int32)]


class Acoustic(C.Structure):
    """struct vs_acoustic (96 bytes)"""

    _fields_ = [(n, C.c_double) for n in ("f0_hz", "jitter_local", "jitter_abs_s", "jitter_rap", "jitter_ppq5",
                                          "shimmer_local", "shimmer_db", "shimmer_apq3", "shimmer_apq5", "hnr_db")] + \
               [(n, C.c_int32) for n in ("p0", "n_periods", "first_mark", "status")]


class GlottalOpts(C.Structure):
    """struct vs_glottal_opts (16 bytes)"""

    _fields_ = [("level_open", C.c_int32), ("level_mid", C.c_int32), ("polarity", C.c_int32), ("reserved_", C.c_int32)]


class GlottalRec(C.Structure):
    """struct vs_glottal_rec (56 bytes)"""

    _fields_ = [(n, C.c_double) for n in ("oq", "clq", "sq", "qoq", "naq")] + \
               [(n, C.c_int32) for n in ("n_cycles", "n_rejected", "status", "reserved_")]


class GlottalCycle(C.Structure):
    """struct vs_glottal_cycle (48 bytes)"""

    _fields_ = [(n, C.c_int32) for n in ("peak", "period", "trough", "amp", "open", "close", "open_mid", "close_mid",
                                         "gci", "decl", "status", "reserved_")]


class LpcOpts(C.Structure):
    """struct vs_lpc_opts (48 bytes)"""

    _fields_ = [("order", C.c_int32), ("window", C.c_int32), ("pre_emphasis", C.c_int32), ("n_formants", C.c_int32),
                ("window_s", C.c_double), ("hop_s", C.c_double), ("f_lo", C.c_double), ("reserved_", C.c_int64)]


class IaifOpts(C.Structure):
    """struct vs_iaif_opts (56 bytes)"""

    _fields_ = [("order", C.c_int32), ("glottal_order", C.c_int32), ("window", C.c_int32), ("n_formants", C.c_int32),
                ("window_s", C.c_double), ("hop_s", C.c_double), ("f_lo", C.c_double), ("leak", C.c_double),
                ("reserved_", C.c_int64)]


class CplpcOpts(C.Structure):
    """struct vs_cplpc_opts (56 bytes)"""

    _fields_ = [("order", C.c_int32), ("anchor", C.c_int32), ("delay", C.c_int32), ("span_q", C.c_int32),
                ("min_equations", C.c_int32), ("n_formants", C.c_int32), ("window_s", C.c_double), ("hop_s", C.c_double),
                ("f_lo", C.c_double), ("reserved_", C.c_int64)]


class PitchOpts(C.Structure):
    """struct vs_pitch_opts (40 bytes)"""

    _fields_ = [("f0_min", C.c_float), ("f0_max", C.c_float), ("voicing_q", C.c_int32), ("octave_q", C.c_int32),
                ("jump_q", C.c_int32), ("vuv_q", C.c_int32), ("silence_rms", C.c_int32), ("reserved_", C.c_int32),
                ("hop_s", C.c_double)]


class PitchFrame(C.Structure):
    """struct vs_pitch_frame (96 bytes)"""

    _fields_ = [("r0", C.c_int64), ("start", C.c_int32), ("lag", C.c_int32), ("q", C.c_int32), ("status", C.c_int32),
                ("n_cand", C.c_int32), ("reserved_", C.c_int32), ("cand_lag", C.c_int32 * 7), ("cand_q", C.c_int32 * 7),
                ("back", C.c_uint8 * 8)]


class GuidedOpts(C.Structure):
    """struct vs_guided_opts (32 bytes)"""

    _fields_ = [("f0_min", C.c_float), ("f0_max", C.c_float), ("polarity", C.c_int32), ("segments", C.c_int32),
                ("edge_frames", C.c_int32), ("min_frames", C.c_int32), ("hop_s", C.c_double)]


class GuidedRec(C.Structure):
    """struct vs_guided_rec (16 bytes)"""

    _fields_ = [(n, C.c_int32) for n in ("n_segments", "n_marks", "n_frames_walked", "reserved_")]


class GuidedSeg(C.Structure):
    """struct vs_guided_seg (16 bytes)"""

    _fields_ = [(n, C.c_int32) for n in ("first_frame", "n_frames", "first_mark_index", "n_marks")]


class StrackOpts(C.Structure):
    """struct vs_strack_opts (8 bytes)"""

    _fields_ = [("max_reject", C.c_int32), ("reserved_", C.c_int32)]


class StrackRow(C.Structure):
    """struct vs_strack_row (24 bytes)"""

    _fields_ = [(n, C.c_int32) for n in ("n_frames", "hop", "offset", "length", "pmin", "pmax")]


class StrackCycle(C.Structure):
    """struct vs_strack_cycle (32 bytes)"""

    _fields_ = [("start", C.c_int32), ("T", C.c_int32), ("frame", C.c_int32), ("amp", C.c_int32), ("S", C.c_float),
                ("x_pow", C.c_float), ("w_pow", C.c_float), ("reserved_", C.c_int32)]


class StrackStat(C.Structure):
    """struct vs_strack_stat (24 bytes)"""

    _fields_ = [("status", C.c_int32), ("n_cycles", C.c_int32), ("n_resets", C.c_int32), ("n_unvoiced", C.c_int32),
                ("n_draws", C.c_uint64)]


class PsolaOpts(C.Structure):
    """struct vs_psola_opts (16 bytes)"""

    _fields_ = [("pmin", C.c_int32), ("pmax", C.c_int32), ("reserved_", C.c_int32 * 2)]


class PsolaTsOpts(C.Structure):
    """struct vs_psola_ts_opts (16 bytes)"""

    _fields_ = [("pmin", C.c_int32), ("pmax", C.c_int32), ("unvoiced_period", C.c_int32), ("reserved_", C.c_int32)]


class PsolaAnchor(C.Structure):
    """struct vs_psola_anchor (8 bytes)"""

    _fields_ = [("u", C.c_int32), ("v", C.c_int32)]


class PsolaMark(C.Structure):
    """struct vs_psola_mark (16 bytes)"""

    _fields_ = [(n, C.c_int32) for n in ("t", "k", "cycle", "gain")]


class PsolaStat(C.Structure):
    """struct vs_psola_stat (24 bytes)"""

    _fields_ = [(n, C.c_int32) for n in ("status", "n_runs", "n_runs_done", "n_synth", "n_governed", "n_clipped")]


class TrackRow(C.Structure):
    """struct vs_track_row (24 bytes)"""

    _fields_ = [("n_sets", C.c_int32), ("hop", C.c_int32), ("offset", C.c_int32), ("length", C.c_int32),
                ("gain", C.c_float), ("pre_emphasis", C.c_float)]


class TrackStat(C.Structure):
    """struct vs_track_stat (8 bytes)"""

    _fields_ = [("status", C.c_int32), ("n_unusable", C.c_int32)]


class InverseRow(C.Structure):
    """struct vs_inverse_row (24 bytes)"""

    _fields_ = [("n_sets", C.c_int32), ("hop", C.c_int32), ("offset", C.c_int32), ("length", C.c_int32),
                ("scale", C.c_float), ("de_emphasis", C.c_float)]


class InverseStat(C.Structure):
    """struct vs_inverse_stat (16 bytes)"""

    _fields_ = [("status", C.c_int32), ("n_unusable", C.c_int32), ("n_clipped", C.c_int32), ("reserved_", C.c_int32)]


VS_TRACK_GROUP = 24
VS_TRACK_HOLD = 0
VS_TRACK_GLIDE = 1
VS_TRACK_NO_SET = 0x1
VS_INVERSE_NO_SET = 0x1

VS_LPC_MAX_WINDOW = 16384
VS_LPC_MAX_FORMANTS = 20
VS_LPC_MAX_ITER = 100
VS_LPC_FORMANT_TOL_HZ = 1e-6
VS_LPC_HAMMING = 0
VS_LPC_RECTANGULAR = 1
VS_LPC_SILENT = 0x1
VS_LPC_UNSTABLE = 0x2
VS_LPC_NO_ROOTS = 0x4

VS_AC_MAX_LAG = 2048
VS_AC_TOO_SHORT = 0x1
VS_AC_UNVOICED = 0x2
VS_AC_FEW_PERIODS = 0x4
VS_AC_ZERO_AMPLITUDE = 0x8

VS_GL_NO_CYCLES = 0x1
VS_GL_BAD_MARKS = 0x2
VS_GL_REJECTED = 0x4
VS_GL_ALL_REJECTED = 0x8
VS_GLC_ZERO_AMPLITUDE = 0x1
VS_GLC_NO_CLOSURE = 0x2

VS_CP_ANCHOR_CLOSE = 0
VS_CP_ANCHOR_GCI = 1
VS_CP_ANCHOR_PEAK = 2
VS_CP_FEW_EQUATIONS = 0x10
VS_CP_SINGULAR = 0x20
VS_CP_NOT_MINIMUM_PHASE = 0x40

VS_PT_MAX_CAND = 7
VS_PT_SILENT = 0x1
VS_PT_UNVOICED = 0x2
VS_PT_NO_CANDIDATE = 0x4
VS_PT_MAX_COST = 1 << 20
VS_MG_ALL = 0
VS_MG_LONGEST = 1
VS_MG_MAX_EDGE = 16

VS_ST_NO_VOICED = 0x1
VS_ST_INTERNAL = 0x2
VS_ST_MAX_REJECT = 65536

VS_PS_BAD_RUN = 0x1
VS_PS_OVERFLOW = 0x2
VS_PS_NO_RUN = 0x4
VS_PS_RUN_END = -2
VS_PS_BAD_MAP = 0x8
VS_PS_UNVOICED = -3
VS_PS_UNVOICED_FLIP = -4

VS_KERNEL_AUTO = 0
VS_KERNEL_SINGLE = 1
VS_KERNEL_WS = 2
VS_FAULT_WITHHOLD_PROGRESS = 1
VS_FAULT_SHORT_COS_ROWS = 2
VS_FAULT_SHARD_PREPARE = 3
VS_FAULT_SHARD_HANDOVER = 4
VS_FAULT_SIMD_DEALING = 5
VS_FAULT_REROUND = 6
VS_DF_FAST = 0x8


# every symbol include/voice_synth.h declares: (restype, argtypes)
_P = C.POINTER
_vp = C.c_void_p
SYMBOLS = {
    "vs_lane_defaults": (C.c_int, [_P(Lane)]),
    "vs_num_samples": (C.c_int, [C.c_int32, C.c_float, _P(C.c_uint64)]),
    "vs_row_pitch": (C.c_size_t, [C.c_size_t]),
    "vs_vowel_coefficients": (C.c_int, [C.c_int, _P(C.c_double)]),
    "vs_lane_order": (C.c_int, [_P(Lane), _P(C.c_int)]),
    "vs_vowel_name": (C.c_char_p, [C.c_int]),
    "vs_lane_validate": (C.c_int, [_P(Lane)]),
    "vs_strerror": (C.c_char_p, [C.c_int]),
    "vs_flowgen_parse": (C.c_int, [C.c_int, _P(C.c_char_p), _P(FlowgenCmd)]),
    "vs_vowel_parse": (C.c_int, [C.c_int, _P(C.c_char_p), _P(VowelCmd)]),
    "vs_wav_header_write": (C.c_int, [_vp, C.c_int, C.c_int32, C.c_float]),
    "vs_wav_header_read": (
        C.c_int,
        [_vp, C.c_size_t, _P(C.c_int32), _P(C.c_int), _P(C.c_int), _P(C.c_uint64)],
    ),
    "vs_ctx_create": (C.c_int, [C.c_int, _P(_vp)]),
    "vs_ctx_destroy": (None, [_vp]),
    "vs_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "vs_ctx_set_arith": (C.c_int, [_vp, C.c_int]),
    "vs_ctx_last_hip_error": (C.c_int, [_vp]),
    "vs_ctx_set_tuning": (C.c_int, [_vp, _P(Tuning)]),
    "vs_ctx_selftest": (C.c_int, [_vp, _P(C.c_uint64)]),
    "vs_ctx_simd_dealing": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "vs_plan_roles": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "vs_ctx_device_info": (C.c_int, [_vp, C.c_char_p, C.c_size_t, _P(C.c_int)]),
    "vs_ctx_device_pci": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "vs_plan_create": (C.c_int, [_vp, _P(Lane), C.c_size_t, C.c_size_t, _P(_vp)]),
    "vs_plan_destroy": (None, [_vp]),
    "vs_plan_launch": (
        C.c_int,
        [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp],
    ),
    "vs_ctx_synchronize": (C.c_int, [_vp]),
    "vs_ctx_timer_mark": (C.c_int, [_vp, C.c_int]),
    "vs_ctx_timer_elapsed": (C.c_int, [_vp, _P(C.c_double)]),
    "vs_plan_status": (C.c_int, [_vp, _P(C.c_int)]),
    "vs_plan_reseed": (C.c_int, [_vp, _vp, _vp]),
    "vs_plan_info": (C.c_int, [_vp, _P(C.c_size_t), _P(C.c_size_t), _P(C.c_size_t)]),
    "vs_synth": (C.c_int, [_vp, _P(Lane), C.c_size_t, C.c_size_t, _vp]),
    "vs_synth_rows": (C.c_int, [_vp, _P(Lane), C.c_size_t, C.c_size_t, _vp, _vp]),
    "vs_node_create": (C.c_int, [_P(C.c_int), C.c_int, _P(_vp)]),
    "vs_node_destroy": (None, [_vp]),
    "vs_node_shards": (C.c_int, [_vp]),
    "vs_node_ctx": (C.c_int, [_vp, C.c_int, _P(_vp)]),
    "vs_node_set_arith": (C.c_int, [_vp, C.c_int]),
    "vs_node_shard_range": (C.c_int, [_vp, C.c_size_t, C.c_int, _P(C.c_size_t), _P(C.c_size_t)]),
    "vs_node_set_transport": (C.c_int, [_vp, C.c_int]),
    "vs_node_link": (C.c_int, [_vp, C.c_int]),
    "vs_node_last_rccl_error": (C.c_int, [_vp]),
    "vs_node_rccl_ranks": (C.c_int, [_vp, C.c_int]),
    "vs_node_synth_gather": (
        C.c_int,
        [_vp, _P(Lane), C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_int, _P(C.c_double), _P(C.c_double)],
    ),
    "vs_node_synth_rows": (C.c_int, [_vp, _P(Lane), C.c_size_t, C.c_size_t, _vp, _vp]),
    "vs_host_alloc": (C.c_int, [_vp, C.c_size_t, _P(_vp)]),
    "vs_host_free": (C.c_int, [_vp, _vp]),
    "vs_ctx_trim": (C.c_int, [_vp]),
    "vs_plan_timing": (C.c_int, [_vp, _P(C.c_double), _P(C.c_double)]),
    "vs_plan_kernel_name": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_size_t]),
    "vs_source": (
        C.c_int,
        [_vp, _P(Lane), C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp],
    ),
    "vs_filter": (C.c_int, [_vp, _P(Lane), C.c_size_t, C.c_size_t, _vp, _vp]),
    "vs_dev_alloc": (C.c_int, [_vp, C.c_size_t, _P(_vp)]),
    "vs_dev_free": (C.c_int, [_vp, _vp]),
    "vs_dev_upload": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "vs_dev_download": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "vs_measure_defaults": (C.c_int, [_P(MeasureOpts)]),
    "vs_measure_launch": (
        C.c_int,
        [_vp, _P(MeasureOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t],
    ),
    "vs_measure": (
        C.c_int,
        [_vp, _P(MeasureOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t],
    ),
    "vs_lpc_defaults": (C.c_int, [_P(LpcOpts)]),
    "vs_lpc_frames": (C.c_int, [_P(LpcOpts), C.c_int32, C.c_int32, _P(C.c_int32)]),
    "vs_lpc_window": (C.c_int, [C.c_int32, C.c_int32, _vp]),
    "vs_lpc_launch": (
        C.c_int,
        [_vp, _P(LpcOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp],
    ),
    "vs_lpc": (
        C.c_int,
        [_vp, _P(LpcOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp],
    ),
    "vs_iaif_defaults": (C.c_int, [_P(IaifOpts)]),
    "vs_iaif_lpc_opts": (C.c_int, [_P(IaifOpts), _P(LpcOpts)]),
    "vs_iaif_launch": (
        C.c_int,
        [_vp, _P(IaifOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp],
    ),
    "vs_iaif": (
        C.c_int,
        [_vp, _P(IaifOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp],
    ),
    "vs_track_launch": (
        C.c_int,
        [_vp, C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp],
    ),
    "vs_track": (
        C.c_int,
        [_vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp],
    ),
    "vs_track_reflection": (C.c_int, [C.c_int, _vp, _vp]),
    "vs_track_glide_sets": (C.c_int, [C.c_int, _vp, _vp, C.c_int, _vp]),
    "vs_track_from_lpc": (C.c_int, [_P(LpcOpts), C.c_int32, C.c_int32, C.c_int, _P(TrackRow)]),
    "vs_inverse_launch": (
        C.c_int,
        [_vp, C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp],
    ),
    "vs_inverse": (
        C.c_int,
        [_vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp],
    ),
    "vs_inverse_from_lpc": (C.c_int, [_P(LpcOpts), C.c_int32, C.c_int32, C.c_int, _P(InverseRow)]),
    "vs_glottal_defaults": (C.c_int, [_P(GlottalOpts)]),
    "vs_glottal_launch": (
        C.c_int,
        [_vp, _P(GlottalOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t],
    ),
    "vs_glottal": (
        C.c_int,
        [_vp, _P(MeasureOpts), _P(GlottalOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp,
         _vp, _vp, C.c_size_t],
    ),
    "vs_cplpc_defaults": (C.c_int, [_P(CplpcOpts)]),
    "vs_cplpc_frames": (C.c_int, [_P(CplpcOpts), C.c_int32, C.c_int32, _P(C.c_int32)]),
    "vs_cplpc_lpc_opts": (C.c_int, [_P(CplpcOpts), _P(LpcOpts)]),
    "vs_cplpc_launch": (
        C.c_int,
        [_vp, _P(CplpcOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp,
         _vp, _vp],
    ),
    "vs_cplpc": (
        C.c_int,
        [_vp, _P(CplpcOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp,
         _vp, _vp],
    ),
    "vs_pitch_defaults": (C.c_int, [_P(PitchOpts)]),
    "vs_pitch_frames": (C.c_int, [_P(PitchOpts), C.c_int32, C.c_int32, _P(C.c_int32)]),
    "vs_pitch_log2_table": (C.c_int, [C.c_int32, _vp]),
    "vs_pitch_launch": (
        C.c_int,
        [_vp, _P(PitchOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp],
    ),
    "vs_pitch": (
        C.c_int,
        [_vp, _P(PitchOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp],
    ),
    "vs_guided_defaults": (C.c_int, [_P(GuidedOpts)]),
    "vs_guided_plan": (
        C.c_int,
        [_P(GuidedOpts), C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)],
    ),
    "vs_guided_launch": (
        C.c_int,
        [_vp, _P(GuidedOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp,
         _vp, C.c_size_t],
    ),
    "vs_guided": (
        C.c_int,
        [_vp, _P(GuidedOpts), _P(PitchOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp,
         C.c_size_t, _vp, _vp, C.c_size_t],
    ),
    "vs_strack_defaults": (C.c_int, [_P(StrackOpts)]),
    "vs_strack_from_pitch": (C.c_int, [_P(PitchOpts), C.c_int32, C.c_int32, _P(StrackRow)]),
    "vs_strack_launch": (
        C.c_int,
        [_vp, _P(StrackOpts), _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp,
         C.c_size_t, _vp, _vp, C.c_size_t],
    ),
    "vs_strack": (
        C.c_int,
        [_vp, _P(StrackOpts), _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t],
    ),
    "vs_psola_defaults": (C.c_int, [_P(PsolaOpts)]),
    "vs_psola_launch": (
        C.c_int,
        [_vp, _P(PsolaOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp,
         C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_size_t],
    ),
    "vs_psola": (
        C.c_int,
        [_vp, _P(PsolaOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp,
         _vp, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t],
    ),
    "vs_psola_ts_defaults": (C.c_int, [_P(PsolaTsOpts)]),
    "vs_psola_ts_launch": (
        C.c_int,
        [_vp, _P(PsolaTsOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp,
         C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, C.c_size_t,
         C.c_size_t, _vp, _vp, _vp, C.c_size_t],
    ),
    "vs_psola_ts": (
        C.c_int,
        [_vp, _P(PsolaTsOpts), _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp,
         _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t],
    ),
    "vs_version": (C.c_char_p, []),
}

# internal host helpers exported for CPU-side tests of the plan builder (not in the public header)
INTERNAL_SYMBOLS = {
    "vs_expand_lane": (C.c_int, [_P(Lane), C.c_int32, _P(DevLane)]),
    "vs_cos_row": (None, [C.c_int, _P(C.c_double)]),
    "vs_ring_slots_for": (C.c_int, [C.c_int, _P(C.c_int)]),
    "vs_tap_table_build": (C.c_int, [_P(Lane), _P(DevLane), C.c_size_t, C.c_size_t, _P(_P(C.c_double)), _P(C.c_size_t)]),
    "vs_vowel_index": (C.c_int, [C.c_int]),
    "vs_vowel_by_index": (C.c_int, [C.c_int]),
}

_lib = None


def load():
    """Load libvoicesynth.so (built in-tree by `make` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libvoicesynth.so is not built (%s). Run `make` or __graft_entry__.build(); "
            "there is no fallback implementation." % LIB_PATH
        )
    lib = C.CDLL(LIB_PATH)
    for table in (SYMBOLS, INTERNAL_SYMBOLS):
        for name, (res, args) in table.items():
            if "VS_LIB" in os.environ and not hasattr(lib, name):
                continue             # an A/B build of an earlier round (tools/): it simply lacks the newer entries
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


ROWS_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p)


class VsError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        try:
            msg = load().vs_strerror(code).decode()
        except Exception:  # pragma: no cover
            msg = "error"
        super().__init__("%s: %s (%d)" % (where, msg, code))


def check(code, where=""):
    if code != VS_OK:
        raise VsError(code, where)
    return code
