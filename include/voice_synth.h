/*
 * voice_synth.h -- C ABI of the MI355X (gfx950) batched vowel-synthesis engine.
 *
 * This is the drop-in boundary for ONE hot path of jsansao/voice_synth:
 *
 *     flowgen_shimmer (glottal source)  -->  vowel (order-22 all-pole vocal-tract filter)
 *
 * The reference exposes no library or FFI surface -- each stage is the body of a main()
 * (reference flowgen_shimmer.c:246-423 and vowel_new.c:237-331) -- so the entry points
 * below are what a binding for this path binds instead of those loops.  Every entry cites
 * the reference lines it replaces.  Plain C types only: pointers, sizes, fixed-width
 * integers.  No function calls exit(); every failure is a negative return code.
 *
 * Threading: a vs_ctx and the plans made from it may be used by one thread at a time -- with one
 * exception, made for callers who synthesise batch after batch of NEW utterances: while one thread
 * launches, reseeds, waits and times (vs_plan_launch, vs_plan_reseed, vs_plan_status, vs_ctx_synchronize,
 * vs_ctx_timer_*), ONE other thread may be inside vs_plan_create() or vs_plan_destroy() of the same
 * context -- plan creation touches nothing a launch reads, works on host threads and a stream of its
 * own, and the plan it returns is complete (cli/vs_bench.c --fresh does exactly that: the plan of
 * batch k + 1 is made while kernel k runs).  Different contexts are independent.  There is no global
 * mutable state, and the library reads no environment variable after vs_ctx_create() (see
 * vs_ctx_set_tuning()).
 *
 * There is no CPU fallback: if no gfx950 device is usable, vs_ctx_create() fails with
 * VS_ERR_NODEVICE and nothing can be synthesised.
 */
#ifndef VOICE_SYNTH_H
#define VOICE_SYNTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Filter order.  The reference runs Order = 22 for every table (vowel_new.c:172) inside arrays
 * bounded by MAX_ORDER 40 (vowel_new.c:33); its loop (vowel_new.c:279-281, 287-289) is written for
 * any Order.  A VS_VOWEL_CUSTOM coefficient set carries its own order (vs_lane.order, 1..40):
 *   - up to 22 taps it rides the fused kernel like a table (missing taps are zeros: acc - 0*y == acc
 *     while y is finite, so the result equals the reference's loop run with the smaller Order; see "loud and
 *     unstable sets" below for a state that is not);
 *   - 23..40 taps take the WIDE path: the source kernel writes the flow to HBM and a filter kernel
 *     with a 48-sample register window reads it back (un-fused: 6 bytes of HBM traffic per sample
 *     instead of 2, and ~2x the arithmetic).  A plan is wide as a whole as soon as one of its lanes
 *     is. */
#define VS_ORDER 22
#define VS_NCOEF (VS_ORDER + 1)
#define VS_MAX_ORDER 40
#define VS_MAX_NCOEF (VS_MAX_ORDER + 1)

/* return codes */
#define VS_OK 0
#define VS_ERR_ARG (-1)          /* NULL pointer, zero size, bad enum */
#define VS_ERR_RANGE (-2)        /* a parameter the reference would reject with usage() */
#define VS_ERR_UNSUPPORTED (-3)  /* legal for the reference's parser, but undefined behaviour
                                    there or beyond this engine's limits */
#define VS_ERR_HIP (-4)          /* a HIP runtime call failed; see vs_ctx_last_hip_error() */
#define VS_ERR_NOMEM (-5)
#define VS_ERR_NODEVICE (-6)     /* no usable gfx950 device: there is no CPU path */
#define VS_ERR_IO (-7)
#define VS_USAGE (-8)            /* argv parsers: the reference would print usage() and exit(0) */
#define VS_ERR_INTERNAL (-9)     /* a device-side bounded wait ran out (kernel bug, never expected) */

/* vs_lane.flags: which perturbation options were GIVEN on the command line.  The reference
 * tests "arg.X != -1" (flowgen_shimmer.c:248, 295, 373), not only the value. */
#define VS_FLAG_JITTER 0x1u
#define VS_FLAG_SHIMMER 0x2u
#define VS_FLAG_NOISE 0x4u

/* vs_lane.vowel: the reference's -v menu (vowel_new.c:153-156, 548-627) or an explicit
 * coefficient set. */
#define VS_VOWEL_CUSTOM 0

/*
 * One utterance ("lane").  Source fields are struct PAR of flowgen_shimmer.c:73-87 AFTER
 * initialization() (flowgen_shimmer.c:463-546) has converted the command-line units;
 * filter fields are the globals of vowel_new.c:76-77 plus the coefficient choice.
 * Duration is not per lane: a batch has one sample count (see vs_num_samples()).
 */
typedef struct vs_lane {
  float jitter;       /* mean jitter as a fraction: "-j x" / 100            fg:477 */
  float cq;           /* closed quotient                                    fg:490 */
  float K;            /* speed of closure                                   fg:484 */
  float Fg;           /* glottal formant, validation only                   fg:496 */
  float F0;           /* fundamental frequency, 50 <= F0 < Fg               fg:504 */
  float DC;           /* ABSOLUTE DC flow: "-l x" * amp, or 0.25 after -n   fg:182,524 */
  float noise;        /* linear SNR: pow(10, "-n x" / 10)                   fg:511 */
  float Kvar;         /* closure-speed variation                            fg:530 */
  float shimmer;      /* shimmer as a fraction: "-s x" / 100                fg:544 */
  int32_t fs;         /* sampling rate                                      fg:538 */
  int32_t amp;        /* maximum amplitude                                  fg:518 */
  uint32_t flags;     /* VS_FLAG_* */
  uint64_t seed;      /* Philox key of this lane's draw stream (replaces srandom(time), fg:241) */
  float gain;         /* vowel -g                                           vw:131 */
  float pre_emphasis; /* vowel -p                                           vw:126 */
  int32_t vowel;      /* 'a','i','u','1'..'7', or VS_VOWEL_CUSTOM           vw:152 */
  float out_snr;      /* vowel -n: linear SNR pow(10, x/10) of the white noise added to the
                         filtered signal frame by frame, 0 = off                vw:141-143, 302-324 */
  double A[VS_MAX_NCOEF]; /* A(z) when vowel == VS_VOWEL_CUSTOM: A[0] must be 1.0, A[1..order] the taps */
  int32_t order;      /* taps of the VS_VOWEL_CUSTOM set, 1..VS_MAX_ORDER; 0 means VS_ORDER (22) */
  int32_t reserved_;  /* keeps out_seed 8-byte aligned without implicit padding; must be 0 */
  uint64_t out_seed;  /* Philox key of the vowel stage's own draw stream (the reference's vowel
                         process calls srandom(time) itself, vw:234): one draw per sample */
} vs_lane;

/* Per-cycle diagnostics the reference prints inside its loop (flowgen_shimmer.c:307, 409): what flowgen_shimmer
 * prints line by line, and -- with the counts -- a public output of vs_source and vs_plan_launch for any batch (T is
 * the ground truth the acoustic and glottal tests measure against).  x_pow and w_pow are the reference's float sums,
 * added in its order; bit for bit the oracle's in every arithmetic (tests/test_gpu_cycle_log.py). */
typedef struct vs_cycle_rec {
  float S;      /* shimmer draw of the cycle ("%5.2f \n"), 0 when shimmer is off */
  float x_pow;  /* open-phase power   fg:378 */
  float w_pow;  /* noise power        fg:407 ; SNRdb = 10*log10(x_pow / w_pow) */
  int32_t T;    /* period of the cycle in samples */
} vs_cycle_rec;

/* Arithmetic of the filter recurrence.
 * VS_ARITH_EXACT: products and subtractions rounded one by one in the reference's order
 *                 (vowel_new.c:279-281); the double state equals the reference's bit for bit.
 * VS_ARITH_FMA:   fused multiply-adds in two partial sums; the double state differs in the last
 *                 bits, so the int16 output is not guaranteed identical.  For the reference's
 *                 tables: 0 differences in 1.05e9 samples of BASELINE config 3 and in 6e8 samples
 *                 of the option fuzz, bound +-1 LSB.  For explicit sets the distance follows the
 *                 set's conditioning (+-1 LSB measured for max |A| <= 500; a direct form of order
 *                 40 with coefficients of 1e4 moves a few samples by more).  With the vowel stage's own noise
 *                 (out_snr, vowel -n) the bound is +-2 LSB: the width of a frame's noise follows the frame's power, which a
 *                 sample that moved by one LSB moves in its last bits (tools/fuzz_fma.py: 9.6e9 fuzzed samples, 2 LSB in four
 *                 utterances, all of them with vowel -n). */
/* VS_ARITH_F32:   the recurrence in single precision, two taps per packed multiply-add -- 1.25 x the speed of VS_ARITH_FMA
 *                 for a MEASURED distance from the reference (single precision is marginal against 1e-5):
 *                 per table at gain 10 / pre-emphasis 1, RMS of full scale 4.6e-6 (table 7) .. 1.9e-5 (/i/), above 1e-5
 *                 for /i/, /u/ and table 1; at most 6 LSB there, 25 LSB for table 5 without pre-emphasis; 7.5e-6 over
 *                 BASELINE config 3's mix of tables.  The whole table
 *                 is tests/golden/f32_bounds.json (made by tools/f32_survey.py on the device); tests/test_gpu_f32.py holds
 *                 the kernels to it.  The distance is RELATIVE to the filter's state, i.e. it grows with the gain: over the
 *                 option fuzz's ordinary ranges (gain 1..20) RMS 8.4e-6, at most 61 LSB in 1.2e9 samples; with the corner
 *                 draws (vowel -g 100 and 1000: a state of 1e5..1e6 that the output clips) RMS 2.0e-5..2.9e-5 and single
 *                 unclipped samples off by hundreds of LSB, at most 1986 (tools/fuzz_fma.py ... f32, profiles/r06_f32_mode_measured.txt).  Only the fused wave-specialised kernels have this arithmetic: source-only and
 *                 filter-only launches, the one-wave kernel and coefficient sets of 23..40 taps run VS_ARITH_FMA. */
/* ---- the arithmetics of the 22-tap filter, operation by operation ------------------------------------------------------
 * Both opt-in arithmetics are deterministic: what a kernel computes is written out here, tests/arith_ref.py restates it in
 * numpy, and tests/test_gpu_arith.py and tests/test_gpu_synth_hostile.py hold the fused and the one-wave kernels to that
 * restatement byte for byte; the wide kernel (23..40 taps), which runs the FMA form with P = 40, is held to it by
 * tests/test_gpu_synth_hostile.py (the measured
 * distances above are what the written order amounts to: the single-precision restatement reproduces the figures of
 * tests/golden/f32_bounds.json on the CPU).  x[n] is the int16 flow, a_j = A[j], gain and pre the lane's float values,
 * y[n] = 0 for n < 0, fma(a, b, c) = a*b + c rounded once.
 *
 * VS_ARITH_FMA, in double (the form of the coefficient tracks below with P = 22, in a wide plan P = 40 for every lane;
 * a_j = 0 above the lane's order):
 *   acc = (double)x[n]*gain; p0 = acc; p1 = -(a_2*y[n-2]);
 *   for j = 3..P: odd j: p0 = fma(-a_j, y[n-j], p0), even j: p1 = fma(-a_j, y[n-j], p1);
 *   acc = fma(-a_1, y[n-1], p0 + p1); o = fma(-pre, y[n-1], acc); y[n] = acc; out[n] = R(o).
 *   The rounding R depends on the kernel family:
 *   - the one-wave kernel, the filter-only kind (vs_filter) and the wide kernel (23..40 taps): R = round2int, literally
 *     vowel_new.c:413-427 -- a half goes downwards (k + 0.5 -> k), its quirk set included, clamp to [-32767, 32767];
 *   - the wave-specialised kernels (vs_synth_ws_kernel, two and three roles): R = round to nearest, ties to EVEN
 *     (V_RNDNE_F64), a saturating conversion to int32 (NaN -> 0) and the clamp to [-32767, 32767].  This differs from
 *     round2int on exact ties and on round2int's quirk set only, by one LSB.
 *   So the same lane may differ by one LSB between the two families on a sample whose o is k + 0.5 exactly.
 *
 * VS_ARITH_F32 (the wave-specialised kernels; every other kernel runs VS_ARITH_FMA as above): every product and sum is one
 * float operation, fmaf(a, b, c) = a*b + c rounded once to float.  nA_j = -(float)a_j, g = (float)gain, npre = -(float)pre.
 * Samples come in pairs n (even), n + 1, each as two chains over alternate taps:
 *   even sample:  pex = nA_2*y[n-2]; pey = nA_1*y[n-1];
 *                 for k = 1..9: pex = fmaf(nA_(2k+2), y[n-2-2k], pex); pey = fmaf(nA_(2k+1), y[n-1-2k], pey);
 *                 pex = fmaf(nA_22, y[n-22], pex); pey = fmaf(nA_21, y[n-21], pey);
 *                 acc0 = fmaf((float)x[n], g, pex + pey);
 *   odd sample:   pox = nA_3*y[n-2]; poy = nA_2*y[n-1];
 *                 for k = 1..9: pox = fmaf(nA_(2k+3), y[n-2-2k], pox); poy = fmaf(nA_(2k+2), y[n-1-2k], poy);
 *                 sc = fmaf(nA_22, y[n-21], poy); sc = fmaf((float)x[n+1], g, sc + pox); acc1 = fmaf(nA_1, acc0, sc);
 *   out[n] = H(fmaf(npre, y[n-1], acc0)); out[n+1] = H(fmaf(npre, acc0, acc1)); y[n] = acc0; y[n+1] = acc1.
 *   H = round to nearest, ties UPWARDS: floor(o + 0.5), saturating, NaN -> 0 (V_CVT_RPI_I32_F32, which alone would turn a
 *   NaN into +-(2^31 - 1), behind V_MED3_F32(o, 0, o), which turns a NaN into 0 and leaves every number), then the clamp to
 *   [-32767, 32767].  A row of odd length computes its last pair and keeps the first sample of it.  The tests keep every
 *   intermediate above 2^-126 in magnitude (or zero): what the kernels do with single-precision denormals is not promised.
 * The order is the same in every workgroup shape, in both filter loops of the wave-specialised kernels (a wavefront whose
 * lanes share a position; lanes with positions of their own) and in both store paths (16-byte stores; sample by sample).
 *
 * Loud and unstable sets, in every arithmetic (VS_ARITH_EXACT too).  vs_lane_validate() refuses a set only for a tap that
 * is not finite, so a lane may drive its state anywhere.  Every rounding (round2int, nearest-even, half-up) clamps to
 * [-32767, 32767] whatever the size of its argument, past int32 and int64 too; +-inf goes to +-32767 and a NaN to 0.  What is promised
 * of a lane -- the reference's bytes, or the form above -- ends at the first y[n] that is not finite and includes that
 * sample: lanes carry zeros in the taps above their order, and 0 * +-inf is NaN where the reference's shorter loop keeps
 * +-inf (order 1, a_1 = 2, a constant flow: the reference puts out -+32767 for ever, a kernel 0 from two samples behind
 * the first infinity).  Behind that sample only |out| <= 32767 holds (never -32768).  No other lane is affected.
 * tests/test_gpu_synth_hostile.py holds every synthesis filter kernel to this. */
#define VS_ARITH_EXACT 0
#define VS_ARITH_FMA 1
#define VS_ARITH_F32 2

/* What a plan launch computes. */
#define VS_KIND_SYNTH 0   /* source -> filter, flow never leaves the chip      (fg:246-423 + vw:237-331) */
#define VS_KIND_SOURCE 1  /* source only: int16 glottal flow                   (fg:246-423) */
#define VS_KIND_FILTER 2  /* filter only: int16 flow in, int16 speech out      (vw:237-331) */

typedef struct vs_ctx vs_ctx;
typedef struct vs_plan vs_plan;

/* ---- parameter helpers (host only, no device needed) -------------------------------- */

/* Reference defaults: par initialiser flowgen_shimmer.c:87, vowel_new.c:76-77, vowel 'a'. */
int vs_lane_defaults(vs_lane *lane);

/* nSamples = (unsigned long) par.fs * par.dur, a FLOAT product (flowgen_shimmer.c:242). */
int vs_num_samples(int32_t fs, float dur, uint64_t *n_samples);

/* Row pitch (in samples) that suits the kernels' stores for rows of n_samples: a caller who allocates the PCM buffer
 * [n_lanes][pitch] may pick any pitch >= n_samples, and the choice shows in a full-chip launch -- about 2 % between
 * dense rows of 16000 samples and this pitch, 10-13 % against rows a power of two apart (16384 or 32768 samples, dense).
 * Why: a wavefront's store instruction writes 16 bytes into each of 64 rows at the SAME offset, so the distance between
 * the rows decides how those 64 writes spread over the memory channels (profiles/r05_row_pitch.txt,
 * tools/pitch_probe.py).  Returned: n_samples rounded up to a whole number of 128-byte lines, that number being
 * 3 (mod 4); rows shorter than 2 KiB are only rounded up to 16 bytes.  Every pitch >= n_samples remains VALID
 * (vs_plan_launch takes what it is given); this one avoids the slow ones. */
size_t vs_row_pitch(size_t n_samples);

/* The denominator tables of coefficients(), vowel_new.c:430-633.  A receives 23 doubles. */
int vs_vowel_coefficients(int vowel, double *A);

/* Order of the lane's all-pole filter: VS_ORDER for the ten tables, vs_lane.order (1..VS_MAX_ORDER,
 * 0 = VS_ORDER) for a VS_VOWEL_CUSTOM set; VS_ERR_RANGE beyond MAX_ORDER (vowel_new.c:33). */
int vs_lane_order(const vs_lane *lane, int *order);
/* The label coefficients() prints for the entry ("/a/ JPHS", ...), vowel_new.c:550-622. */
const char *vs_vowel_name(int vowel);

/* Range checks of initialization() (flowgen_shimmer.c:470-546) and of vowel's option loop
 * (vowel_new.c:126-143).  VS_ERR_RANGE where the reference prints usage(); VS_ERR_UNSUPPORTED
 * where the reference would run into undefined behaviour or this engine's limits. */
int vs_lane_validate(const vs_lane *lane);

const char *vs_strerror(int code);

/* ---- command-line surface (host only) ------------------------------------------------ */

typedef struct vs_flowgen_cmd {
  vs_lane lane;
  float dur;            /* -d */
  int wav_arg;          /* argv index of the output file name (arg.wav, fg:140) */
} vs_flowgen_cmd;

typedef struct vs_vowel_cmd {
  float gain, pre_emphasis, snr; /* snr already pow(10, x/10), 0 when -n absent */
  int vowel;
  int input_arg, output_arg, noise_arg;
} vs_vowel_cmd;

/* The option loop + initialization() of flowgen_shimmer.c:128-222, 463-546, without the
 * exit(): VS_USAGE where the reference calls usage(). */
int vs_flowgen_parse(int argc, char **argv, vs_flowgen_cmd *cmd);
/* The option loop of vowel_new.c:116-192. */
int vs_vowel_parse(int argc, char **argv, vs_vowel_cmd *cmd);

/* RIFF header as the reference lays it out (flowgen_shimmer.c:49-63, 550-565).
 * header_bytes is 44 (ILP32 build, the standard layout) or 72 (LP64 build).
 * Returns the number of bytes written into buf (>= 72 must be available) or < 0. */
int vs_wav_header_write(unsigned char *buf, int header_bytes, int32_t fs, float dur);
/* Parses either layout (vowel_new.c:196-205 reads its own struct).  Returns header size. */
int vs_wav_header_read(const unsigned char *buf, size_t avail, int32_t *fs, int *format_tag,
                       int *bits_per_sample, uint64_t *data_bytes);

/* ---- device context ------------------------------------------------------------------ */

int vs_ctx_create(int device, vs_ctx **ctx);
void vs_ctx_destroy(vs_ctx *ctx);
/* Use an existing hipStream_t for all launches of this context (NULL = default stream). */
int vs_ctx_set_stream(vs_ctx *ctx, void *hip_stream);
int vs_ctx_set_arith(vs_ctx *ctx, int arith);
int vs_ctx_last_hip_error(const vs_ctx *ctx);

/* Launch tuning.  All zero (the default) = the library's own choices; the fields exist for
 * measurements (tools/) and tests.  Values are validated here, once, and copied into every plan
 * made afterwards; nothing else can change what a plan launches -- in particular no environment
 * variable does, unless VS_DEBUG_TUNING=1 asks vs_ctx_create() to read the experiment knobs
 * (VS_KERNEL, VS_RING_SLOTS, VS_READY_MIN, VS_WS_PAIRS, VS_WS_ROLES, VS_GEN_LOW, VS_GEN_MIN, VS_WS_PRIO, VS_MIXED_RINGS) through this
 * same function.  NULL resets. */
#define VS_KERNEL_AUTO 0
#define VS_KERNEL_SINGLE 1 /* one wavefront per 64 utterances generates and filters */
#define VS_KERNEL_WS 2     /* wave-specialised: two or three wavefronts per 64 utterances, one job each */
#define VS_FAULT_WITHHOLD_PROGRESS 1 /* tests: the generator wavefront never publishes its progress */
#define VS_FAULT_SHORT_COS_ROWS 2    /* tests: the kernel finds no room for its cos rows (plan and kernel disagree) */
#define VS_FAULT_SHARD_PREPARE 3     /* tests: a context that serves a shard of a node fails to prepare its chunks (vs_node_synth_gather) */
#define VS_FAULT_SHARD_HANDOVER 4    /* tests: ... fails while handing its first chunk over, after the others have started */
#define VS_FAULT_SIMD_DEALING 5      /* tests: plans behave as if vs_ctx_simd_dealing() had found the wavefronts NOT dealt four at a time */
#define VS_FAULT_REROUND 6           /* tests: every seventh super-step of the kernels that take vowel -n's frame powers along rounds its results twice, as if
                                        round2int()'s quirk set had been hit -- the frames concerned must come from the streaming pass instead */
typedef struct vs_tuning {
  int32_t kernel;     /* VS_KERNEL_* */
  int32_t ring_slots; /* LDS ring capacity per utterance in samples (rounded to 24, clamped to what fits) */
  int32_t ready_min;  /* 1..64: a super-step runs when ready lanes * 64 >= live lanes * ready_min */
  int32_t ws_pairs;   /* 1, 2 or 4 generator/filter pairs per workgroup (as many as fit the LDS) */
  int32_t gen_low;    /* >= 24: a lane with fewer buffered samples starts a generator round at once */
  int32_t gen_min;    /* 1..64: a round starts when wanting lanes * 64 >= needing lanes * gen_min */
  int32_t spin_limit; /* polls before a waiting wavefront gives up with VS_ERR_INTERNAL */
  int32_t fault;      /* VS_FAULT_* */
  int32_t ws_filter_prio; /* s_setprio of the filter wavefront: 0 = default (3), 1..3, -1 = leave it at 0 */
  int32_t ws_roles;   /* wavefronts per 64 utterances of the wave-specialised launch: 0 = the library's choice,
                         2 = generator | filter, 3 = open phase | noise | filter (full grids) */
  int32_t mixed_rings; /* batches whose groups differ in period: 0 = the library's choice (a workgroup holds groups from
                          across the period range, each with the ring depth ITS periods need), -1 = never (uniform rings),
                          > 1 = the same with this many slots as the shallowest ring (measurements) */
} vs_tuning;
int vs_ctx_set_tuning(vs_ctx *ctx, const vs_tuning *tuning);
/* Device self-test of the arithmetic shortcuts the kernels take: [0] division shortcut
 * (exhaustive over all 2^31 draws), [1] Philox known answers, [2] integer square root,
 * [3] rounding, [4] one-fma noise sample (exhaustive over the draws at 16 widths), [5] two-block
 * Philox with prepared round keys, [6] workgroups of the wave-to-SIMD probe below that were NOT dealt
 * "wavefront w next to wavefront w % 4" (a performance assumption, not a correctness one -- but on the hardware this
 * library is written for it holds, and a chip where it does not is worth a failed self-test), [7] the output-noise sample of vowel -n
 * (conversion of a draw and the one-instruction rounding, exhaustive over the draws and over every float).  failures
 * (optional) receives VS_SELFTEST_COUNTERS counters; VS_OK if all are zero, else VS_ERR_INTERNAL. */
#define VS_SELFTEST_COUNTERS 8
int vs_ctx_selftest(vs_ctx *ctx, uint64_t *failures);
/* How the hardware deals the wavefronts of a workgroup to the four SIMDs of a compute unit, read from HW_ID by a
 * one-workgroup-per-CU probe launch (once per context, cached): *cyclic12 / *cyclic8 = 1 if in every probed
 * 12- / 8-wavefront workgroup the first four wavefronts ran on four different SIMDs and wavefront w ran on the SIMD
 * of wavefront w % 4 (MI355X: four rotations of the order 0, 2, 1, 3) -- what the three-role layouts of the fused
 * kernel are built on (the three wavefronts of ONE group share a SIMD; on half-filled chips the filter wavefront has one to
 * itself).  Where it does not hold, plans take the two-role kernel instead of running the three roles in an order
 * that is 2.5 x slower (vs_plan_roles says so). */
int vs_ctx_simd_dealing(vs_ctx *ctx, int *cyclic12, int *cyclic8);
/* Name, CU count of the device in use. */
int vs_ctx_device_info(const vs_ctx *ctx, char *name, size_t name_len, int *cu_count);
/* PCI bus id of the device in use ("0000:05:00.0", hipDeviceGetPCIBusId): what tells two devices of a node
 * apart when a multi-GPU run has to show that N DIFFERENT devices took part (bench.py, vs_bench). */
int vs_ctx_device_pci(const vs_ctx *ctx, char *bus_id, size_t len);

/* ---- plans: host preparation once, any number of launches ---------------------------- */

/* Validates the lanes, builds the per-T2 cosine tables with the host libm (flowgen_shimmer.c:
 * 319, 328 call cos() per sample; T2 = ceil(.5*cq*P) is fixed per utterance), and uploads the
 * lane records.  The lanes array may be freed afterwards.
 * Limits (VS_ERR_UNSUPPORTED beyond them): n_lanes < 2^31 - 64, n_samples < 2^31 - 256, periods
 * whose ring does not fit a compute unit's LDS: fs/F0 up to ~930 (with jitter; ~1120 without) runs
 * on the kernels with 64 utterances per wavefront, up to ~3800 (~4500) on the narrow build of the
 * one-wave kernel (16 utterances per wavefront, slow: vs_plan_kernel_name says which).  The narrow build's figures are those
 * of a homogeneous batch, whose wavefronts stage one cos row: what has to fit the LDS is the ring of the batch's longest
 * period plus the cos rows of its worst wavefront of 16 (one row of ceil(.5*cq*P) doubles per distinct value among its
 * lanes), so a batch of long periods that differ in period and cq is refused when they do not, even if every lane of it
 * passes alone.  An utterance's draw stream is
 * indexed with 32 bits: about one draw per sample, so the sample limit keeps it in range for every
 * setting short of rejection loops that retry thousands of times per cycle.
 * Cost (65536 utterances: about 1 ms on the host and 0.2 ms of upload, profiles/r05_plan_cost.txt): batches of 8192
 * utterances and more are expanded by worker threads of the context's own -- up to 15, started with the first such plan,
 * asleep between plans, signals blocked, ended by vs_ctx_destroy -- into page-locked memory, and go up as DMA transfers
 * that run next to a launch that is under way: a caller who synthesises NEW utterances makes the plan of batch k + 1
 * while batch k's kernel runs (for new DRAWS of the same utterances there is vs_plan_reseed).  Like the HIP runtime
 * under it, a context does not survive fork(). */
int vs_plan_create(vs_ctx *ctx, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
                   vs_plan **plan);
/* May be called while launches of the plan are still running: the plan's device blocks (records, tables, the output-noise
 * tables) are not freed -- hipFree waits for the whole device, i.e. for the kernels of the batches behind -- but kept by the
 * context (up to 32 of them: 9 MB per plan of 65536 utterances) and handed to the next plan of that size once the launches
 * that read them are over (an event recorded behind the plan's last launch).  vs_ctx_trim() / vs_ctx_destroy() free them. */
void vs_plan_destroy(vs_plan *plan);

/* Launch on the context's stream; returns without waiting for the device.
 *   in_dev   : VS_KIND_FILTER only, int16 [n_lanes][in_pitch] glottal flow (device pointer)
 *   out_dev  : int16 [n_lanes][out_pitch] (device pointer), out_pitch >= n_samples (vs_row_pitch() names the fast one)
 *   log_dev  : optional vs_cycle_rec [n_lanes][log_pitch] (device pointer) or NULL
 *   ncyc_dev : optional int32 [n_lanes], cycles generated per lane, or NULL
 * Of row l of the log a launch writes records [0, min(ncyc[l], log_pitch)) and nothing else: what lies behind them, and
 * behind the last row, keeps what it held -- a launch does not clear the log (vs_source below does: its rows come back
 * zero behind the last record).  ncyc[l] is the FULL count of cycles generated, also where log_pitch cut the row's log
 * short.  Row l belongs to lanes[l] of vs_plan_create, whatever order the plan keeps its records in.  A launch with a
 * log runs the one-wave kernel; the log and the counts do not depend on the context's arithmetic. */
int vs_plan_launch(vs_plan *plan, int kind, const int16_t *in_dev, size_t in_pitch,
                   int16_t *out_dev, size_t out_pitch, vs_cycle_rec *log_dev, size_t log_pitch,
                   int32_t *ncyc_dev);
int vs_ctx_synchronize(vs_ctx *ctx);
/* Device time between two points of the context's launch stream, for callers who have no HIP of their own (the C programs
 * of this package): vs_ctx_timer_mark(ctx, 0) and (ctx, 1) record an event each behind what has been enqueued so far;
 * vs_ctx_timer_elapsed waits for mark 1 and gives the milliseconds from mark 0 to it. */
int vs_ctx_timer_mark(vs_ctx *ctx, int which);
int vs_ctx_timer_elapsed(vs_ctx *ctx, double *ms);
/* Waits for the context's stream, then reports the health word of the plan's launches:
 * VS_OK, or VS_ERR_INTERNAL if a device-side check failed (*flags, optional, gets the raw bits:
 * 1, 2, 4 = a bounded wait of the generator / filter / noise wavefront ran out, 8 = plan and kernel
 * disagree about the room for the cos rows).  The one-call conveniences below check it themselves.
 * What such a launch has written is NOT the utterances (lanes whose check failed synthesise from whatever
 * the LDS holds): every row of every launch of the plan since the last VS_OK status must be discarded.  The
 * chunked paths (vs_synth_rows, vs_node_synth_gather, vs_node_synth_rows) read the status of a chunk only
 * after it has been delivered, so rows a callback has already seen, or that already lie in the caller's
 * buffer, are to be discarded as well when the call returns VS_ERR_INTERNAL. */
int vs_plan_status(vs_plan *plan, int *flags);
/* The same utterances with NEW draws: replaces every lane's seed (and out_seed: out_seeds may be NULL = the same values)
 * in the plan's device records -- what running the reference's programs again does, which seed from the clock
 * (flowgen_shimmer.c:241, vowel_new.c:234).  seeds[i] belongs to lanes[i] of vs_plan_create, whatever order the plan
 * keeps its records in; the arrays are the caller's again when the call returns.  Stream-ordered with the plan's
 * launches on the context's stream (launches enqueued before see the old seeds, launches after the new ones); 16 bytes
 * per lane go up instead of a whole new plan (65536 lanes: 0.1 ms against 3 ms).  A lane's seed does not change which
 * kernel or ring the plan uses. */
int vs_plan_reseed(vs_plan *plan, const uint64_t *seeds, const uint64_t *out_seeds);

/* Host cost of vs_plan_create(): host_ms = validation, parameter expansion, sorting, cosine
 * tables (cut over up to 8 host threads for batches >= 8192); upload_ms = device allocation,
 * upload and the wait for it.  Neither is part of a launch. */
int vs_plan_timing(const vs_plan *plan, double *host_ms, double *upload_ms);
/* Name of the kernel a launch of this kind runs ("vs_synth_kernel<0, 0, false, true>", ...), as
 * rocprofv3 prints it; for measurement scripts. */
int vs_plan_kernel_name(const vs_plan *plan, int kind, char *buf, size_t len);

/* Dynamic LDS bytes per 64-lane workgroup and launch geometry a plan will use. */
/* Launch shape of the fused kind: *roles = wavefronts per 64 utterances (1 = the one-wave kernel, 2, 3), *layout =
 * 0 role-major / 1 spread (the filter wavefront alone on its SIMD), *simd_fallback = 1 if the plan wanted three
 * roles and took two because vs_ctx_simd_dealing() found the wavefronts dealt differently.  Any pointer may be NULL. */
int vs_plan_roles(const vs_plan *plan, int *roles, int *layout, int *simd_fallback);
int vs_plan_info(const vs_plan *plan, size_t *lds_bytes, size_t *n_workgroups,
                 size_t *ring_slots);

/* ---- host-buffer entry points (plan, launch, deliver) --------------------------------- */

/* fg:246-423 then vw:237-331 for every lane; pcm is int16 [n_lanes][n_samples].
 * The reference writes its samples out cycle by cycle (flowgen_shimmer.c:413-421) and frame by
 * frame (vowel_new.c:327); here the finished rows cross PCIe in 16 MiB blocks while later
 * chunks of the batch are still being synthesised (chunks of 16384 utterances, two device
 * buffers, four DMA workers with pinned staging buffers owned by the context).  If pcm is
 * PINNED host memory (vs_host_alloc, hipHostMalloc, hipHostRegister) the blocks are DMAed straight
 * into it; otherwise each block is copied from its staging buffer into pcm by its worker.  A
 * staging buffer always holds at least one whole row: utterances of more than 8 388 608 samples
 * make the context allocate larger ones (four of them, pinned). */
int vs_synth(vs_ctx *ctx, const vs_lane *lanes, size_t n_lanes, size_t n_samples, int16_t *pcm);

/* The same pipeline with the caller in the place of the memcpy: cb receives `rows` finished
 * consecutive rows starting at `row0` (int16 [rows][n_samples], contiguous) in a pinned staging
 * buffer that is valid only during the call.  cb runs on the library's delivery threads, up to
 * four calls at a time for different blocks, in no particular order; every row is delivered
 * exactly once.  A non-zero return stops the pipeline with VS_ERR_IO.  (vs_batch writes its
 * .wav files from here: header + payload, fwrite after fwrite, as the reference does.) */
typedef int (*vs_rows_cb)(void *user, size_t row0, size_t rows, const int16_t *pcm);
int vs_synth_rows(vs_ctx *ctx, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
                  vs_rows_cb cb, void *user);

/* Pinned host memory for callers without a HIP binding of their own. */
int vs_host_alloc(vs_ctx *ctx, size_t bytes, void **ptr);
int vs_host_free(vs_ctx *ctx, void *ptr);
/* Releases the buffers the context keeps between calls (device PCM chunks, staging, streams, the device blocks of
 * destroyed plans). */
int vs_ctx_trim(vs_ctx *ctx);
/* fg:246-423; flow is int16 [n_lanes][n_samples].  recs/ncyc optional (NULL): recs is [n_lanes][recs_pitch], cleared by
 * the call -- records [0, min(ncyc, recs_pitch)) of a row are the cycles', the rest of it zero. */
int vs_source(vs_ctx *ctx, const vs_lane *lanes, size_t n_lanes, size_t n_samples, int16_t *flow,
              vs_cycle_rec *recs, size_t recs_pitch, int32_t *ncyc);
/* vw:237-331; only gain, pre_emphasis, vowel/A, out_snr/out_seed and fs (frame length of the
 * output noise) of each lane are used; the source fields are not even validated, so a flow of
 * any sample rate can be filtered (vowel_new.c:196-205). */
int vs_filter(vs_ctx *ctx, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
              const int16_t *flow, int16_t *pcm);

/* ---- one batch over the GPUs of a node --------------------------------------------- */

/* Utterances are independent (all carried state of the reference is per utterance:
 * flowgen_shimmer.c:121-122, vowel_new.c:90), so a batch shards as contiguous blocks of lanes,
 * block s of S (blocks differ by at most one lane, vs_node_shard_range), with no data-path collective; a lane's draws
 * are keyed by the seed in its own record, so S shards give byte for byte what one device
 * gives.  devices[] lists one device per shard; a device may appear more than once ("logical
 * shards": how the N-device path is exercised on one GPU).  devices[0] is the root.  One
 * context, two streams and one host thread per shard; calls on a node are not re-entrant. */
typedef struct vs_node vs_node;
int vs_node_create(const int *devices, int n_shards, vs_node **node);
void vs_node_destroy(vs_node *node);
int vs_node_shards(const vs_node *node);
int vs_node_ctx(vs_node *node, int shard, vs_ctx **ctx); /* e.g. for vs_ctx_set_tuning */
int vs_node_set_arith(vs_node *node, int arith);
int vs_node_shard_range(const vs_node *node, size_t n_lanes, int shard, size_t *lo, size_t *hi);
/* How vs_node_synth_gather moves a finished chunk into the root's memory.
 *   VS_NODE_TRANSPORT_PEER (default): peer DMA, one copy stream per shard.
 *   VS_NODE_TRANSPORT_RCCL (EXPERIMENTAL until a multi-GPU node has run it: what one GPU can exercise -- the
 *     communicator, the all-or-nothing start, the abort path -- is tested; a send and a receive between two devices
 *     are not): ncclSend / ncclRecv on ONE RCCL communicator over the node's devices,
 *     created here and owned by the node (librccl is opened with dlopen at this call).  Needs every
 *     shard on a device of its own (VS_ERR_UNSUPPORTED otherwise, or when librccl is not there) and a
 *     packed root buffer (root_pitch == n_samples).
 *     The exchange is all or nothing (every shard prepares all of its chunks before anybody enqueues anything); a
 *     failure behind that point aborts the communicators (ncclCommAbort) and leaves the node on the peer transport.
 * vs_node_link(): how shard's PCM reaches the root -- VS_NODE_LINK_SELF (same device, in place),
 * _PEER (peer DMA), _STAGED (no peer access between the two devices: the copies go through host
 * memory), _RCCL.  vs_node_last_rccl_error(): the ncclResult_t of the last failing RCCL call.
 * vs_node_rccl_ranks(): ncclCommCount of the shard's communicator -- the number of ranks RCCL itself says it spans (the
 * node's shard count on a healthy node), 0 while the node is on the peer transport, < 0 on error: what a pre-flight prints
 * next to the PCI bus ids (cli/vs_bench.c --gpus N --rccl).  Switching to the RCCL transport ends with a link check: 64 KiB
 * from the root's communicator to itself through the entry points the gather uses (group, receive, send), compared byte
 * for byte; a library that fails it is refused (the ncclResult_t in vs_node_last_rccl_error, or VS_ERR_INTERNAL for bytes
 * that differ) and the node stays on peer copies. */
#define VS_NODE_TRANSPORT_PEER 0
#define VS_NODE_TRANSPORT_RCCL 1
#define VS_NODE_LINK_SELF 0
#define VS_NODE_LINK_PEER 1
#define VS_NODE_LINK_STAGED 2
#define VS_NODE_LINK_RCCL 3
int vs_node_set_transport(vs_node *node, int transport);
int vs_node_link(const vs_node *node, int shard);
int vs_node_last_rccl_error(const vs_node *node);
int vs_node_rccl_ranks(vs_node *node, int shard);
/* Synthesis with the final PCM gathered into the ROOT device's memory (root_dev: int16
 * [n_lanes][root_pitch] on devices[0]).  Every shard works through its block in chunks of 16384
 * utterances; with VS_NODE_OVERLAP a finished chunk travels to its rows of root_dev by a peer
 * DMA (one transfer stream per shard = per xGMI link into the root, no ring) while the shard's
 * next chunk is being synthesised; without it copies and kernels alternate (the comparison
 * case).  Shards on the root device are synthesised in place unless VS_NODE_STAGE_ALL sends them
 * through the chunk buffers and the copy too (tests of the transfer path on one GPU).
 * total_ms: host clock over the whole call; max_compute_ms: the slowest shard from its first
 * launch to its last kernel's end.  Both optional. */
#define VS_NODE_OVERLAP 1
#define VS_NODE_STAGE_ALL 2
int vs_node_synth_gather(vs_node *node, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
                         int16_t *root_dev, size_t root_pitch, int flags, double *total_ms,
                         double *max_compute_ms);
/* Synthesis with host delivery: every shard runs the vs_synth_rows() pipeline over its own PCIe
 * link; cb sees global row numbers (and is called from up to 4 threads per shard). */
int vs_node_synth_rows(vs_node *node, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
                       vs_rows_cb cb, void *user);

/* Raw device memory for callers without a HIP binding of their own (the CLIs). */
int vs_dev_alloc(vs_ctx *ctx, size_t bytes, void **ptr);
int vs_dev_free(vs_ctx *ctx, void *ptr);
int vs_dev_upload(vs_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int vs_dev_download(vs_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- acoustic measurement: F0, jitter, shimmer, HNR of int16 rows (csrc/vs_acoustic.hip) ------------------
 *
 * The "acoustic" tool the reference's README names ("measurement of jitter, shimmer, f0 and snr") and never shipped.
 * Every quantity that decides a mark or a period is an exact integer, so the result does not depend on the order of a
 * sum; the doubles are then evaluated in the order written here (the library is compiled with -ffp-contract=off).
 *
 * Per row: x[0..len) int16, the row's rate fs, and from the options f0_min, f0_max (float) and polarity p (+1 marks
 * maxima, -1 minima); y = p * x.  The host computes, in double,
 *     tmin = (int)floor((double)fs / f0_max),   tmax = (int)ceil((double)fs / f0_min)
 * and the call fails with VS_ERR_RANGE for any row with tmin < 2, tmin >= tmax or tmax > VS_AC_MAX_LAG.
 *
 * A. Period estimate and HNR (one window from the middle of the row, away from the filter's start-up transient and the
 *    cut last cycle).  W = 2*tmax.  len < 3*tmax + 2: status VS_AC_TOO_SHORT, all doubles NaN, no marks.  Else
 *    s = (len - W - tmax - 1) / 2 (integer division) and, exactly,
 *        r(t) = sum_{k<W} y[s+k] * y[s+k+t]     for t = 0 and t in [tmin-1, tmax+1].
 *    rmax = max r(t) over [tmin, tmax]; rmax <= 0: status VS_AC_UNVOICED (all doubles NaN, no marks).
 *    P0 = the smallest t in [tmin, tmax] with r(t) > r(t-1), r(t) >= r(t+1) and 10*r(t) >= 9*rmax (int64); if there is
 *    none, the first t with r(t) == rmax.  e = sum_{k<W} y[s+k+P0]^2;
 *        rho = (double)r(P0) / sqrt((double)r(0) * (double)e),  clamped to [1e-10, 1 - 1e-10],
 *        hnr_db = 10*log10(rho / (1 - rho))     (Boersma's autocorrelation HNR: the README's "snr"; within +-100 dB).
 *
 * B. Cycle marks, one forward pass, ties to the first index.  m_0 = first argmax of y over [0, tmax).  With
 *    lo1 = max(tmin, (2*P0+2)/3), hi1 = min(tmax, (3*P0)/2) and d = (P0 + 3)/4, the window of m_1 is m_0 + [lo1, hi1]
 *    and the window of m_{i+1} is m_i + [max(lo1, T_i - d), min(hi1, T_i + d)], T_i = m_i - m_{i-1}; m_{i+1} = first
 *    argmax of y over its window.  (Every period stays within [lo1, hi1]: bounded by tmin/tmax alone, a walk that
 *    once steps onto a formant peak of noisy speech follows ever shorter periods down to tmin.)  The walk stops at the first window whose upper end is >= len (the last, partial cycle is not
 *    measured).  Periods T_1..T_K; amplitudes a_i = y[m_i] - min(y[m_{i-1} .. m_i)) (the mark's peak above the trough
 *    before it -- not max - min over the cycle, which masks growing amplitudes).
 *
 * C. Summary (Praat's voice-report definitions):
 *        Tm           = (double)sum T / K                     f0_hz        = (double)fs / Tm
 *        jitter_local = ((double)sum_{i<K} |T_{i+1} - T_i| / (double)(K-1)) / Tm
 *        jitter_abs_s = ((double)sum_{i<K} |T_{i+1} - T_i| / (double)(K-1)) / (double)fs
 *        jitter_rap   = ((double)sum_{i=2..K-1} |3T_i - (T_{i-1} + T_i + T_{i+1})| / (3.0*(double)(K-2))) / Tm
 *        jitter_ppq5  = ((double)sum_{i=3..K-2} |5T_i - sum_{j=i-2..i+2} T_j| / (5.0*(double)(K-4))) / Tm
 *    shimmer_local, shimmer_apq3, shimmer_apq5: the same three on a (Am = (double)sum a / K in place of Tm);
 *        shimmer_db   = (sum_{i<K} |20*log10((double)a_{i+1} / (double)a_i)|, summed in order of i) / (double)(K-1).
 *    A field that needs more periods than there are (f0: 1, local/abs/db: 2, rap/apq3: 3, ppq5/apq5: 5) is NaN, and so
 *    is every shimmer field when some a_i <= 0 (VS_AC_ZERO_AMPLITUDE).  K < 2 sets VS_AC_FEW_PERIODS (a row long
 *    enough for stage A always holds two: the bit only completes the record).
 *
 * Records: p0 = P0 (0 when stage A gave up), n_periods = K, first_mark = m_0 (-1 without marks), status = VS_AC_* bits.
 * Marks (optional): m_0..m_K of row i at marks[i * marks_pitch + j] for j < marks_pitch (the rest of the row untouched).
 */
#define VS_AC_MAX_LAG 2048        /* largest tmax (96 kHz at 47 Hz) */
#define VS_AC_TOO_SHORT 0x1       /* len < 3*tmax + 2 */
#define VS_AC_UNVOICED 0x2        /* rmax <= 0 */
#define VS_AC_FEW_PERIODS 0x4     /* K < 2 */
#define VS_AC_ZERO_AMPLITUDE 0x8  /* some a_i <= 0: the shimmer fields are NaN */
typedef struct vs_measure_opts {
  float f0_min;       /* Hz, default 50 (the reference's lower bound for F0, fg:504) */
  float f0_max;       /* Hz, default 500 */
  int32_t polarity;   /* +1 (default): marks on maxima; -1: on minima */
  int32_t reserved_;  /* must be 0 */
} vs_measure_opts;
typedef struct vs_acoustic {
  double f0_hz, jitter_local, jitter_abs_s, jitter_rap, jitter_ppq5;
  double shimmer_local, shimmer_db, shimmer_apq3, shimmer_apq5, hnr_db;
  int32_t p0, n_periods, first_mark, status;
} vs_acoustic; /* 96 bytes */
int vs_measure_defaults(vs_measure_opts *opts);
/* Device pointers: pcm_dev [n_lanes][pitch] int16 (pitch >= n_samples), out_dev vs_acoustic [n_lanes], marks_dev int32
 * [n_lanes][marks_pitch] or NULL.  fs (one rate per row) and lengths (NULL: n_samples for every row; each <= n_samples)
 * are HOST arrays; the library uploads what the kernels need from them itself.  Enqueued on the context's stream --
 * behind a vs_plan_launch() into pcm_dev, say -- and returns without waiting.  opts NULL: vs_measure_defaults(). */
int vs_measure_launch(vs_ctx *ctx, const vs_measure_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                      size_t n_samples, const int32_t *fs, const int32_t *lengths, vs_acoustic *out_dev,
                      int32_t *marks_dev, size_t marks_pitch);
/* Host buffers: upload, vs_measure_launch, download, wait. */
int vs_measure(vs_ctx *ctx, const vs_measure_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes,
               size_t n_samples, const int32_t *fs, const int32_t *lengths, vs_acoustic *out, int32_t *marks,
               size_t marks_pitch);

/* ---- LPC analysis: vocal-tract coefficients and formants of int16 rows (csrc/vs_lpc.hip) -------------------------
 *
 * The filter half of the measurement: autocorrelation linear prediction per frame gives A(z) (ready for vs_lane.A), the
 * reflection coefficients' prediction error and, from the roots of A(z), the formants.  r(k) is an exact integer and
 * the recursion is evaluated in the order written here (the library is compiled with -ffp-contract=off), so r0, err,
 * start, status and the coefficients do not depend on how the device sums.
 *
 * Rows and frames.  Per row: x[0..len) int16, its rate fs.  pre (opts.pre_emphasis) is 0, or 1 for the analysis
 * pre-emphasis d[n] = x[n] - x[n-1] (an integer first difference); without it d = x.
 *     L = (int)floor((double)window_s * fs + 0.5),   H = (int)floor((double)hop_s * fs + 0.5)     (in double)
 * The call fails with VS_ERR_RANGE unless order < L <= VS_LPC_MAX_WINDOW for every row, and H >= 1 when hop_s > 0.
 *     hop_s > 0:  n_frames = len >= pre + L ? 1 + (len - pre - L) / H : 0; frame j starts at s = pre + j*H.
 *     hop_s == 0: one frame from the middle, s = pre + (len - pre - L) / 2 (n_frames 0 when len < pre + L): the
 *                 copy-synthesis mode.
 * Window: Hamming quantised to integers, w[n] = (int)floor(256 * (0.54 - 0.46*cos(2*pi*n/(L-1))) + 0.5) (double, on the
 * host: vs_lpc_window), or rectangular, w[n] = 256.  v[n] = w[n] * d[s+n], n < L.
 *
 * Autocorrelation, exact:  r(k) = sum_{n<L-k} v[n]*v[n+k] for k = 0..order, an exact integer, then (double).
 *     |v| < 2^24, so every product is below 2^48; with L <= 2^14, |r| < 2^62 fits int64.  Any partial sum of up to 32
 *     products is an exact fp64 integer, so the device may sum in any order (it sums blocks of 32 in fp64 and adds the
 *     blocks in int64).  fp64 matrix instructions would be exact too, but give no extra rate on gfx950
 *     (profiles/r04_ubench6_fp64_mfma.txt).
 * Levinson-Durbin, in the order written:  e_0 = r(0); for i = 1..order:
 *     acc = r(i); for j = 1..i-1: acc = acc + a[j]*r(i-j);      k_i = -acc / e_{i-1};
 *     for j = 1..i-1: a'[j] = a[j] + k_i*a[i-j];  a'[i] = k_i;  e_i = e_{i-1} * (1 - k_i*k_i).
 * Status: r(0) == 0: VS_LPC_SILENT; !(|k_i| < 1) or e_i <= 0: VS_LPC_UNSTABLE (the recursion stops).  In both cases err,
 * the taps A[1..order] and the formants are NaN.  Root finding that did not converge: VS_LPC_NO_ROOTS (the coefficients
 * and err stay valid, the formants are NaN, n_formants 0).  NO_ROOTS is the root finder's verdict, not part of the exact
 * definition: it marks ill-conditioned root sets, e.g. a frame with a single non-zero sample, whose A(z) = z^p has a
 * p-fold root at 0 (the iteration converges only linearly there).
 *
 * Formants (opts.n_formants > 0): the roots z of z^p + a_1 z^(p-1) + ... + a_p with Im z > 0 give
 *     f = fs*atan2(Im z, Re z)/(2*pi),   bw = -fs*log|z|/pi;
 * those with f_lo <= f <= fs/2 - f_lo, in ascending f, fill the first n_formants (f, bw) pairs; unused slots are NaN.
 * A successful recursion has every |k_i| < 1, so A(z) is minimum-phase and every root lies strictly inside the unit
 * circle: a fixed start on a circle of radius 0.9 cannot be far from any root.  The device runs Aberth-Ehrlich
 * iterations, one lane per root, from z_q = 0.9*exp(2*pi*i*(q + 0.25)/p); a frame has converged when every correction
 * of one iteration has |w| <= 1e-12; at most VS_LPC_MAX_ITER iterations, then one Newton step per root.  These doubles
 * are not bit-exact: against numpy.roots of the same A every f and bw agrees within VS_LPC_FORMANT_TOL_HZ, 1e-6 Hz
 * (held by tests/test_gpu_lpc.py on configs 2, 3 and 5 at orders 1..40; the largest difference measured, on config 3
 * at orders 12, 22 and 40, is 6e-11 Hz).  That holds where numpy.roots itself resolves the roots that finely: on noise,
 * constants, pure tones, squares, chirps and ramps (tests/hostile_signals.py) the largest difference is 2e-9 Hz, but on
 * a train of single-sample impulses at order 40 with pre-emphasis numpy.roots' own roots move 4e-4 Hz under one Newton
 * step against the same A, and the device lies 8e-5 Hz from them (profiles/lpc_hostile_signals.txt).
 *
 * Records: vs_lpc_frame at frames[i*frames_pitch + j] (frames_pitch >= every row's n_frames); formants (optional)
 * double [n_lanes][frames_pitch][2*n_formants]; coefs (optional) double [n_lanes][frames_pitch][order+1] with A[0] = 1,
 * ready for vs_lane.A.  Frames beyond a row's n_frames are left untouched, in all three.
 */
#define VS_LPC_MAX_WINDOW 16384
#define VS_LPC_MAX_FORMANTS 20
#define VS_LPC_MAX_ITER 100
#define VS_LPC_FORMANT_TOL_HZ 1e-6
#define VS_LPC_HAMMING 0
#define VS_LPC_RECTANGULAR 1
#define VS_LPC_SILENT 0x1    /* r(0) == 0 */
#define VS_LPC_UNSTABLE 0x2  /* some !(|k_i| < 1) or e_i <= 0 */
#define VS_LPC_NO_ROOTS 0x4  /* the root finder did not converge within VS_LPC_MAX_ITER */
typedef struct vs_lpc_opts {
  int32_t order;         /* 1..VS_MAX_ORDER, default VS_ORDER (22) */
  int32_t window;        /* VS_LPC_HAMMING (default) or VS_LPC_RECTANGULAR */
  int32_t pre_emphasis;  /* 0 (default: vowel -p 1 output is pre-emphasised already) or 1 */
  int32_t n_formants;    /* 0..VS_LPC_MAX_FORMANTS, default 5; 0 skips the root finding */
  double window_s;       /* seconds, default 0.025 */
  double hop_s;          /* seconds, default 0.010; 0: one centre frame */
  double f_lo;           /* Hz, default 50 */
  int64_t reserved_;     /* must be 0 */
} vs_lpc_opts;           /* 48 bytes */
typedef struct vs_lpc_frame {
  double r0, err;        /* (double)r(0); e_order (NaN unless status is 0 or VS_LPC_NO_ROOTS) */
  int32_t start;         /* s */
  int32_t n_formants;    /* pairs written (<= opts.n_formants) */
  int32_t status;        /* VS_LPC_* */
  int32_t reserved_;     /* 0 */
} vs_lpc_frame;          /* 32 bytes */
int vs_lpc_defaults(vs_lpc_opts *opts);
/* Host only, no device: frames of a row of len samples at rate fs (VS_ERR_RANGE / VS_ERR_ARG as vs_lpc_launch would
 * refuse the row), and the window table w[0..L) (window: VS_LPC_HAMMING or VS_LPC_RECTANGULAR, 2 <= L <= 16384). */
int vs_lpc_frames(const vs_lpc_opts *opts, int32_t fs, int32_t len, int32_t *n_frames);
int vs_lpc_window(int32_t L, int32_t window, int32_t *w);
/* Device pointers: pcm_dev [n_lanes][pitch] int16 (pitch >= n_samples), frames_dev vs_lpc_frame
 * [n_lanes][frames_pitch], formants_dev / coefs_dev as above or NULL.  fs and lengths (NULL: n_samples for every row)
 * are HOST arrays; the per-row records and one window table per distinct L go up through the context's retired-block
 * cache.  Enqueued on the context's stream -- behind a vs_plan_launch() into pcm_dev, say -- and returns without
 * waiting.  opts NULL: vs_lpc_defaults(). */
int vs_lpc_launch(vs_ctx *ctx, const vs_lpc_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                  size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
                  vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev);
/* Host buffers: upload (the three outputs too, so that what no frame covers stays as it was), vs_lpc_launch, download,
 * wait. */
int vs_lpc(vs_ctx *ctx, const vs_lpc_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
           const int32_t *fs, const int32_t *lengths, size_t frames_pitch, vs_lpc_frame *frames, double *formants,
           double *coefs);

/* ---- IAIF: blind vocal-tract estimation that leaves the source in (csrc/vs_iaif.hip) ------------------------------
 *
 * Linear prediction of speech absorbs part of the glottal spectrum into A(z), so the residual of vs_lpc's own sets is
 * not the flow (README, "inverse filtering").  Iterative Adaptive Inverse Filtering (Alku 1992) estimates the glottal
 * contribution with a low-order predictor, takes it out of the speech, and estimates the vocal tract from what is left;
 * then once more.  What comes out is one coefficient set per frame in the layout vs_lpc_launch writes, so
 * vs_inverse_launch, vs_track_launch and vs_measure_launch take it unchanged.  It is still a blind filter: README,
 * "IAIF", says with numbers what it gains over vs_lpc's sets and where it does worse.
 *
 * Per call: vs_iaif_opts.  p = order, g = glottal_order (1..p), rho = leak (0..1); window, n_formants, window_s, hop_s
 * and f_lo as in vs_lpc_opts.  There is no analysis pre-emphasis: the order-1 stage is the adaptive one.  L, H, n_frames
 * and the frame starts s are those of vs_lpc_frames with pre_emphasis 0 (vs_iaif_lpc_opts gives that vs_lpc_opts); the
 * window table is vs_lpc_window's integers w[n].
 *
 * Per frame, with M = p + 1: the extended frame e[n] = (double)x[s+n] for -M <= n < L, and 0 where s + n < 0.  Two
 * operators, both with zero state before n = -M:
 *     FIR_c(e)[n]:  acc = e[n]; for j = 1..len(c): acc = fma(c_j, e[n-j], acc)   (j ascending; e[n-j] = 0 for n-j < -M)
 *     INT(y)[n]  =  fma(rho, INT(y)[n-1], y[n])
 * LPC_q(y):
 *     1. v[n] = (double)w[n] * y[n], 0 <= n < L;
 *     2. r(k), k = 0..q:  acc = 0.0; for n = 0..L-1-k ascending: acc = fma(v[n], v[n+k], acc);
 *     3. the Levinson-Durbin of the LPC analysis above, word for word, at order q.
 * The four stages:
 *     1. c1 = LPC_1(e)                      2. V1 = LPC_p(FIR_c1(e))
 *     3. c2 = LPC_g(INT(FIR_V1(e)))         4. V2 = LPC_p(FIR_c2(e))
 * Every fma is a single rounding; everything else is rounded on its own (-ffp-contract=off, IEEE division), as in the
 * rest of this header.  That fixes one result per frame, whatever the launch geometry and whichever frames share a
 * workgroup, and the device equals the numpy restatement (tests/iaif_ref.py) bit for bit.  Adding a zero product to a
 * chain changes nothing that matters (a +0 accumulator stays +0, every v is finite), so the device pads its chunks with
 * v = 0.
 *
 * Status: the first stage that has r(0) == 0 sets VS_LPC_SILENT, the first that fails |k_i| < 1 or e_i > 0 sets
 * VS_LPC_UNSTABLE; either ends the frame.
 *
 * Records: vs_lpc_frame as vs_lpc writes it: r0 and err are those of stage 4 (a frame that ended earlier: r0 of the
 * stage that ended it; NaN err, taps and formants on failure), reserved_ 0.  coefs: V2 with element 0 = 1, double
 * [n_lanes][frames_pitch][p+1].  glottal (optional): c2 with element 0 = 1, [n_lanes][frames_pitch][g+1], NaN taps when
 * the frame failed at or before stage 3.  formants: of V2, through the root finder of the LPC analysis with the same
 * promise (VS_LPC_FORMANT_TOL_HZ against numpy.roots of the same A, not bit-exactness; VS_LPC_NO_ROOTS as there).
 * Frames beyond a row's n_frames are left untouched, in all four.
 */
typedef struct vs_iaif_opts {
  int32_t order;         /* p: 1..VS_MAX_ORDER, default VS_ORDER (22) */
  int32_t glottal_order; /* g: 1..order, default 4 */
  int32_t window;        /* VS_LPC_HAMMING (default) or VS_LPC_RECTANGULAR */
  int32_t n_formants;    /* 0..VS_LPC_MAX_FORMANTS, default 5; 0 skips the root finding */
  double window_s;       /* seconds, default 0.025 */
  double hop_s;          /* seconds, default 0.010; 0: one centre frame */
  double f_lo;           /* Hz, default 50 */
  double leak;           /* rho: 0..1, default 0.99 */
  int64_t reserved_;     /* must be 0 */
} vs_iaif_opts;          /* 56 bytes */
int vs_iaif_defaults(vs_iaif_opts *opts);
/* Host only, no device: the vs_lpc_opts with the same frame plan (pre_emphasis 0), so that vs_lpc_frames,
 * vs_track_from_lpc and vs_inverse_from_lpc serve IAIF unchanged.  The errors of vs_iaif_launch's options: VS_ERR_ARG /
 * VS_ERR_RANGE as vs_lpc_launch answers them, VS_ERR_RANGE for glottal_order outside 1..order or leak outside 0..1 (NaN
 * included), VS_ERR_ARG for a non-zero reserved_.  opts NULL: vs_iaif_defaults(). */
int vs_iaif_lpc_opts(const vs_iaif_opts *opts, vs_lpc_opts *lpc);
/* Device pointers as vs_lpc_launch, and glottal_dev [n_lanes][frames_pitch][glottal_order+1] or NULL.  Enqueued on the
 * context's stream and returns without waiting.  opts NULL: vs_iaif_defaults(). */
int vs_iaif_launch(vs_ctx *ctx, const vs_iaif_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                   size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
                   vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev, double *glottal_dev);
/* Host buffers: upload (the four outputs too, so that what no frame covers stays as it was), vs_iaif_launch, download,
 * wait. */
int vs_iaif(vs_ctx *ctx, const vs_iaif_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
            const int32_t *fs, const int32_t *lengths, size_t frames_pitch, vs_lpc_frame *frames, double *formants,
            double *coefs, double *glottal);

/* ---- coefficient tracks: a time-varying vocal-tract filter on int16 flow rows (csrc/vs_track.hip) ------------------
 *
 * The consumer of what vs_lpc produces: the all-pole filter of vs_filter (vowel_new.c:266-289) whose coefficient set
 * changes along the utterance.  Two uses: copy synthesis with ALL frames of a recording (vs_lpc_launch writes coefs_dev,
 * vs_track_launch reads it, chained on the context's stream without a host round trip), and glides between a few anchor
 * sets (a diphthong: tables 'a' and 'i') with the sets in between made on the device.
 *
 * Why glides go through reflection coefficients: the straight line between two stable direct-form sets leaves the
 * stable region (the ten tables, 33 steps per ordered pair: 246 of the 2970 interpolated sets have a root outside the
 * unit circle, the largest radius 1.0120), while every |k_i| < 1 is kept by convexity, hence every interpolated set is
 * minimum-phase (the same 2970 sets: largest root radius 0.9953; DESIGN.md says how to recompute both).
 *
 * Per call: order (1..VS_MAX_ORDER), mode (VS_TRACK_HOLD / VS_TRACK_GLIDE), sets_pitch, coefs double
 * [n_lanes][sets_pitch][order+1] (the layout vs_lpc_launch writes; element 0 of a set is ignored and taken as 1),
 * gains (optional) double [n_lanes][sets_pitch].  Per row a vs_track_row: K = n_sets sets, hop samples per set, offset,
 * length, gain, pre_emphasis.
 *
 * 1. Usable sets.  Set k is usable if A[1..order] are all finite (and its gain, when gains are given) and, in glide mode
 *    only, its step-down succeeds (every |k_i| < 1).  n_unusable counts the k in [0, K) that are not.  Forward fill:
 *    E_k = set k if usable, else E_{k-1}; E_{-1} = the first usable set.  No usable set at all: status VS_TRACK_NO_SET
 *    and the row's output (its first `length` samples) is all zeros.  (vs_lpc marks silent and unstable frames with NaN
 *    taps: its output is directly consumable.)  Hold mode does NOT test stability: like vs_filter, it runs what it is
 *    given.
 * 2. Which set.  For sample n let m = n - n % VS_TRACK_GROUP (the group start).  m < offset: k = 0, t = 0.  Else
 *    k = min((m - offset) / hop, K - 1) (integer division) and, in glide mode with k < K - 1,
 *    t = (double)(m - offset - k*hop) / (double)hop, else t = 0; m - offset and k*hop in 64-bit integers.
 *      hold:  a = the taps of E_k, G = the gain of E_k.
 *      glide: kappa_i = ka_i + t*(kb_i - ka_i), ka / kb the reflection coefficients of E_k / E_{k+1}; a = step-up of
 *             kappa; G = ga + t*(gb - ga).  (Always through the step-up, also at t = 0; K = 1 is a constant set.)
 * 3. Step-down, in this order (p = order, a^(p) = the set): for i = p..1: k_i = a^(i)_i; fail unless |k_i| < 1;
 *    d = 1.0 - k_i*k_i; for j = 1..i-1: a^(i-1)_j = (a^(i)_j - k_i*a^(i)_(i-j)) / d.
 *    Step-up: for i = 1..p: for j = 1..i-1: a'_j = a_j + kappa_i*a_(i-j); a'_i = kappa_i.
 *    Every product, sum and quotient is rounded on its own (-ffp-contract=off, IEEE division), in every arithmetic.
 * 4. The recurrence is vowel_new.c:266-289 with the set of step 2, the state carried across set changes and zero at
 *    n = 0: acc = (double)x[n] * (double)gain (then * G when gains are given; without gains there is no second product);
 *    for j = 1..order: acc = acc - a_j*y[n-j]; out[n] = round2int(acc - pre*y[n-1]); y[n] = acc.  VS_ARITH_EXACT as
 *    written; VS_ARITH_FMA uses the two partial sums of the wide filter kernel.  The track kernels have no
 *    single-precision form: a context set to VS_ARITH_F32 runs the FMA form, as it does on the wide path.
 *    The FMA form, with acc as above, fma(a, b, c) = a*b + c rounded once, P = 22 for order <= 22 and 40 above, and
 *    a_j = 0 for order < j <= P: p0 = acc; p1 = -(a_2*y[n-2]); for j = 3..P: odd j: p0 = fma(-a_j, y[n-j], p0), even j:
 *    p1 = fma(-a_j, y[n-j], p1); acc = fma(-a_1, y[n-1], p0 + p1); out[n] = round2int(fma(-pre, y[n-1], acc));
 *    y[n] = acc.  Steps 1 to 3 and the products (x*gain)*G are the same in every arithmetic.
 *    round2int clamps to [-32767, 32767] whatever the size of its argument, past int32 too; what is promised ends at a
 *    state that is not finite (hold mode runs unstable sets: they get there on a long enough row).
 *
 * Consequence (held by tests/test_gpu_track.py): hold mode with K = 1 is vs_filter with that set, byte for byte.
 * Samples past a row's length are left untouched.  The flow goes through HBM (6 bytes per sample, as on the wide
 * path): the track filter is not fused into the synthesis kernels.
 */
#define VS_TRACK_GROUP 24   /* samples: the kernels' register-window pass; a set never changes inside one */
#define VS_TRACK_HOLD 0
#define VS_TRACK_GLIDE 1
#define VS_TRACK_NO_SET 0x1 /* no usable set: the row's output is zeros */
typedef struct vs_track_row {
  int32_t n_sets;      /* K, 1..sets_pitch */
  int32_t hop;         /* samples per set, >= 1 */
  int32_t offset;      /* sample at which set 0's span (hold) / anchor 0 (glide) lies; may be negative */
  int32_t length;      /* samples of this row, <= n_samples; the rest of the output row is left untouched */
  float gain;          /* vowel -g */
  float pre_emphasis;  /* vowel -p */
} vs_track_row;        /* 24 bytes */
typedef struct vs_track_stat {
  int32_t status;      /* VS_TRACK_* */
  int32_t n_unusable;
} vs_track_stat;       /* 8 bytes */
/* Device pointers: flow_dev int16 [n_lanes][in_pitch], out_dev int16 [n_lanes][out_pitch] (both pitches >= n_samples),
 * coefs_dev / gains_dev as above (gains_dev may be NULL), stat_dev vs_track_stat [n_lanes] or NULL.  rows is a HOST
 * array of n_lanes records; it goes up through the context's retired-block cache.  Enqueued on the context's stream --
 * behind a vs_lpc_launch() into coefs_dev, say -- and returns without waiting.
 * NULL / zero sizes: VS_ERR_ARG; order, mode, hop, n_sets or length out of range: VS_ERR_RANGE; sizes beyond 2^31:
 * VS_ERR_UNSUPPORTED. */
int vs_track_launch(vs_ctx *ctx, int mode, int order, const int16_t *flow_dev, size_t in_pitch, int16_t *out_dev,
                    size_t out_pitch, size_t n_lanes, size_t n_samples, const vs_track_row *rows,
                    const double *coefs_dev, const double *gains_dev, size_t sets_pitch, vs_track_stat *stat_dev);
/* Host buffers (flow and pcm int16 [n_lanes][n_samples], stat optional): upload (pcm too, so that what lies past a
 * row's length stays as it was), vs_track_launch, download, wait. */
int vs_track(vs_ctx *ctx, int mode, int order, const int16_t *flow, int16_t *pcm, size_t n_lanes, size_t n_samples,
             const vs_track_row *rows, const double *coefs, const double *gains, size_t sets_pitch,
             vs_track_stat *stat);
/* Host only, no device.  vs_track_reflection: the step-down of A[0..order] (A[0] ignored) into k[0..order) = k_1..k_p;
 * VS_ERR_RANGE for a tap that is not finite or a |k_i| >= 1.  vs_track_glide_sets: n_sets >= 2 sets
 * coefs[n_sets][order+1], set s = step-up(k_from + ((double)s / (double)(n_sets - 1)) * (k_to - k_from)) with element
 * 0 = 1; VS_ERR_RANGE if either end fails its step-down. */
int vs_track_reflection(int order, const double *A, double *k);
int vs_track_glide_sets(int order, const double *A_from, const double *A_to, int n_sets, double *coefs);
/* The track row that plays the frames vs_lpc makes of a row of len samples at rate fs (opts NULL: vs_lpc_defaults()):
 * n_sets = vs_lpc_frames(), hop = H; glide: offset = s0 + L/2 (the frame centres are the anchors); hold:
 * offset = s0 + L/2 - H/2 (a frame governs the hop around its centre); length = len, gain 1, pre_emphasis 0.
 * VS_ERR_RANGE as vs_lpc_frames, and for a row without frames or options with hop_s == 0. */
int vs_track_from_lpc(const vs_lpc_opts *opts, int32_t fs, int32_t len, int mode, vs_track_row *row);

/* ---- inverse filtering: from speech back to the glottal flow (csrc/vs_inverse.hip) ----------------------------------
 *
 * The missing corner next to synthesis (source -> filter), vs_measure (the source), vs_lpc (the filter) and vs_track (a
 * time-varying filter): A(z) applied as an FIR filter to int16 speech rows, behind the inverse of the output
 * pre-emphasis.  With the filter known, what comes out is the flow again, and vs_measure reads the source's shimmer
 * where on the speech itself the vocal tract's ringing dilutes it (README, "inverse filtering").  With vs_lpc's own sets
 * of the recording (vs_lpc_launch -> vs_inverse_launch on one stream) it is the LPC residual; vs_track_launch of that
 * residual with the same coefs_dev gives the recording back (copy synthesis), and vs_measure_launch behind the inverse
 * measures the source -- all without a host round trip.  A blind filter is weaker than a known one: LPC absorbs part of
 * the glottal spectrum, so the residual is closer to the flow than the speech is, but it is not the flow.
 *
 * Per call: mode (VS_TRACK_HOLD / VS_TRACK_GLIDE), order (1..VS_MAX_ORDER), sets_pitch, coefs double
 * [n_lanes][sets_pitch][order+1] (the layout vs_lpc_launch writes; element 0 of a set is ignored).  There are no per-set
 * gains.  Per row a vs_inverse_row: K = n_sets, hop, offset, length as in vs_track_row, scale, de_emphasis.
 *
 * 1. to 3. are steps 1 to 3 of the coefficient tracks above without gains, word for word: usable sets, n_unusable and
 *    forward fill (no usable set at all: status VS_INVERSE_NO_SET, and the row's first `length` samples are zeros);
 *    which set governs a group of VS_TRACK_GROUP samples; the glide through step-down, interpolation and step-up, every
 *    operation rounded on its own in every arithmetic.  The same row (K, hop, offset, mode, sets) therefore selects the
 *    same taps a_1..a_order at the same sample in vs_track and here.
 * 4. With rho = (double)de_emphasis, c = (double)scale, s the int16 input and u[n] = 0 for n < 0:
 *      VS_ARITH_EXACT: u[n] = (double)s[n] + rho*u[n-1]; e = u[n]; for j = 1..order: e = e + a_j*u[n-j];
 *                      out[n] = round2int(e*c).  Every product and sum is rounded on its own.
 *      VS_ARITH_FMA (and VS_ARITH_F32, which runs this form as on the track path), P = 22 for order <= 22 and 40 above,
 *                      a_j = 0 for order < j <= P: u[n] = fma(rho, u[n-1], (double)s[n]); p0 = u[n]; p1 = a_2*u[n-2];
 *                      for j = 3..P: odd j: p0 = fma(a_j, u[n-j], p0), even j: p1 = fma(a_j, u[n-j], p1);
 *                      e = fma(a_1, u[n-1], p0 + p1); out[n] = round2int(e*c).
 *    round2int is the track kernels' (vowel_new.c:413-427: x + 1 where x - floor(x) > 0.5, then floor, then the clamp to
 *    [-32767, 32767] whatever the size of the value, past int32 too).  n_clipped counts the n < length at which the clamp
 *    changed the value, i.e. the floor lay outside [-32767, 32767].  What is promised ends where e is not finite (u
 *    always is: |u[n]| <= 32768*(n+1)).  Samples past a row's length are left untouched.  Input and output must not
 *    overlap.
 *
 * Consequences (held by tests/test_inverse_ref.py and tests/test_gpu_inverse.py):
 * (a) de_emphasis 0 gives u = s exactly.
 * (b) All taps 0, de_emphasis 0 and scale 1 copy the row, except that -32768 becomes -32767 (and counts as clipped).
 * (c) If vs_track ran a row (K, hop, offset, gain g, pre-emphasis mu) in mode M on the sets C, the inverse with the same
 *     (K, hop, offset, M, C), de_emphasis = mu and scale = 1/g undoes it up to the int16 rounding of what vs_track wrote:
 *     where no sample of that output clipped, |inverse - flow| <= 0.5*scale*sum_{n<N}|h[n]| + 1.5, h the impulse response
 *     of A(z)/(1 - rho z^-1) and N the row's length.  For a constant set this is derived, not measured: vs_track's
 *     output is x = (1 - mu z^-1)/A(z) applied to g*flow, plus a rounding r with |r[n]| <= 0.5; the inverse is linear, so
 *     it returns scale*(g*flow + h * r) = flow + scale*(h * r), and |h * r| <= 0.5*sum|h|; the 1.5 covers the inverse's own
 *     rounding to int16, the float rounding of scale against 1/g (under 0.01 at these sizes) and the double arithmetic
 *     of both filters.  Through a glide the sets change inside h; the tests hold the error to twice the larger bound of
 *     the two ends.
 *     For rho = 1 the bound grows with N (sum|h| does: 1/(1 - z^-1) is an integrator, which keeps every rounding error
 *     it has seen), and a clipped input sample makes a rho = 1 inverse drift from there to the end of the row.  For real
 *     recordings take de_emphasis < 1 (0.9 .. 0.99): the error of a clipped or rounded sample then dies away.
 */
#define VS_INVERSE_NO_SET 0x1 /* no usable set: the row's output is zeros */
typedef struct vs_inverse_row {
  int32_t n_sets;      /* K, 1..sets_pitch */
  int32_t hop;         /* samples per set, >= 1 */
  int32_t offset;      /* as vs_track_row.offset; may be negative */
  int32_t length;      /* samples of this row, <= n_samples; the rest of the output row is left untouched */
  float scale;         /* c: 1/gain of the synthesis to be undone; finite */
  float de_emphasis;   /* rho: the pre-emphasis to be undone, 0..1 */
} vs_inverse_row;      /* 24 bytes */
typedef struct vs_inverse_stat {
  int32_t status;      /* VS_INVERSE_* */
  int32_t n_unusable;
  int32_t n_clipped;
  int32_t reserved_;   /* 0 */
} vs_inverse_stat;     /* 16 bytes */
/* Device pointers: pcm_dev int16 [n_lanes][in_pitch], out_dev int16 [n_lanes][out_pitch] (both pitches >= n_samples; the
 * two must not overlap), coefs_dev as above, stat_dev vs_inverse_stat [n_lanes] or NULL.  rows is a HOST array of
 * n_lanes records; it goes up through the context's retired-block cache.  Enqueued on the context's stream -- behind a
 * vs_lpc_launch() into coefs_dev, say -- and returns without waiting.
 * NULL / zero sizes: VS_ERR_ARG; order, mode, hop, n_sets, length, de_emphasis (outside 0..1, NaN) or scale (not finite)
 * out of range: VS_ERR_RANGE; sizes beyond 2^31: VS_ERR_UNSUPPORTED. */
int vs_inverse_launch(vs_ctx *ctx, int mode, int order, const int16_t *pcm_dev, size_t in_pitch, int16_t *out_dev,
                      size_t out_pitch, size_t n_lanes, size_t n_samples, const vs_inverse_row *rows,
                      const double *coefs_dev, size_t sets_pitch, vs_inverse_stat *stat_dev);
/* Host buffers (pcm and flow int16 [n_lanes][n_samples], stat optional): upload (flow too, so that what lies past a
 * row's length stays as it was), vs_inverse_launch, download, wait. */
int vs_inverse(vs_ctx *ctx, int mode, int order, const int16_t *pcm, int16_t *flow, size_t n_lanes, size_t n_samples,
               const vs_inverse_row *rows, const double *coefs, size_t sets_pitch, vs_inverse_stat *stat);
/* Host only, no device.  The inverse row over the frames vs_lpc makes of a row of len samples at rate fs: n_sets, hop,
 * offset and length of vs_track_from_lpc (and its errors), scale 1, de_emphasis 0. */
int vs_inverse_from_lpc(const vs_lpc_opts *opts, int32_t fs, int32_t len, int mode, vs_inverse_row *row);

/* ---- glottal parameters: OQ, ClQ, SQ, QOQ and NAQ of every cycle (csrc/vs_glottal.hip) -------------------------------
 *
 * The reader of the pulse SHAPE, which is all that flowgen_shimmer -c and -k set: the time-domain quotients of every
 * cycle between the marks that vs_measure_launch left on the device, so that synthesis -> vs_inverse / vs_iaif ->
 * vs_measure -> vs_glottal runs on one stream.  Everything that places an instant is an exact integer; each quotient is
 * one IEEE division of two exactly representable doubles and the row means are summed in the order of the cycles (the
 * library is compiled with -ffp-contract=off), so the result does not depend on how the device goes about it.
 *
 * Per row: x[0..n_samples) int16, the row's vs_acoustic record, its marks marks[row*marks_pitch + j] as vs_measure_launch
 * wrote them with the same polarity p, y = p*x.  Options: level_open q_o (0..255), level_mid q_h (q_o..255), polarity.
 *
 * 1. Marks.  K = n_periods.  A record with VS_AC_TOO_SHORT or VS_AC_UNVOICED: status VS_GL_NO_CYCLES, all doubles NaN,
 *    n_cycles 0, no cycle record written.  Else K < 0: VS_GL_BAD_MARKS (the same empty record).  Else M = min(K + 1,
 *    marks_pitch); M < 3: VS_GL_NO_CYCLES.  Else the M marks are checked as a whole: m_0 >= 0, m_j < m_{j+1},
 *    m_{M-1} < n_samples.  If any of that fails: VS_GL_BAD_MARKS, and NO SAMPLE OF THE ROW IS READ.  Nothing the kernel
 *    reads or writes depends on the marks being vs_measure's: any M marks that pass are measured as written below.
 * 2. Cycles c = 1..M-2, each around its peak m_c.  lo = the first index of min y over [m_{c-1}, m_c); b = y[lo],
 *    a = y[m_c] - b, T = m_{c+1} - m_c.  a <= 0: the cycle is rejected with VS_GLC_ZERO_AMPLITUDE.  "n is above level q"
 *    means 256*(y[n] - b) > q*a (lo never is, m_c always is).  For q = q_o and q = q_h:
 *        open_q  = 1 + the largest n in [lo, m_c) that is not above q,
 *        close_q = the smallest n in (m_c, m_{c+1}) that is not above q.
 *    No close at q_o: the cycle is rejected with VS_GLC_NO_CLOSURE (a close at q_o implies one at q_h, and
 *    open_o <= open_h <= m_c < close_h <= close_o).  d = max over n in [m_c, close_o) of y[n] - y[n+1] (> 0: the sample
 *    before close_o is above q_o, close_o is not); gci = 1 + the first n that attains d.
 * 3. Per accepted cycle, in double:
 *        OQ  = (double)(close_o - open_o) / (double)T         ClQ = (double)(close_o - m_c) / (double)T
 *        SQ  = (double)(m_c - open_o) / (double)(close_o - m_c)
 *        QOQ = (double)(close_h - open_h) / (double)T         NAQ = (double)a / ((double)d * (double)T)
 *    (QOQ: Alku's quasi-open quotient, the time above half the amplitude; NAQ: the normalised amplitude quotient, the
 *    amplitude over the steepest closing slope, per period.)
 * 4. The row record: for each of the five, s = 0.0; for the accepted c ascending s = s + v_c; mean = s / (double)n_cycles.
 *    n_cycles counts the accepted cycles, n_rejected the rejected ones; VS_GL_REJECTED if some cycle was rejected, and
 *    VS_GL_ALL_REJECTED as well, with the doubles NaN, if all were.  The record always covers all M - 2 cycles.
 * 5. Cycle records (optional) [n_lanes][cycles_pitch]: cycle c goes to slot c - 1 when c - 1 < cycles_pitch; every other
 *    slot is left untouched.  peak = m_c, period = T, trough = lo, amp = a, open / close = open_o / close_o, open_mid /
 *    close_mid = open_h / close_h, gci, decl = d, status = VS_GLC_* (0: accepted).  A rejected cycle has -1 in the five
 *    positions from open to gci and decl 0.
 *
 * On this project's own pulses (DC 0, no glottal noise -n), at level_open 0: peak - open = T2 - 1 and close - peak =
 * T3 - T2 for every cycle, T2 = ceil(0.5*cq*P) the rising and T3 - T2 the falling half of fg:317-330, and period is the
 * cycle log's T (tests/test_glottal_ref.py).  The way back to the command line, each within the one-sample quantisation
 * of rise and fall:  cq ~ 2*(rise + 1)/P,   K ~ (1 - DC/amp)/(1 - cos(pi*fall/T2)).  With flowgen -n the closed phase
 * carries noise and b is that noise's minimum: level 0 then means nothing and level_open has to lie above the noise
 * (at -n 20, OQ is usable from about 20 % = level 51 upwards).  The default 26 is 10 %; level_mid 128 is the half
 * amplitude of QOQ.
 */
#define VS_GL_NO_CYCLES 0x1       /* the measurement gave up, or fewer than three marks */
#define VS_GL_BAD_MARKS 0x2       /* n_periods negative, or the marks not increasing within [0, n_samples) */
#define VS_GL_REJECTED 0x4        /* some cycle was rejected */
#define VS_GL_ALL_REJECTED 0x8    /* every cycle was: the doubles are NaN */
#define VS_GLC_ZERO_AMPLITUDE 0x1 /* a <= 0 */
#define VS_GLC_NO_CLOSURE 0x2     /* y stays above level_open up to the next mark */
typedef struct vs_glottal_opts {
  int32_t level_open; /* q_o in 256ths of the amplitude, 0..255, default 26 */
  int32_t level_mid;  /* q_h, level_open..255, default 128 */
  int32_t polarity;   /* that of the vs_measure_launch that wrote the marks */
  int32_t reserved_;  /* must be 0 */
} vs_glottal_opts;    /* 16 bytes */
typedef struct vs_glottal_rec {
  double oq, clq, sq, qoq, naq; /* means over the accepted cycles */
  int32_t n_cycles, n_rejected, status, reserved_;
} vs_glottal_rec;     /* 56 bytes */
typedef struct vs_glottal_cycle {
  int32_t peak, period, trough, amp, open, close, open_mid, close_mid, gci, decl, status, reserved_;
} vs_glottal_cycle;   /* 48 bytes */
int vs_glottal_defaults(vs_glottal_opts *opts);
/* Device pointers: pcm_dev [n_lanes][pitch] int16 (pitch >= n_samples), meas_dev and marks_dev [n_lanes][marks_pitch] as
 * the vs_measure_launch before it on the context's stream wrote them, out_dev vs_glottal_rec [n_lanes], cycles_dev
 * vs_glottal_cycle [n_lanes][cycles_pitch] or NULL.  There are no per-row host arrays and nothing is uploaded.  Returns
 * without waiting.  opts NULL: vs_glottal_defaults().
 * NULL pointers, zero sizes, marks_pitch 0, a cycles_dev with cycles_pitch 0, a polarity other than +-1 or a non-zero
 * reserved_: VS_ERR_ARG; levels out of range: VS_ERR_RANGE; sizes beyond 2^31: VS_ERR_UNSUPPORTED. */
int vs_glottal_launch(vs_ctx *ctx, const vs_glottal_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                      size_t n_samples, const vs_acoustic *meas_dev, const int32_t *marks_dev, size_t marks_pitch,
                      vs_glottal_rec *out_dev, vs_glottal_cycle *cycles_dev, size_t cycles_pitch);
/* Host buffers: upload, vs_measure_launch, vs_glottal_launch, download, one wait.  meas, marks (filled with -1 past the
 * last mark, as in vs_measure) and out are required, cycles is optional (slots past a row's cycles come back as they
 * went in).  VS_ERR_ARG when the polarities of mopts and gopts differ. */
int vs_glottal(vs_ctx *ctx, const vs_measure_opts *mopts, const vs_glottal_opts *gopts, const int16_t *pcm, size_t pitch,
               size_t n_lanes, size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t marks_pitch,
               vs_acoustic *meas, int32_t *marks, vs_glottal_rec *out, vs_glottal_cycle *cycles, size_t cycles_pitch);

/* ---- closed-phase covariance LPC: a blind filter that reaches the flow (csrc/vs_cplpc.hip) ----------------------------
 *
 * While the glottis is closed the speech is the free response of the vocal tract alone, so covariance-method linear
 * prediction over only those samples estimates A(z) with no source in it.  Where each cycle closes is what
 * vs_glottal_launch leaves on the device (vs_glottal_cycle: close, gci, peak, period), typically measured on a first-pass
 * residual of the same row: an FIR inverse has no delay, so its instants are the speech's.  The chain vs_iaif_launch ->
 * vs_inverse_launch -> vs_measure_launch -> vs_glottal_launch -> vs_cplpc_launch -> vs_inverse_launch runs on one stream.
 * Every covariance is an exact integer and the solve is evaluated in the order written here (the library is compiled with
 * -ffp-contract=off; fma(a, b, c) = a*b + c rounded once), so the result is fixed bit for bit, whatever the launch
 * geometry.  README, "vclosed", says with numbers what the sets gain over IAIF's and where they do worse.
 *
 * Per call: vs_cplpc_opts; p = order.  Per row: x[0..len) int16, the row's vs_glottal_rec and its
 * vs_glottal_cycle[cycles_pitch] as vs_glottal_launch wrote them.
 *
 * 1. Cycles.  C = min(n_cycles + n_rejected, cycles_pitch); C = 0 when the record has VS_GL_NO_CYCLES or VS_GL_BAD_MARKS,
 *    or when that sum is negative.  Only slots c < C with status == 0 and period > 0 are used.
 * 2. The span of a cycle, all in 64-bit integers: b = anchor_field + delay (anchor_field: the cycle's close, gci or peak,
 *    by opts.anchor), e = b + ((int64)span_q * period) / 256.
 * 3. Acceptance.  A span is accepted iff 0 <= b, and e <= len and e - b >= p + 1, and no n in [b, e) has x[n] >= 32767
 *    or x[n] <= -32767 (a sample at the clamp of round2int, or beyond it in a foreign file: one such sample inside a
 *    span moves a set by more than 1 in some tap).
 * 4. Garbage in the records.  Nothing outside [0, len) is ever read, whatever the records hold; the kernel trusts no
 *    field of them.  Overlapping spans (fabricated records) both count.
 * 5. Frames.  window_s == 0: one frame, start = 0, and it pools every accepted span; the row a consumer (vs_inverse_row,
 *    vs_track_row) gives such a set is n_sets 1, hop 1, offset 0.  window_s > 0: L, H, n_frames and the starts s_j of
 *    vs_lpc_frames with pre-emphasis 0 (vs_cplpc_lpc_opts gives that vs_lpc_opts, so vs_track_from_lpc and
 *    vs_inverse_from_lpc serve unchanged); frame j pools the accepted spans with s_j <= b and e <= s_j + L.
 * 6. Covariance, exact.  phi(i,k) = sum over the pooled spans of sum_{n=b+p}^{e-1} x[n-i]*x[n-k], 0 <= i, k <= p;
 *    n_eq = sum (e - b - p).  Spans are pooled in the order of their slots; an accepted span of the frame (step 3 comes
 *    first: a span with a clamped sample is skipped, not counted) that would bring the frame's n_eq to 2^31 or more is
 *    not pooled, and none behind it is (only fabricated, overlapping records get there: real spans do
 *    not overlap, so n_eq < len).  Every product is below 2^30 and there are fewer than 2^31 equations, so each phi is
 *    an exact int64 and the device may sum in any order and by any method.
 * 7. min = min_equations, or 2*p when that is 0.  n_eq < min: status VS_CP_FEW_EQUATIONS; taps, err and formants NaN;
 *    r0 = (double)phi(0,0).  Else phi(0,0) == 0: VS_LPC_SILENT, with the same NaNs.
 * 8. The solve, on c_ik = (double)phi(i,k) (the C conversion: nearest-even).  LDL^T without square roots, for j = 1..p:
 *        for k < j: u_k = l_jk * d_k;
 *        d_j = c_jj, then for k = 1..j-1 ascending: d_j = fma(-l_jk, u_k, d_j);
 *        unless d_j > 0 and finite: VS_CP_SINGULAR (NaN taps, err and formants), and stop;
 *        for i = j+1..p: t = c_ij; for k = 1..j-1 ascending: t = fma(-l_ik, u_k, t); l_ij = t / d_j.
 *    Forward: z_i = -c_i0; for k = 1..i-1 ascending: z_i = fma(-l_ik, z_k, z_i).  y_i = z_i / d_i.
 *    Back, for i = p..1: a_i = y_i; for k = i+1..p ascending: a_i = fma(-l_ki, a_k, a_i).
 *    err = c_00; for i = 1..p ascending: err = fma(a_i, c_0i, err).  r0 = c_00.
 * 9. Minimum phase.  The covariance method does not promise it: the step-down of the coefficient tracks (step 3 there)
 *    runs on the set, and if it fails the status gets VS_CP_NOT_MINIMUM_PHASE.  The taps and err stay valid: the inverse
 *    is an FIR filter and hold mode runs what it is given; glide mode counts the set unusable by its own rule.
 * 10. Formants.  Only for frames with status 0, through the root finder of the LPC analysis with the same promise
 *    (VS_LPC_FORMANT_TOL_HZ against numpy.roots of the same A, not bit-exactness; VS_LPC_NO_ROOTS as there).  Otherwise
 *    NaN and n_formants 0.
 *
 * Records: vs_lpc_frame exactly as vs_lpc lays it out (start = s_j, or 0; reserved_ 0); coefs double
 * [n_lanes][frames_pitch][p+1] with element 0 = 1, the layout vs_inverse_launch and vs_track_launch read; formants as
 * vs_lpc's; counts (optional) int32 [n_lanes][frames_pitch][2] = {spans pooled, n_eq}.  Frames beyond a row's n_frames
 * are left untouched, in all four.
 *
 * What err / r0 tells: on a span set that really was closed it is the rounding noise of the recording (1e-8 .. 1e-7 on
 * this project's vowels); a first pass that marked every other cycle (an octave error) runs the spans into the next open
 * phase, and err / r0 rises a hundredfold while the set goes off by units.  Bound the pitch range of the first pass so
 * that it excludes the octave below (README, "vclosed").
 */
#define VS_CP_ANCHOR_CLOSE 0
#define VS_CP_ANCHOR_GCI 1
#define VS_CP_ANCHOR_PEAK 2
#define VS_CP_FEW_EQUATIONS 0x10      /* n_eq < min_equations */
#define VS_CP_SINGULAR 0x20           /* some d_j <= 0 or not finite */
#define VS_CP_NOT_MINIMUM_PHASE 0x40  /* the step-down failed: taps and err are valid */
typedef struct vs_cplpc_opts {
  int32_t order;          /* p: 1..VS_MAX_ORDER, default VS_ORDER */
  int32_t anchor;         /* VS_CP_ANCHOR_CLOSE (default), _GCI or _PEAK */
  int32_t delay;          /* samples from the anchor to the span's start, -32768..32767, default 4 */
  int32_t span_q;         /* span length in 256ths of the cycle's period, 1..256, default 77 (0.30) */
  int32_t min_equations;  /* 0 (default): 2*order; else >= order */
  int32_t n_formants;     /* 0..VS_LPC_MAX_FORMANTS, default 5; 0 skips the root finding */
  double window_s;        /* 0 (default): one set per row from all its spans; > 0: frames as vs_lpc */
  double hop_s;           /* seconds, default 0.010; read when window_s > 0 */
  double f_lo;            /* Hz, default 50 */
  int64_t reserved_;      /* must be 0 */
} vs_cplpc_opts;          /* 56 bytes */
int vs_cplpc_defaults(vs_cplpc_opts *opts);
/* Host only, no device.  vs_cplpc_frames: the frames of a row of len samples at rate fs: 1 when window_s == 0, else
 * vs_lpc_frames of the same plan.  vs_cplpc_lpc_opts: the vs_lpc_opts with the same frame plan (rectangular window,
 * pre_emphasis 0) when window_s > 0; with window_s == 0 it checks the options and leaves in *lpc the order, n_formants,
 * f_lo and hop_s with window_s 0, which vs_lpc_frames refuses: there is no frame plan then.  The errors of
 * vs_cplpc_launch's options: VS_ERR_ARG for a NULL, a non-zero reserved_ and what vs_lpc_launch answers so (n_formants,
 * f_lo, values that are not finite, a negative hop_s); VS_ERR_RANGE for order, anchor, delay, span_q, min_equations, a
 * negative window_s, and for window_s or hop_s as vs_lpc_launch refuses them.  opts NULL: vs_cplpc_defaults(). */
int vs_cplpc_frames(const vs_cplpc_opts *opts, int32_t fs, int32_t len, int32_t *n_frames);
int vs_cplpc_lpc_opts(const vs_cplpc_opts *opts, vs_lpc_opts *lpc);
/* Device pointers: pcm_dev [n_lanes][pitch] int16 (pitch >= n_samples), glottal_dev vs_glottal_rec [n_lanes] and cycles_dev
 * vs_glottal_cycle [n_lanes][cycles_pitch] as the vs_glottal_launch before it on the context's stream wrote them,
 * frames_dev vs_lpc_frame [n_lanes][frames_pitch], formants_dev / coefs_dev / counts_dev as above or NULL.  fs and lengths
 * (NULL: n_samples for every row) are HOST arrays, as for vs_lpc_launch; the per-row records go up through the context's
 * retired-block cache.  Enqueued on the context's stream, returns without waiting.  opts NULL: vs_cplpc_defaults().
 * NULL pointers, zero sizes, cycles_pitch 0, frames_pitch 0 (here and in vs_cplpc): VS_ERR_ARG; a row with more frames
 * than frames_pitch: VS_ERR_RANGE; sizes beyond 2^31: VS_ERR_UNSUPPORTED. */
int vs_cplpc_launch(vs_ctx *ctx, const vs_cplpc_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                    size_t n_samples, const int32_t *fs, const int32_t *lengths, const vs_glottal_rec *glottal_dev,
                    const vs_glottal_cycle *cycles_dev, size_t cycles_pitch, size_t frames_pitch,
                    vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev, int32_t *counts_dev);
/* Host buffers: upload (the four outputs too, so that what no frame covers stays as it was), vs_cplpc_launch, download,
 * wait. */
int vs_cplpc(vs_ctx *ctx, const vs_cplpc_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
             const int32_t *fs, const int32_t *lengths, const vs_glottal_rec *glottal, const vs_glottal_cycle *cycles,
             size_t cycles_pitch, size_t frames_pitch, vs_lpc_frame *frames, double *formants, double *coefs,
             int32_t *counts);

/* ---- pitch track: per-frame F0, voicing and one Viterbi path (csrc/vs_pitch.hip) ------------------------------------
 *
 * vs_measure takes ONE period estimate from ONE window in the middle of a row.  The track asks every frame of the row
 * instead -- candidates per frame, one dynamic-programming path through them (Praat's "To Pitch (ac)", RAPT) -- so that
 * an octave error of one window, a gliding F0 and an unvoiced stretch are each decided with their neighbours in view.
 * Everything is an integer: the device and any restatement agree bit for bit.
 *
 * Per row: x[0..len) int16, the rate fs, y = x (the sign of y plays no part).  tmin and tmax are vs_measure's, from
 * f0_min and f0_max by the same formulas, with the same VS_ERR_RANGE rules and VS_AC_MAX_LAG.  W = 2*tmax,
 *     H = (int)floor(hop_s * fs + 0.5)                   H < 1 (or beyond 2^31 - 1): VS_ERR_RANGE
 *     n_frames = len >= 3*tmax + 2 ? 1 + (len - (3*tmax + 2)) / H : 0
 * Frame f starts at s = f*H and reads y[s .. s + W + tmax].
 *
 * A. Per frame, exactly (every sum is below 2^42):
 *        r(t) = sum_{k<W} y[s+k] * y[s+k+t],   e(t) = sum_{k<W} y[s+k+t]^2      for t in [tmin-1, tmax+1];   r0 = e(0)
 *        q(t) = (r(t) > 0 && r0 + e(t) > 0) ? (r(t) << 16) / (r0 + e(t)) : 0     (int64 division; 0..32768)
 *    q is 1 - d(t) / (r0 + e(t)) in Q16/2 with d the squared-difference function: the normalisation that needs no root.
 *    r0 < W * silence_rms^2 (int64): the frame is VS_PT_SILENT and has no candidate.  Else the candidates are every t in
 *    [tmin, tmax] with q(t) > 0, q(t) > q(t-1) and q(t) >= q(t+1); of these the VS_PT_MAX_CAND best by (q descending,
 *    t ascending) are kept and stored in ascending t: cand_lag[0..n_cand), cand_q[0..n_cand), the other slots 0.  A
 *    frame that is not silent and has none is VS_PT_NO_CANDIDATE.
 *
 * B. Costs.  Lg[t] = (int)floor(256*log2(t) + 0.5) (vs_pitch_log2_table; no value is closer than 2.4e-4 to a rounding
 *    tie for t <= VS_AC_MAX_LAG).  State 0 of a frame is "unvoiced", states 1..n_cand its candidates in ascending lag.
 *        D(0) = voicing_q,      D(j) = cand_q[j-1] + ((octave_q * (Lg[tmax] - Lg[cand_lag[j-1]])) >> 8)
 *        trans(0, 0) = 0,   trans(0, j) = trans(i, 0) = vuv_q,   trans(i, j) = (jump_q * |Lg[t_i] - Lg[t_j]|) >> 8
 *    (products and sums in int64).
 *
 * C. Path.  delta_0(j) = D_0(j);  delta_f(j) = D_f(j) + max_i (delta_{f-1}(i) - trans(i, j)) over the states i of frame
 *    f-1, ties to the smallest i, which is back[j] (back[j] = 0 for the j beyond n_cand and in frame 0).  The last frame
 *    takes the state of the largest delta, ties to the smallest j; each frame before it the back[] of its successor's
 *    state.  lag = the chosen state's lag (0: state 0, and VS_PT_UNVOICED is set), q = its cand_q (voicing_q for state 0).
 *
 * Records: frame f of row i at frames[i * frames_pitch + f]; what lies past a row's n_frames is not touched.
 */
#define VS_PT_MAX_CAND 7
#define VS_PT_SILENT 0x1        /* r0 < W * silence_rms^2: no candidates were looked for */
#define VS_PT_UNVOICED 0x2      /* the path chose state 0 */
#define VS_PT_NO_CANDIDATE 0x4  /* not silent, and no lag qualified */
#define VS_PT_MAX_COST (1 << 20)
typedef struct vs_pitch_opts {
  float f0_min;         /* Hz, default 50 */
  float f0_max;         /* Hz, default 500 */
  int32_t voicing_q;    /* Q15 like the three below, each 0..VS_PT_MAX_COST; default 14746 (Praat's 0.45) */
  int32_t octave_q;     /* default 328 (0.01) */
  int32_t jump_q;       /* default 11469 (0.35) */
  int32_t vuv_q;        /* default 4588 (0.14) */
  int32_t silence_rms;  /* 0..32767, default 16 */
  int32_t reserved_;    /* must be 0 */
  double hop_s;         /* seconds, default 0.010 */
} vs_pitch_opts;        /* 40 bytes */
typedef struct vs_pitch_frame {
  int64_t r0;
  int32_t start, lag, q, status;
  int32_t n_cand, reserved_;
  int32_t cand_lag[VS_PT_MAX_CAND], cand_q[VS_PT_MAX_CAND];
  uint8_t back[VS_PT_MAX_CAND + 1];
} vs_pitch_frame;       /* 96 bytes */
int vs_pitch_defaults(vs_pitch_opts *opts);
/* Host only, no device.  vs_pitch_frames: n_frames of a row of len samples at rate fs (VS_ERR_ARG for a NULL, options
 * that are not finite, a cost or silence_rms outside its range, a non-zero reserved_; VS_ERR_RANGE for the lag bounds, H
 * and len < 0).  vs_pitch_log2_table: lg[t] = Lg[t] for t in [1, n), lg[0] = 0; n in 1..VS_AC_MAX_LAG + 1. */
int vs_pitch_frames(const vs_pitch_opts *opts, int32_t fs, int32_t len, int32_t *n_frames);
int vs_pitch_log2_table(int32_t n, int32_t *lg);
/* Device pointers: pcm_dev [n_lanes][pitch] int16 (pitch >= n_samples), frames_dev vs_pitch_frame [n_lanes][frames_pitch].
 * fs and lengths (NULL: n_samples for every row) are HOST arrays; the row records and the Lg table go up through the
 * context's retired-block cache.  Enqueued on the context's stream, returns without waiting.  opts NULL:
 * vs_pitch_defaults().  NULL pointers, zero sizes and frames_pitch 0: VS_ERR_ARG; a row with more frames than
 * frames_pitch: VS_ERR_RANGE; sizes (and the frames of the call together) beyond 2^31: VS_ERR_UNSUPPORTED. */
int vs_pitch_launch(vs_ctx *ctx, const vs_pitch_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                    size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
                    vs_pitch_frame *frames_dev);
/* Host buffers: upload (the records too, so that what no frame covers stays as it was), vs_pitch_launch, download, wait. */
int vs_pitch(vs_ctx *ctx, const vs_pitch_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
             const int32_t *fs, const int32_t *lengths, size_t frames_pitch, vs_pitch_frame *frames);

/* ---- guided marks: the pitch track steers the measurement's cycle walk (csrc/vs_guided.hip) -------------------------
 *
 * vs_measure walks a whole row with every period inside [2/3, 3/2] * P0 of ONE estimate.  The guided walk takes the
 * period from the pitch track instead, frame by frame, and walks only where the track is voiced: a gliding F0 is
 * followed, a pause is left out, and an octave error of one window does not reach the marks.  Everything that places a
 * mark is an exact integer.
 *
 * Per row: x[0..len) int16, the rate fs, the polarity p, y = p * x, and the row's vs_pitch_frame records as
 * vs_pitch_launch wrote them.  tmin, tmax, H and n_frames come from f0_min, f0_max and hop_s by the formulas and
 * refusals of the pitch track: the caller passes the options of the vs_pitch_launch that wrote the frames.
 * C = tmax + tmax/2 (integer division); the centre of frame f is f*H + C.
 *
 * A. Voiced.  Frame f is voiced iff tmin <= lag_f <= tmax.  Nothing else of the record is trusted but q (stage E): a
 *    lag outside the range, whatever wrote it, counts as unvoiced.
 *
 * B. Runs.  A run is a maximal stretch [fa, fb] of voiced frames.  Trim: fa += edge_frames if fa > 0; fb -= edge_frames
 *    if fb < n_frames - 1 (the side at the row's end is not trimmed: there is nothing unvoiced behind it that the
 *    frame's window could have reached into).  A run is kept iff fb - fa + 1 >= min_frames.  VS_MG_ALL walks all kept
 *    runs in order; VS_MG_LONGEST only the one with the most frames after trimming, ties to the first.
 *
 * C. Samples.  The frame of sample n is f(n) = 0 for n <= C, else min(n_frames - 1, (n - C + H/2) / H).  The samples of
 *    a run [fa, fb] are [a, b) with
 *        a = fa == 0 ? 0 : C + fa*H - H/2,        b = fb == n_frames - 1 ? len : min(len, C + (fb+1)*H - H/2):
 *    exactly the n with fa <= f(n) <= fb.  Runs do not touch, so the walk of a row is one forward pass.
 *
 * D. The walk in a run, ties to the first index.  m_0 = first argmax of y over [a, min(a + lag_fa, b)).  After mark m_i:
 *    P = the lag of frame f(m_i) (that frame is always in the run),
 *        lo1 = max(tmin, (2P+2)/3),   hi1 = min(tmax, 3P/2),   d = (P+3)/4.
 *    The window of the run's second mark is m_0 + [lo1, hi1]; afterwards it is
 *        m_i + [max(lo1, T_i - d), min(hi1, T_i + d)],   T_i = m_i - m_{i-1},
 *    and if that is empty (the track jumped) m_i + [lo1, hi1] again.  m_{i+1} = first argmax of y over the window.  The
 *    run's walk stops at the first window whose upper end is >= b.  Periods and amplitudes exist only inside a run:
 *    a_i = y[m_i] - min y over [m_{i-1}, m_i).
 *
 * E. Summary: the vs_acoustic record, with Praat's sums taken over neighbours inside one run only.  K = the count of all
 *    periods, N2 / N3 / N5 = the counts of adjacent pairs / triples / quintuples of periods within runs.
 *        Tm = (double)sum T / K,  f0_hz = fs / Tm,  Am = (double)sum a / K
 *        jitter_local = ((double)sum|dT| / (double)N2) / Tm          jitter_abs_s = ((double)sum|dT| / (double)N2) / fs
 *        jitter_rap   = ((double)sum3 / (3.0*(double)N3)) / Tm       jitter_ppq5  = ((double)sum5 / (5.0*(double)N5)) / Tm
 *    the shimmer fields alike on a with Am; shimmer_db = (the sum of |20*log10(a_{i+1}/a_i)| in mark order) / (double)N2.
 *    A field whose count is 0 is NaN; every shimmer field is NaN when some a_i <= 0.  With one run every field equals
 *    what vs_measure's formulas give on the same marks (N2 = K-1, N3 = K-2, N5 = K-4).
 *    hnr_db comes from the track: Q = sum of clamp(q_f, 0, 32768) over the frames of the walked (trimmed, kept) runs
 *    (int64), nF their count; rho = (double)Q / (32768.0 * (double)nF), clamped to [1e-10, 1 - 1e-10];
 *    hnr_db = 10*log10(rho / (1 - rho)).
 *
 * Records: p0 = the lag of frame f(first_mark), first_mark = m_0 of the first walked run (-1 and p0 0 without one),
 * n_periods = K.  Status: VS_AC_TOO_SHORT when n_frames == 0, VS_AC_UNVOICED when no run is kept (both: all doubles NaN,
 * no marks), VS_AC_FEW_PERIODS when K < 2, VS_AC_ZERO_AMPLITUDE as in vs_measure.
 * Marks (optional): all marks of all walked runs, one behind the other, in marks[i * marks_pitch + j] for
 * j < marks_pitch; the rest of the row is untouched.  vs_guided_rec: the counts of the row.  vs_guided_seg (optional):
 * run k of the row at segs[i * seg_pitch + k] for k < seg_pitch; runs beyond seg_pitch are walked and summarised but not
 * recorded, and slots past n_segments are untouched.
 *
 * In VS_MG_LONGEST mode the record and the marks are those of one contiguous train: vs_glottal_launch and everything
 * behind it take them unchanged.  In VS_MG_ALL mode with more than one run they are NOT input for vs_glottal_launch,
 * which would read the K + n_segments marks as one train and measure the pauses as cycles.
 */
#define VS_MG_ALL 0
#define VS_MG_LONGEST 1
#define VS_MG_MAX_EDGE 16
typedef struct vs_guided_opts {
  float f0_min;         /* Hz, default 50: the three the pitch track shares, as given to the vs_pitch_launch before */
  float f0_max;         /* Hz, default 500 */
  int32_t polarity;     /* +1 (default): marks on maxima; -1: on minima */
  int32_t segments;     /* VS_MG_ALL (default) or VS_MG_LONGEST */
  int32_t edge_frames;  /* 0..VS_MG_MAX_EDGE, default 1: frames cut from a run's side that borders an unvoiced frame */
  int32_t min_frames;   /* >= 1, default 3: a shorter run (after the cut) is not walked */
  double hop_s;         /* seconds, default 0.010 */
} vs_guided_opts;       /* 32 bytes */
typedef struct vs_guided_rec {
  int32_t n_segments, n_marks, n_frames_walked, reserved_;
} vs_guided_rec;        /* 16 bytes */
typedef struct vs_guided_seg {
  int32_t first_frame, n_frames, first_mark_index, n_marks;
} vs_guided_seg;        /* 16 bytes */
int vs_guided_defaults(vs_guided_opts *opts);
/* Host only, no device: tmin, tmax, H, n_frames and C of a row (each pointer may be NULL).  VS_ERR_ARG for options that
 * are not finite, a polarity that is not +-1 or a segments value that is neither mode; VS_ERR_RANGE for the lag bounds,
 * H, len < 0, edge_frames and min_frames. */
int vs_guided_plan(const vs_guided_opts *opts, int32_t fs, int32_t len, int32_t *tmin, int32_t *tmax, int32_t *hop,
                   int32_t *n_frames, int32_t *centre);
/* Device pointers: pcm_dev [n_lanes][pitch] int16 (pitch >= n_samples), frames_dev vs_pitch_frame [n_lanes][frames_pitch]
 * (read only), out_dev vs_acoustic [n_lanes], marks_dev int32 [n_lanes][marks_pitch] or NULL, rec_dev vs_guided_rec
 * [n_lanes], segs_dev vs_guided_seg [n_lanes][seg_pitch] or NULL.  fs and lengths (NULL: n_samples for every row) are
 * HOST arrays; the row records go up through the context's retired-block cache, which also lends the plan kernel's
 * scratch.  Enqueued on the context's stream, returns without waiting.  opts NULL: vs_guided_defaults().  NULL pointers,
 * zero sizes, frames_pitch 0, a marks_dev with marks_pitch 0 and a segs_dev with seg_pitch 0: VS_ERR_ARG; a row with
 * more frames than frames_pitch: VS_ERR_RANGE; sizes beyond 2^31: VS_ERR_UNSUPPORTED. */
int vs_guided_launch(vs_ctx *ctx, const vs_guided_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                     size_t n_samples, const int32_t *fs, const int32_t *lengths, const vs_pitch_frame *frames_dev,
                     size_t frames_pitch, vs_acoustic *out_dev, int32_t *marks_dev, size_t marks_pitch,
                     vs_guided_rec *rec_dev, vs_guided_seg *segs_dev, size_t seg_pitch);
/* Host buffers: upload, vs_pitch_launch, vs_guided_launch, download, one wait.  pitch_opts (NULL: vs_pitch_defaults())
 * gives the track's costs and silence_rms; its f0_min, f0_max and hop_s are replaced by those of opts.  frames (NULL:
 * not wanted) receives the track's records, [n_lanes][frames_pitch] (uploaded first, like vs_pitch's); frames_pitch is
 * needed either way.  The marks come back -1 past the last; the segment records go up first, so the slots past a row's
 * runs come back as they went. */
int vs_guided(vs_ctx *ctx, const vs_guided_opts *opts, const vs_pitch_opts *pitch_opts, const int16_t *pcm, size_t pitch,
              size_t n_lanes, size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
              vs_pitch_frame *frames, vs_acoustic *out, int32_t *marks, size_t marks_pitch, vs_guided_rec *rec,
              vs_guided_seg *segs, size_t seg_pitch);

/* ---- source track: a glottal source that follows an F0 contour (csrc/vs_strack.hip) ---------------------------------
 *
 * The source of vs_source with a period -- and, optionally, an amplitude -- that changes along the row: the consumer of
 * what vs_pitch_launch writes (a lag per frame), as the coefficient tracks are the consumer of vs_lpc_launch.  Chained
 * behind the pitch track and in front of vs_track_launch it resynthesises a recording's F0, voicing and formants with
 * jitter, shimmer and closed-phase noise under the caller's control.
 *
 * Per call: max_reject, 1..65536 (default 256).  Per row: a vs_lane that passes vs_lane_validate (F0 and Fg are not read;
 * amp is read only without an amplitude track; the filter fields play no part), a vs_strack_row, period[f] int32 for
 * f in [0, n_frames) and, optionally, amp[f] int32.
 * VS_ERR_RANGE: n_frames < 1 or above frames_pitch; hop < 1; length outside [0, n_samples]; pmin < 2,
 * pmax > VS_AC_MAX_LAG or pmin > pmax; ceil(0.5 * cq * pmin) < 1.  offset may be any int32.
 *
 * 1. Frame of a sample.  f(n) = n < offset ? 0 : min((n - offset) / hop, n_frames - 1), in 64-bit integers.  Frame f is
 *    voiced iff pmin <= period[f] <= pmax and, with an amplitude track, 0 <= amp[f] <= 32766.  Nothing else is trusted:
 *    whatever wrote the arrays, a value outside the range counts as unvoiced.
 *
 * 2. Walk.  g = 0, draw index 0 of the lane's Philox stream (seed), DeltaPer[0] = DeltaShimmer[0] = 0, T4 = 0, no
 *    previous cycle.  While g < length:
 *      f(g) unvoiced: e = offset + f2*hop (64-bit) for the smallest voiced f2 > f(g), capped at length; without such a
 *        frame e = length.  Samples [g, e) are (short)DC, no draw is taken, g = e, the three state values return to 0 and
 *        there is no previous cycle.
 *      else a cycle: P = period[f(g)], A0 = amp[f(g)] (the lane's amp without an amplitude track).
 *        With a previous cycle and P != P_prev:   DeltaPer[0] = (float)((double)DeltaPer[0] * (double)P / (double)P_prev)
 *                                                 and T4 = 0.
 *        With a previous cycle and A0 != A0_prev: DeltaShimmer[0] = A0_prev ? (float)((double)DeltaShimmer[0] *
 *                                                 (double)A0 / (double)A0_prev) : 0.
 *        Then the reference's cycle, flowgen_shimmer.c:248-411, statement by statement, with P and A0 in the places of
 *        P and par.amp: in the jitter and shimmer recursions, in their bounds ((float)1.2*P, (float)0.8*P, (float)1.8*A0,
 *        (float)0.2*A0) and in T2 = ceil(0.5*cq*P).  Without jitter T = P.  NoiseDistWidth is the floor of the root, 0 for
 *        an argument that is NaN or negative zero (T3 == T4 cannot be reached from valid lanes).
 *        One change: a rejection loop that has rejected max_reject draws ends -- jitter with T = P and DeltaPer[0] = 0,
 *        shimmer with Amplitude = A0 and DeltaShimmer[0] = 0 -- and n_resets counts each such end; the draws that were
 *        taken stay taken.  (Without the rescaling an octave step down with small jitter leaves DeltaPer outside 0.2*P
 *        for ever; the cap is what bounds every loop of the kernel by construction.)
 *        The cycle's first min(T, length - g) samples are stored at g; g += T.
 *    Samples past length are not touched.
 *
 * 3. Consequence (held by tests/test_gpu_strack.py): on a track whose every frame holds (int)((float)fs / F0), without
 *    an amplitude track, the rows are vs_source's byte for byte, for every lane in which no loop rejects max_reject draws;
 *    the cycle periods and the draw count agree too.
 *
 * The cos values are the host's (libm, vs_cos_row): one row per T2 that the rows of the call can reach, every T2 in
 * [T2(pmin), T2(pmax)] of each row, uploaded with the row records.
 *
 * Not in this version: no aspiration noise in unvoiced stretches (they are DC); the contour is a staircase per cycle (the
 * period is not interpolated inside a frame); no filter is fused (the flow goes through HBM to vs_track_launch or
 * vs_plan_launch(VS_KIND_FILTER)).
 */
#define VS_ST_NO_VOICED 0x1  /* the row has no cycle */
#define VS_ST_INTERNAL 0x2   /* the launch's error word: the kernel met a T2 without a cos row or a cycle beyond its buffer
                                ("cannot happen"); the row's walk ended there and what it stored is not promised */
#define VS_ST_MAX_REJECT 65536
typedef struct vs_strack_opts {
  int32_t max_reject;  /* 1..VS_ST_MAX_REJECT, default 256 */
  int32_t reserved_;   /* must be 0 */
} vs_strack_opts;      /* 8 bytes */
typedef struct vs_strack_row {
  int32_t n_frames;    /* 1..frames_pitch */
  int32_t hop;         /* samples per frame, >= 1 */
  int32_t offset;      /* frame f governs [offset + f*hop, offset + (f+1)*hop), frame 0 what lies before, the last what lies behind */
  int32_t length;      /* samples of this row, <= n_samples; the rest of the output row is left untouched */
  int32_t pmin, pmax;  /* a period outside [pmin, pmax] is unvoiced; 2 <= pmin <= pmax <= VS_AC_MAX_LAG */
} vs_strack_row;       /* 24 bytes */
typedef struct vs_strack_cycle {
  int32_t start;       /* g of the cycle */
  int32_t T;           /* its period in samples */
  int32_t frame;       /* f(g) */
  int32_t amp;         /* A0 */
  float S, x_pow, w_pow; /* as in vs_cycle_rec */
  int32_t reserved_;
} vs_strack_cycle;     /* 32 bytes */
typedef struct vs_strack_stat {
  int32_t status;      /* VS_ST_* */
  int32_t n_cycles;
  int32_t n_resets;    /* rejection loops ended by max_reject */
  int32_t n_unvoiced;  /* samples of the unvoiced stretches */
  uint64_t n_draws;    /* draws taken: the index of the next one */
} vs_strack_stat;      /* 24 bytes */
int vs_strack_defaults(vs_strack_opts *opts);
/* Host only, no device: the row that plays the frames vs_pitch makes of a row of len samples at rate fs (pitch_opts NULL:
 * vs_pitch_defaults()): n_frames = vs_pitch_frames(), hop = H, offset = C - H/2 with C = tmax + tmax/2, pmin = tmin,
 * pmax = tmax, length = len -- the f(n) of the guided marks.  VS_ERR_RANGE as vs_pitch_frames, and for a row without
 * frames. */
int vs_strack_from_pitch(const vs_pitch_opts *pitch_opts, int32_t fs, int32_t len, vs_strack_row *row);
/* lanes and rows are HOST arrays of n_lanes records; they and the cos rows go up through the context's retired-block
 * cache.  Device pointers: the period of frame f of row i is the int32 at byte (i*frames_pitch + f) * period_stride of
 * period_dev, the amplitude (amp_dev may be NULL) likewise with amp_stride; strides are multiples of 4 and at least 4
 * (period_dev = &frames_dev->lag with stride sizeof(vs_pitch_frame) reads what vs_pitch_launch wrote, with no host
 * round trip).  flow_dev int16 [n_lanes][out_pitch] (out_pitch >= n_samples), stat_dev vs_strack_stat [n_lanes],
 * cycles_dev vs_strack_cycle [n_lanes][cycles_pitch] or NULL: cycle k of row i at cycles_dev[i*cycles_pitch + k] for
 * k < cycles_pitch, later cycles are counted only, slots past n_cycles are untouched.  Enqueued on the context's stream,
 * returns without waiting.  opts NULL: vs_strack_defaults().  NULL pointers, zero sizes, a bad stride, a cycles_dev with
 * cycles_pitch 0, a non-zero reserved_: VS_ERR_ARG; what vs_lane_validate answers for a lane; the VS_ERR_RANGE cases
 * above and max_reject; sizes beyond 2^31: VS_ERR_UNSUPPORTED. */
int vs_strack_launch(vs_ctx *ctx, const vs_strack_opts *opts, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
                     const vs_strack_row *rows, const int32_t *period_dev, size_t period_stride, size_t frames_pitch,
                     const int32_t *amp_dev, size_t amp_stride, int16_t *flow_dev, size_t out_pitch,
                     vs_strack_stat *stat_dev, vs_strack_cycle *cycles_dev, size_t cycles_pitch);
/* Host buffers: period and amp (may be NULL) int32 [n_lanes][frames_pitch], flow int16 [n_lanes][n_samples], stat
 * [n_lanes], cycles [n_lanes][cycles_pitch] or NULL.  Upload (the flow and the cycle records too, so that what lies past a
 * row's length or its cycles stays as it was), vs_strack_launch, download, wait. */
int vs_strack(vs_ctx *ctx, const vs_strack_opts *opts, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
              const vs_strack_row *rows, const int32_t *period, size_t frames_pitch, const int32_t *amp, int16_t *flow,
              vs_strack_stat *stat, vs_strack_cycle *cycles, size_t cycles_pitch);

/* ---- PSOLA: a recording's own cycles, placed at target periods (csrc/vs_psola.hip) -----------------------------------
 *
 * Pitch-synchronous overlap-add.  The source track makes a Fant pulse on a contour; this takes the recording itself,
 * cuts a grain around each analysis mark and puts the grains down at new instants: the F0 or the cycle-to-cycle
 * perturbation changes, the waveform stays the voice's own.  Behind vs_guided_launch (the marks and their runs) and
 * vs_strack_launch (a cycle log with the caller's jitter on the recording's contour) it is one chain on one stream.
 * Everything is an integer.  Q = 32768.
 *
 * Per row: x[0..len) int16, a sample index outside [0, len) reads as 0; the analysis marks a[] int32 as
 * vs_guided_launch or vs_measure_launch wrote them, marks_pitch of them; the row's runs -- run r has the marks
 * a[first .. first + m) with first = segs[r].first_mark_index and m = segs[r].n_marks, for r below rec.n_segments capped
 * at seg_pitch (a negative count is 0); without segs the row is one run with first = 0 and m = rec.n_marks capped at
 * marks_pitch --; a target of J cycles start[j], T[j] and, optionally, gain[j], all int32.  The gain is Q15, 0..65535,
 * Q is unity; a gain outside 0..65535 is a cycle that governs nothing.  J is the row's count capped at target_pitch; a
 * negative count is 0.  Per call: pmin and pmax, 2 <= pmin <= pmax <= VS_AC_MAX_LAG.
 * Output: y[0..len); samples past len are not touched.
 *
 * A run is usable iff m >= 2, 0 <= first and first + m <= marks_pitch, its marks are strictly increasing inside
 * [0, len), no two neighbours are more than VS_AC_MAX_LAG apart, and its first mark is greater than the last mark of
 * the usable run before it.  A run that is not usable is copied and VS_PS_BAD_RUN is set.  With a_0..a_{m-1} the marks
 * of a usable run and E = a_{m-1}:
 *     PR(k) = a_{k+1} - a_k, and a_{m-1} - a_{m-2} for k = m-1;      PL(k) = a_k - a_{k-1}, and a_1 - a_0 for k = 0.
 *
 * A. Synthesis marks of a usable run.  t_0 = a_0, k_0 = 0, no governing cycle before.  At t_i the cycle c is
 *      c' + 1, if the mark before was governed by c', c' + 1 < J and start[c'+1] == start[c'] + T[c'] (64 bits): inside
 *        a contiguous stretch of the target the cycles are taken one by one -- no draw of a jittered target is skipped
 *        or used twice, and the offset to the target's own instants stays what it was at the stretch's first mark;
 *      else the largest c with start[c''] <= t_i for ALL c'' <= c (a prefix scan, defined for any array), and only if
 *        t_i < start[c] + T[c] (64 bits).
 *    Either way c governs only if pmin <= T[c] <= pmax and its gain is valid.  With a governing cycle T_i = T[c] and
 *    g_i = gain[c] (Q without a gain array); without one T_i = PR(k_i) and g_i = Q: where the target is silent the
 *    recording's own period stands.  If E - t_i <= T_i + T_i/2 the next mark is the run's last: t = E, k = m-1, and the
 *    last gap lies in (T_i/2, 3*T_i/2].  Else t_{i+1} = t_i + T_i and k_{i+1} is the index in [k_i, m-1] whose mark
 *    is nearest to t_{i+1}, ties to the smaller.  The first and the last synthesis mark of a run have gain Q: the run
 *    joins what is copied around it.
 *
 * B. Samples.  Outside [a_0, E) of every resynthesised run y[n] = x[n].  For t_i <= n < t_{i+1}: d = n - t_i,
 *    G = t_{i+1} - t_i (<= 3 * VS_AC_MAX_LAG / 2), e = G - d, A = a[k_i], B = a[k_{i+1}],
 *        L  = min(G, PR(k_i)),      wl = d < L  ? Q - d*Q / L         : 0
 *        L' = min(G, PL(k_{i+1})),  wr = e < L' ? (L' - e)*Q / L'     : 0        (integer divisions of non-negatives)
 *        y[n] = clamp_int16((x[A + d]*wl*g_i + x[B - e]*wr*g_{i+1} + 2^29) >> 30)      (64 bits, arithmetic shift)
 *    and n_clipped counts the samples the clamp changed.  Two grains cover every sample; each is a triangle cut at its
 *    own analysis period, so a lowered pitch does not repeat the neighbouring pulse.
 *
 * C. Consequences (held by tests/test_psola_ref.py).  A target that governs nowhere (J = 0) gives t_i = a_i,
 *    wl + wr = Q, both grains read x[n]: y == x byte for byte.  At n = t_i, wl = Q and wr = 0: without gains
 *    y[t_i] == x[a[k_i]], the peak sample survives.  A contiguous target that starts at or before the run is read back
 *    exactly: the differences of the synthesis marks but the last are T[c_0], T[c_0 + 1], ...
 *
 * D. Records.  vs_psola_mark [n_lanes][synth_pitch]: the synthesis marks of the resynthesised runs, one run behind the
 *    other; t strictly increases along a row.  They are what the plan kernel hands the overlap-add kernel and an
 *    output; slots past n_synth are not touched.  cycle is the governing cycle, -1 without one, and VS_PS_RUN_END at a
 *    run's last mark (which looks for no cycle): between that record and the next the samples are copied.
 *    A run that needs more slots than are left is copied: n_synth and n_governed stay where they were before it,
 *    VS_PS_OVERFLOW is set and the later runs of the row are copied too, without a look at them.
 *    vs_psola_stat: n_runs counts the row's runs, n_runs_done the resynthesised ones, n_governed the marks with a
 *    governing cycle; VS_PS_NO_RUN when n_runs_done == 0 (the row is a copy).
 *
 * Not in this entry point: a duration change (y is as long as x and every run keeps its first and last mark; see "PSOLA
 * with a time map" below).  Not in this version: no Hann windows and never more than two grains (a pitch raised by more than 2 leaves out samples between the marks, lowered
 * by more than 2 it leaves zeros); no device-side shimmer gains (vs_strack_cycle does not log the cycle's amplitude:
 * gains are the caller's array); nothing is done to unvoiced stretches, they are copied.
 */
#define VS_PS_BAD_RUN 0x1
#define VS_PS_OVERFLOW 0x2
#define VS_PS_NO_RUN 0x4
#define VS_PS_RUN_END (-2)
typedef struct vs_psola_opts {
  int32_t pmin, pmax;   /* a target period outside [pmin, pmax] governs nothing; 2 <= pmin <= pmax <= VS_AC_MAX_LAG */
  int32_t reserved_[2]; /* must be 0 */
} vs_psola_opts;        /* 16 bytes */
typedef struct vs_psola_mark {
  int32_t t;            /* the synthesis instant */
  int32_t k;            /* the index in the row's mark array of the analysis mark whose grain is placed there */
  int32_t cycle;        /* the governing cycle of the target, -1, or VS_PS_RUN_END */
  int32_t gain;         /* g_i, Q15 */
} vs_psola_mark;        /* 16 bytes */
typedef struct vs_psola_stat {
  int32_t status;       /* VS_PS_* */
  int32_t n_runs, n_runs_done, n_synth, n_governed, n_clipped;
} vs_psola_stat;        /* 24 bytes */
/* pmin = 32, pmax = 320: tmin and tmax of vs_guided_plan for the default F0 range (50..500 Hz) at 16 kHz.  A caller at
 * another rate or range sets them from vs_guided_plan (or from the vs_strack_row that made the target). */
int vs_psola_defaults(vs_psola_opts *opts);
/* Device pointers: pcm_dev int16 [n_lanes][pitch] (pitch >= n_samples), marks_dev int32 [n_lanes][marks_pitch], rec_dev
 * vs_guided_rec [n_lanes], segs_dev vs_guided_seg [n_lanes][seg_pitch] or NULL.  The target is read in place: start[j] of
 * row i is the int32 at byte (i*target_pitch + j) * start_stride of start_dev, T[j] likewise with period_stride, gain[j]
 * (gain_dev may be NULL) with gain_stride, and the row's count is the int32 at byte i * count_stride of count_dev;
 * strides are multiples of 4 and at least 4.  &cycles_dev->start and &cycles_dev->T at stride sizeof(vs_strack_cycle)
 * with &stat_dev->n_cycles at stride sizeof(vs_strack_stat) and target_pitch = cycles_pitch read what vs_strack_launch
 * wrote, with no host round trip.  out_dev int16 [n_lanes][out_pitch] (out_pitch >= n_samples) must not overlap pcm_dev:
 * a grain reads samples that another workgroup may already have replaced.  stat_dev vs_psola_stat [n_lanes], synth_dev
 * vs_psola_mark [n_lanes][synth_pitch].  lengths (NULL: n_samples for every row) is a HOST array and goes up through the
 * context's retired-block cache, which also lends the scratch between the two kernels.  Enqueued on the context's
 * stream, returns without waiting.  opts NULL: vs_psola_defaults().
 * VS_ERR_ARG: NULL pointers, zero sizes, pitch or out_pitch below n_samples, a segs_dev with seg_pitch 0, a stride that
 * is under 4 or no multiple of 4, synth_pitch < 2, a pointer that is not aligned to its items, a non-zero reserved_;
 * VS_ERR_RANGE: pmin, pmax, a length outside [0, n_samples]; VS_ERR_UNSUPPORTED: sizes beyond 2^31. */
int vs_psola_launch(vs_ctx *ctx, const vs_psola_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                    size_t n_samples, const int32_t *lengths, const int32_t *marks_dev, size_t marks_pitch,
                    const vs_guided_rec *rec_dev, const vs_guided_seg *segs_dev, size_t seg_pitch,
                    const int32_t *start_dev, size_t start_stride, const int32_t *period_dev, size_t period_stride,
                    const int32_t *gain_dev, size_t gain_stride, const int32_t *count_dev, size_t count_stride,
                    size_t target_pitch, int16_t *out_dev, size_t out_pitch, vs_psola_stat *stat_dev,
                    vs_psola_mark *synth_dev, size_t synth_pitch);
/* Host buffers: pcm [n_lanes][pitch], marks [n_lanes][marks_pitch], rec [n_lanes], segs [n_lanes][seg_pitch] or NULL,
 * start, period and gain (may be NULL) int32 [n_lanes][target_pitch], count int32 [n_lanes], out int16
 * [n_lanes][n_samples], stat [n_lanes], synth [n_lanes][synth_pitch].  Upload (out and synth too, so that what lies past
 * a row's length or its synthesis marks comes back as it went), vs_psola_launch, download, one wait. */
int vs_psola(vs_ctx *ctx, const vs_psola_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
             const int32_t *lengths, const int32_t *marks, size_t marks_pitch, const vs_guided_rec *rec,
             const vs_guided_seg *segs, size_t seg_pitch, const int32_t *start, const int32_t *period,
             const int32_t *gain, const int32_t *count, size_t target_pitch, int16_t *out, vs_psola_stat *stat,
             vs_psola_mark *synth, size_t synth_pitch);

/* ---- PSOLA with a time map: the duration changes too (csrc/vs_psola_ts.hip) -------------------------------------------
 *
 * The other half of TD-PSOLA.  "PSOLA" above re-times the cycles and leaves every run where it was; here a map from
 * output time to input time says which grain is due at an output instant: a grain is repeated where time is
 * stretched and left out where it is compressed, and the synthesis marks are stepped as above, so the pitch is still the
 * target's or the recording's own.  Unvoiced stretches get marks too.  Everything is an integer; Q, x, the marks, the
 * runs, "usable", PR, PL, the target, J, pmin and pmax are those of "PSOLA", whose stages A and B are referred to.
 *
 * Per row, in addition: an output length len_out in [0, out_samples] and a map of W anchors (u_j, v_j), int32, read
 * from vs_psola_anchor [n_lanes][map_pitch] with the row's W in an int32 per row.  The map is valid iff
 * 2 <= W <= map_pitch, u_0 = v_0 = 0, u_{W-1} = len_out, v_{W-1} = len, u strictly increases and v does not decrease
 * (so len_out = 0 has no valid map).  For u_j <= n < u_{j+1}
 *     M(n) = v_j + floor((n - u_j) * (v_{j+1} - v_j) / (u_{j+1} - u_j))                                       (64 bits)
 * and Minv(p) is the smallest n in [0, len_out] with M(n) >= p, where M(len_out) counts as reached; Minv(0) = 0 and
 * Minv(len) = len_out by definition (also where a frozen piece, v_j = v_{j+1}, reaches len earlier).  An invalid map
 * sets VS_PS_BAD_MAP: y[0..len_out) is 0, n_synth is 0 and no run is looked at.
 * THE TARGET IS IN OUTPUT TIME: start[c] is compared with synthesis instants.
 * Per call, in addition: the unvoiced period U, 2 <= U <= 2 * VS_AC_MAX_LAG / 3 = 1365.  The intervals between the
 * marks of an unvoiced stretch (step 1) are U or lie in (U/2, U + U/2] or are a whole gap of at most U + U/2 samples:
 * at most 1365 + 682 = 2047 <= VS_AC_MAX_LAG, like a usable run's.  A synthesis step T_i is a target period
 * (<= pmax <= VS_AC_MAX_LAG) or an analysis interval, and a stretch's last gap is at most T_i + T_i/2: every synthesis
 * interval G is at most 3 * VS_AC_MAX_LAG / 2, as in stage B.
 * Output: y[0..len_out); samples past len_out are not touched.
 *
 * 1. The row is a chain of stretches that covers [0, len].  A VOICED stretch is the marks of a usable run (a run that is
 *    not usable sets VS_PS_BAD_RUN and its span is unvoiced).  An UNVOICED stretch fills every gap [g0, g1) of positive
 *    length: g0 is 0 or the E of the usable run before, g1 the a_0 of the next usable run or len.  Its marks are
 *    p_0 = g0, p_{i+1} = p_i + U while g1 - p_i > U + U/2, then g1.  With b_0..b_{m-1} the marks of a stretch (m >= 2),
 *    PR and PL are taken inside the stretch with the end rules of "PSOLA".  A row with len = 0 has no stretch.
 *
 * 2. Synthesis marks of a stretch.  t_s = Minv(b_0), t_e = Minv(b_{m-1}); a stretch with t_e <= t_s has no marks.  Else
 *    stage A with t_0 = t_s, k_0 = 0, no governing cycle before, and
 *      (a) t_e where stage A has E: if t_e - t_i <= T_i + T_i/2 the next mark is the stretch's last, at t_e with k = m-1;
 *      (b) k_{i+1} is the index in [k_i, m-1] whose mark is nearest to M(t_{i+1}), ties to the smaller;
 *      (c) a cycle can govern only in a voiced stretch; in an unvoiced one T_i = PR(k_i), g_i = Q and the target is not
 *          looked at;
 *      (d) in an unvoiced stretch a mark whose k is the k of the mark before has flip = !flip of that mark, every other
 *          mark has flip = 0: a repeated noise grain is played backwards every other time and does not turn tonal.
 *    The stretches with marks share their boundary marks: the last mark of one is the first mark of the next (Minv does
 *    not decrease, so a stretch without marks between them has t_e = t_s).  Along a row t starts at 0, ends at len_out
 *    and strictly increases.  A boundary mark has gain Q and flip 0.
 *
 * 3. Samples.  Stage B for every t_i <= n < t_{i+1} of every stretch with marks, with A = b[k_i] and PR(k_i) of the
 *    stretch of the interval, B = b[k_{i+1}] and PL(k_{i+1}) likewise (a boundary mark is the right grain of the stretch
 *    before it with that stretch's last mark and PL, the left grain of the stretch behind it with that stretch's first
 *    mark and PR).  A flipped left grain reads x[A - d] for x[A + d], a flipped right grain x[B + e] for x[B - e].
 *    There are no copy regions: every sample of y[0..len_out) is the sum of two grains.  A row without marks (len = 0,
 *    an invalid map, an overflow) has y[0..len_out) = 0.
 *
 * 4. Consequences (held by tests/test_psola_ts_ref.py).  With the identity map (len_out = len, two anchors) y and
 *    n_clipped are those of vs_psola_launch for ANY target and any U (an unvoiced stretch has t_i = p_i, wl + wr = Q and
 *    both grains read x[n]; a run's marks are stage A's).  With the identity map and J = 0, y == x.  With any valid map
 *    and no governing cycle the voiced marks step by the recording's own periods: the duration changes, the pitch does
 *    not.  A contiguous target that starts at or before a voiced stretch's t_s is read back exactly.
 *
 * 5. Records.  One vs_psola_mark per synthesis mark, a boundary is ONE record.  t as above.  k: in a voiced stretch the
 *    index in the row's mark array, in an unvoiced stretch the index i of p_i inside the stretch; a boundary has the k of
 *    its left grain (the first mark of the stretch behind it), the row's last record the k of its right grain.  cycle:
 *    in a voiced stretch the governing cycle or -1; in an unvoiced one VS_PS_UNVOICED, or VS_PS_UNVOICED_FLIP with
 *    flip = 1; a boundary as the first mark of the stretch behind it; VS_PS_RUN_END at the row's last record.
 *    vs_psola_stat keeps its meaning: n_runs the row's runs, n_runs_done the usable ones (with or without marks),
 *    n_governed the marks with a governing cycle, VS_PS_NO_RUN when n_runs_done == 0.  A row whose marks do not fit
 *    synth_pitch sets VS_PS_OVERFLOW: n_synth and n_governed are 0 and y[0..len_out) is 0; nothing is stored past the
 *    count.  With VS_PS_BAD_MAP n_runs is still the row's, every other count is 0 and VS_PS_NO_RUN is set.
 *
 * Not in this version: Hann windows and more than two grains; a map made on the device; device-side shimmer gains;
 * aspiration noise.
 */
#define VS_PS_BAD_MAP 0x8
#define VS_PS_UNVOICED (-3)
#define VS_PS_UNVOICED_FLIP (-4)
typedef struct vs_psola_ts_opts {
  int32_t pmin, pmax;      /* as in vs_psola_opts */
  int32_t unvoiced_period; /* U, 2 .. 2 * VS_AC_MAX_LAG / 3 */
  int32_t reserved_;       /* must be 0 */
} vs_psola_ts_opts;        /* 16 bytes */
typedef struct vs_psola_anchor {
  int32_t u, v;            /* output instant u is input instant v */
} vs_psola_anchor;         /* 8 bytes */
/* pmin = 32, pmax = 320 (vs_psola_defaults), unvoiced_period = 80: 5 ms at 16 kHz. */
int vs_psola_ts_defaults(vs_psola_ts_opts *opts);
/* Device pointers.  pcm_dev .. target_pitch: as in vs_psola_launch.  map_dev vs_psola_anchor [n_lanes][map_pitch] and
 * map_count_dev int32 [n_lanes], the row's W: a later stage can make the map on the device.  out_dev int16
 * [n_lanes][out_pitch] (out_pitch >= out_samples) must not overlap pcm_dev.  lengths (NULL: n_samples for every row) and
 * out_lengths (NULL: out_samples for every row) are HOST arrays and go up in the row record through the context's
 * retired-block cache, which also lends the scratch between the two kernels.  The overlap-add kernel has 5136 bytes of
 * static LDS.  Enqueued on the context's stream, returns without waiting.  opts NULL: vs_psola_ts_defaults().
 * VS_ERR_ARG: as vs_psola_launch, and: out_samples or map_pitch 0, map_pitch < 2, out_pitch below out_samples, NULL
 * map pointers, out_dev's rows overlapping pcm_dev's; VS_ERR_UNSUPPORTED: sizes beyond 2^31; VS_ERR_RANGE: pmin, pmax,
 * unvoiced_period, a length outside [0, n_samples], an output length outside [0, out_samples]. */
int vs_psola_ts_launch(vs_ctx *ctx, const vs_psola_ts_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                       size_t n_samples, const int32_t *lengths, const int32_t *marks_dev, size_t marks_pitch,
                       const vs_guided_rec *rec_dev, const vs_guided_seg *segs_dev, size_t seg_pitch,
                       const int32_t *start_dev, size_t start_stride, const int32_t *period_dev, size_t period_stride,
                       const int32_t *gain_dev, size_t gain_stride, const int32_t *count_dev, size_t count_stride,
                       size_t target_pitch, const vs_psola_anchor *map_dev, const int32_t *map_count_dev,
                       size_t map_pitch, int16_t *out_dev, size_t out_pitch, size_t out_samples,
                       const int32_t *out_lengths, vs_psola_stat *stat_dev, vs_psola_mark *synth_dev, size_t synth_pitch);
/* Host buffers: as vs_psola, and: map [n_lanes][map_pitch], map_count int32 [n_lanes], out int16
 * [n_lanes][out_samples].  Upload (out and synth too), vs_psola_ts_launch, download, one wait. */
int vs_psola_ts(vs_ctx *ctx, const vs_psola_ts_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes,
                size_t n_samples, const int32_t *lengths, const int32_t *marks, size_t marks_pitch,
                const vs_guided_rec *rec, const vs_guided_seg *segs, size_t seg_pitch, const int32_t *start,
                const int32_t *period, const int32_t *gain, const int32_t *count, size_t target_pitch,
                const vs_psola_anchor *map, const int32_t *map_count, size_t map_pitch, int16_t *out, size_t out_samples,
                const int32_t *out_lengths, vs_psola_stat *stat, vs_psola_mark *synth, size_t synth_pitch);

/* Library version string. */
const char *vs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VOICE_SYNTH_H */
