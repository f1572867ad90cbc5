/*
 * vs_synth_one_wave.hip -- gfx950 (MI355X) kernels of the batched vowel synthesiser: the one-wave kernel, and what all
 * the synthesis kernels have in common.
 *
 * Mapping: ONE UTTERANCE PER LANE, 64 utterances per group.  A group is served either by one
 * wavefront that alternates between generating and filtering (vs_synth_kernel) or by a generator
 * wavefront and a filter wavefront (vs_synth_ws_kernel, the default for the fused kind).  Either
 * way the work is CYCLE-MAJOR: lanes do not share a sample clock.  Each lane owns a column of
 * an int16 ring in LDS (layout [slot][lane], 128 B per slot; a lane only ever touches its own
 * column) and its own position n in its own utterance.  The two kinds of work:
 *
 *   generator round (reference flowgen_shimmer.c:246-423): every lane with room produces its
 *       next glottal cycle -- jitter / shimmer recursions with their rejection loops, rising
 *       and falling half-pulse from a host-built cos table (staged in LDS), closed phase,
 *       closed-phase noise from a counter-based Philox stream (4 draws per block) -- and
 *       appends T samples to its ring column.  All lanes walk the SAME phase of their own
 *       cycle together, so branches stay nearly wave-uniform although every lane has its own
 *       period, amplitude and draw counter; and
 *
 *   filter super-steps (reference vowel_new.c:266-289): while a lane holds >= 24 buffered flow
 *       samples it runs 24 steps of the order-22 all-pole recurrence in fp64.  The state
 *       y[n-1..n-22] lives in a rotating window of 24 double registers (no shifting, no LDS);
 *       the 24 int16 results leave as three 16-byte stores per lane at that lane's own n.
 *       The flow itself never reaches HBM.
 *
 * Next to them, each in a file of its own: vs_out_noise.hip (vowel -n, second half), vs_filter_wide.hip (explicit
 * coefficient sets of 23..40 taps: the same recurrence on a 48-sample window, reading a flow row
 * from HBM -- the un-fused path), vs_selftest.hip (the arithmetic shortcuts against their
 * literal forms, on the device).
 *
 * No MFMA: the path is a scalar recurrence per utterance, not a contraction -- and the block form that would make
 * it one (16 samples x 16 utterances per tile, 40 multiply-adds per sample instead of 22) loses on gfx950, whose
 * fp64 matrix instructions run at the vector rate on the vector issue port (tools/ubench/ubench6.hip).
 *
 * Arithmetic contract: these files are compiled with -ffp-contract=off.  VS_ARITH_EXACT keeps
 * the reference's rounding sequence operation by operation (mul, then sub, j = 1..22), so the
 * double state is bit-identical to the C reference; VS_ARITH_FMA is the explicit, opt-in
 * fused variant.  IEEE fp64 mul/add/fma/div and fp32 mul/add/div are correctly rounded on
 * gfx950 (HIP's default -fhip-fp32-correctly-rounded-divide-sqrt is kept); cos() values come
 * from the host libm table; the device sqrt() only seeds an exact fix-up (an integer search in
 * the source, one exact Newton test in the output-noise kernel).
 */
#include "vs_kernel_table.h"
#include "vs_dev_generator.h"
#include "vs_dev_filter.h"

template <int ARITH, int KIND, bool LOG, bool PRE1>
__global__ void __launch_bounds__(VS_WAVE) vs_synth_kernel(VsKernelArgs args)
{
  extern __shared__ __attribute__((aligned(16))) int16_t ring[];

  const int lane = (int)threadIdx.x;
  const long gl = (long)blockIdx.x * VS_GROUP_LANES + lane;
  const bool valid = (lane < VS_GROUP_LANES) && (gl < (long)args.n_lanes);
  const VsDevLane *__restrict__ L = args.lanes + (valid ? gl : (long)args.n_lanes - 1);
  const int N = args.n_samples;
  const int C = args.ring_slots;

  /* filter constants and state in registers */
  double a[VS_ORDER + 1];
  double y[VS_SS];
  vs_load_taps<ARITH>(args.taps, L, a);
#pragma unroll
  for (int j = 0; j < VS_SS; ++j) y[j] = 0.0; /* vowel_new.c:222-224 */
  const double gain = L->gain;
  const double pre = L->pre;
  const long row = (long)L->row;
  /* the group's super-step threshold (the same in all its lanes), unless the launch sets one */
  const int ready_min = (args.ready_min > 0) ? args.ready_min : __builtin_amdgcn_readfirstlane(L->ready_min);

  VsCfg c;
  VsGen s;
  double *ltab = (double *)(ring + (size_t)(C + VS_TRASH_ROWS) * VS_GROUP_LANES); /* slots [C, C+8) are the trash rows */
  bool uni = false; /* a uniform group (vs_dev_generator.h) */
  if (KIND != VS_KIND_FILTER) {
    vs_load_cfg(L, c, s);
    uni = vs_stage_cos_rows<!LOG>(L, c, ltab, args.costab, args.ltab_entries, lane, valid, args);
    __syncthreads(); /* single-wave workgroup: orders the staging writes before the row reads */
  }
  vs_cycle_rec *logrow = nullptr;
  if (LOG && args.log) logrow = (vs_cycle_rec *)args.log + row * args.log_pitch;

  int16_t *__restrict__ orow = args.out + row * args.out_pitch;
  const int16_t *__restrict__ irow = (KIND == VS_KIND_FILTER) ? args.in + row * args.in_pitch : nullptr;

  VsDiag dg;
#ifdef VS_DIAG
#pragma unroll
  for (int k = 0; k < 8; ++k) dg.acc[k] = 0;
  dg.t = vs_stamp();
#endif
  vs_u32x4 xpre[VS_SS / 8]; /* filter-only kind: the next super-step's input, loaded ahead */
  if (KIND == VS_KIND_FILTER && valid && args.vec_ok && VS_SS <= N) {
#pragma unroll
    for (int k = 0; k < VS_SS / 8; ++k) xpre[k] = *(const vs_u32x4 *)(irow + 8 * k);
  }
  int n = 0;     /* this lane's position in its own utterance */
  int rslot = 0; /* ring slot of sample n */
  bool live = valid;
  /* Scheduling: a super-step costs the same whether 1 or 64 lanes take
   * part, and so does a generator round.  Run a super-step when at least ready_min/64 of the
   * live lanes hold 24 samples; otherwise let every lane with room produce its next cycle
   * (the lanes that are short always have room).  Lanes whose periods run long fill their
   * ring and sit rounds out -- they have fewer cycles to produce anyway.
   * A lane's scalar draws for cycle k+1 are made right behind the samples of cycle k, inside the
   * generator branch: the room check needs the period, and the generator's constants are then
   * not live across the super-step (which needs every register it can get). */
  if (KIND != VS_KIND_FILTER) {
    if (live && (s.g < N)) vs_cycle_scalars(c, s, dg); /* fixes the first period s.T */
  }
  while (__any(live)) {
    bool ready = live;
    if (KIND != VS_KIND_FILTER) {
      ready = live && ((s.g - n >= VS_SS) || (s.g >= N));
      /* room for the whole cycle plus the 8 slots a trip of the short sequences may run past it */
      const bool want = live && s.pend && (s.g - n + s.T + VS_TRASH_ROWS <= C);
      const int n_live = __builtin_popcountll(__ballot(live));
      const int n_ready = __builtin_popcountll(__ballot(ready));
      const bool filter_now = (n_ready > 0) && ((n_ready * 64 >= n_live * ready_min) || !__any(want));
      if (!filter_now) {
        if (want) {
          vs_cycle_emit<LOG>(c, s, ring, C, lane, N, ltab, uni, args.costab, logrow, (int)args.log_pitch, dg);
          if (s.g < N) vs_cycle_scalars(c, s, dg); /* the next period */
        }
        continue;
      }
    }

    /* ---- filter super-steps: a lane runs while it holds 24 buffered samples (or its tail) ---- */
    if (ready) {
      int outv[VS_SS];
      vs_superstep<ARITH, KIND, PRE1>(a, y, gain, pre, ring + rslot * VS_GROUP_LANES + lane, irow, orow, n, N,
                                      args.vec_ok != 0, outv, xpre);
      if (KIND != VS_KIND_FILTER) {
        rslot += VS_SS;
        if (rslot >= C) rslot = 0;
      }
      n += VS_SS;
      if (n >= N) live = false;
    }
    VS_DIAG_ADD(dg, 6)
  }
#ifdef VS_DIAG
  if (args.diag && lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) args.diag[(size_t)blockIdx.x * 8 + k] = dg.acc[k];
  }
#endif

  if (KIND != VS_KIND_FILTER && args.ncyc && valid) args.ncyc[row] = s.cyc;
}

/* The table of this build: 64 utterances per wavefront, or the narrow build's 16 (the kernel's own name differs too:
 * vs_dev_primitives.h).  <ARITH, KIND, LOG, PRE1>.  The source kind always runs exact and without PRE1, and only the exact
 * filter has a PRE1 form; the filter kind keeps no log (pick_one_wave, vs_planhost.c, asks for LOG = false whatever it is told). */
#if VS_GROUP_LANES == VS_WAVE
#define VS_ONE_WAVE_FAMILY VS_KF_ONE_WAVE
#define VS_ONE_WAVE_TABLE vs_kernel_table_one_wave
#else
#define VS_ONE_WAVE_FAMILY VS_KF_NARROW
#define VS_ONE_WAVE_TABLE vs_kernel_table_narrow
#endif
#define VS_E_ONE_WAVE(A, K, L, P) {VS_KERNEL_ID(VS_ONE_WAVE_FAMILY, A, K, L, P), vs_synth_kernel<A, K, L, P>}
#define VS_E_ONE_WAVE_LOGS(A, K, P) VS_E_ONE_WAVE(A, K, false, P), VS_E_ONE_WAVE(A, K, true, P)
#define VS_ONE_WAVE_ENTRIES                                                                                               \
  VS_E_ONE_WAVE_LOGS(VS_ARITH_EXACT, VS_KIND_SYNTH, false), VS_E_ONE_WAVE_LOGS(VS_ARITH_EXACT, VS_KIND_SYNTH, true),       \
      VS_E_ONE_WAVE_LOGS(VS_ARITH_EXACT, VS_KIND_SOURCE, false), VS_E_ONE_WAVE_LOGS(VS_ARITH_FMA, VS_KIND_SYNTH, false),    \
      VS_E_ONE_WAVE(VS_ARITH_EXACT, VS_KIND_FILTER, false, false), VS_E_ONE_WAVE(VS_ARITH_EXACT, VS_KIND_FILTER, false, true), \
      VS_E_ONE_WAVE(VS_ARITH_FMA, VS_KIND_FILTER, false, false)
const VsKernelEntry VS_ONE_WAVE_TABLE[] = {VS_ONE_WAVE_ENTRIES, {0, nullptr}};
